/* include/lsq_hip_pack.h -- export of group-wise LSQ weights as packed 4- / 2-bit codes on gfx950, and the way back.
 *
 * Exported by `liblsq_hip_pack.so` (built from lsqfakequantize-pytorch_amd/csrc/pack/ for gfx950), a companion of
 * `liblsq_hip.so` and `liblsq_hip_group.so`: their ABIs (include/lsq_hip.h version 6, include/lsq_hip_group.h version 2)
 * are unchanged, this header only borrows lsq_params, the dtype codes and the status codes of lsq_hip.h, and the library
 * imports no lsq_hip_* / lsq_group_* symbol.  Same contract as lsq_hip.h: caller-owned device buffers, kernels enqueued on
 * `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation, no environment variables,
 * no mutable global state, 0 / negative LSQ_E* / positive hipError_t returns, never throws; lsq_pack_last_error() describes
 * the calling thread's last failure.
 *
 * THE FORMAT (the contract between lsq_pack_quantize, lsq_pack_dequantize, lsq_pack_unpack and any other reader):
 *  - `bits` is 4 or 2, and quant_max - quant_min <= 2^bits - 1.
 *  - x is `n` dense elements; group j is elements [j * G, (j + 1) * G), n % G == 0 (the layout of lsq_hip_group.h).
 *  - The code of an element is c = level - quant_min, 0 <= c <= 2^bits - 1, where `level` is exactly the integer level
 *    lsq_group_forward emits with aux_kind 0: rne(clamp(x * (1 / s) + zp, quant_min, quant_max)); a NaN x lands on
 *    quant_min (code 0) as there.
 *  - The codes are a row-major flat bit stream, little-endian inside the byte: element i occupies bits
 *    [(i mod (8 / bits)) * bits, + bits) of byte i * bits / 8.  For 4 bits, element 0 is the LOW nibble of byte 0.
 *    n * bits / 8 bytes in all.
 *  - G % (8 / bits) == 0 is required, so every group -- and with it every row of a [rows, K] weight with K % G == 0 --
 *    starts on a byte boundary.
 *  - Per group, next to the codes:
 *      qscale = fmax(eps, |scale|)                       float (double for F64 storage); eps = FLT_ / DBL_EPSILON
 *      qzero  = zp - quant_min                            int32: the zero point in code units, with
 *               zp = rne(clamp(-shift * (1 / qscale), type_min, type_max)), the zero point of the group-wise forward.
 *  - Dequantization is y = (T(c) - T(qzero)) * qscale in the arithmetic type T (float; double for F64), rounded to the
 *    storage type as the forward rounds its result.  c - qzero == level - zp and both differences are exact small
 *    integers (lsq_pack_quantize rejects ranges beyond +-2^23), so y carries the bits of lsq_group_forward's y for all four
 *    storage types -- with one exception, the sign of a zero, which codes cannot carry.  With quant_min < 0 an
 *    x * (1 / s) + zp in [-0.5, 0) rounds to the level -0.0, and the forward's (-0.0 - zp) * s is -0.0 when zp is +0.0, where
 *    (c - qzero) * qscale is +0.0.  So: y is bit-identical to the forward's iff quant_min >= 0 or the group's zp is not +0.0.
 *    zp is +0.0 exactly when -shift * (1 / qscale) lies in [+0.0, 0.5]; that INCLUDES shift = -0.0.  A shift of +0.0 gives
 *    zp = -0.0 and a zero point that rounds to a non-zero integer is safe too.  Everywhere the values are equal as numbers.
 */
#ifndef LSQ_HIP_PACK_H_
#define LSQ_HIP_PACK_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_PACK_ABI_VERSION 1

/* LSQ_PACK_ABI_VERSION the library was built with. */
int lsq_pack_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_pack_last_error(void);

/* One pass over x: writes the n * bits / 8 bytes of `codes` and the n / G values of `qscale` (float; double for F64) and
 * `qzero` (int32).  scale / shift as in lsq_group_forward (n / G values each).  x must be element-aligned (16-byte alignment
 * is not needed); `codes` may sit at any byte offset (a codes pointer that is not aligned to the bytes one lane writes takes
 * the byte form).  Of `p` the four range fields are read, each within +-2^23; p->numel_for_scaler must be 0. */
int lsq_pack_quantize(int dtype, const void* x, int64_t n, int64_t group_size, const void* scale, const void* shift,
                      const lsq_params* p, int bits, void* codes, void* qscale, void* qzero, void* stream);

/* codes -> the fake-quantized values y (n elements of `dtype`, element-aligned).  `codes` may sit at any byte offset (a
 * pointer that is not aligned to the code bytes of one 16-byte packet of y takes the element form). */
int lsq_pack_dequantize(int dtype, const void* codes, int64_t n, int64_t group_size, int bits, const void* qscale,
                        const void* qzero, void* y, void* stream);

/* codes -> one byte per element: (c + quant_min - level_bias) mod 256, the byte lsq_group_forward writes for
 * (level_bias, aux_kind 0).  n % (8 / bits) == 0; [quant_min, quant_min + 2^bits - 1] - level_bias must fit int8 or uint8.
 * Any alignment of `codes` and `levels` (16 elements per lane when codes is 8-byte and levels 16-byte aligned, one code
 * byte per lane otherwise). */
int lsq_pack_unpack(const void* codes, int64_t n, int bits, int quant_min, int level_bias, void* levels, void* stream);

/* Host only, nothing is launched: the launches of the three ops for (dtype, n, group_size, bits) on the current device (256
 * compute units are assumed when there is none) with aligned buffers.  out8 = [quantize grid, dequantize grid, unpack grid,
 * workgroup size, quantize form (1 = 16-byte packets of x, one group per lane; 0 = one code byte per lane), dequantize form
 * (1 = 16-byte packets of y; 0 = per element), elements per lane of the quantize packet form, elements per packet of y]. */
int lsq_pack_plan(int dtype, int64_t n, int64_t group_size, int bits, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
