/* include/lsq_hip_eltwise_w8.h -- elementwise ops on 8-bit LEVELS on gfx950: a 256-entry byte table (every activation function of
 * a per-tensor 8-bit input is a map from bytes to bytes) and the squeeze-and-excitation multiply x * gate with the next
 * quantizer's levels out.  What keeps a converted MobileNetV3 / EfficientNet / ConvNeXt block in levels at its activations and
 * at its SE gate.
 *
 * Exported by `liblsq_hip_eltwise_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/eltwise_w8/ for gfx950), the fourteenth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h, and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device buffers, kernels
 * enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation, no environment
 * variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is validated before anything is
 * enqueued; lsq_eltwise_w8_last_error() describes the calling thread's last failure.
 *
 * THE TABLE OP.  x is n >= 1 bytes at any byte offset, table 256 bytes on the device, y n bytes at any byte offset:
 *     y[i] = table[x[i]]            the index is the BYTE as stored: an int8 level l reads entry l & 0xff
 * The kernel knows no level dtype, quantizer or function; `table[x.long()]` is the whole definition.  (The package builds the
 * table from existing ops: dequantize the 256 bytes, apply the function, take the next quantizer's levels.)
 *
 * THE GATE MULTIPLY.  x is [B, H, W, C] bytes (channels-last) of x_dtype, g is [B, C] bytes of g_dtype (LSQ_ELTWISE_W8_U8:
 * 0..255, LSQ_ELTWISE_W8_I8: -128..127, the two independent), y is [B, H, W, C]; all dense, at any byte offset (a floating y:
 * element-aligned).  H = W = 1 is the same-shape product of two [B, C] tensors.  With s_x, zx, s_g, zg ONE float32 / int32 each
 * on the device, read in the kernel as they are, and `mid` = mul->mid_dtype (LSQ_F32: identity, LSQ_BF16, LSQ_F16):
 *     a = float(round_to(mid, (float(lx) - float(zx)) * s_x))          fp32 subtract, one rounded fp32 multiply, one rounding
 *     g = float(round_to(mid, (float(lg[b, c]) - float(zg)) * s_g))
 *     t = float(round_to(mid, a * g))                                  one rounded fp32 multiply, never contracted
 *     with out_scale:  q = level(t; out),  y = q mod 256               lsq_math.hpp's level() with make_qparams(
 *                                                                      sanitize_scale_per_tensor(out_scale[0]), out_shift[0],
 *                                                                      range); a NaN goes to quant_min
 *     without:         y = round_to(mid, a * g), stored as mid
 * No atomics; launches repeat bit for bit; an output depends on its own byte, its image's gate byte for its channel and the
 * constants alone; the GPU result equals the package's CPU path (the existing ops composed) bit for bit.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued).  Table op: a NULL x, table or y; n < 1; y overlapping x; table
 * overlapping y.  Gate multiply: a NULL shape, constants, x, g or y; NULL or misaligned s_x, zx, s_g, zg, out_scale, out_shift
 * (out_scale and out_shift come together); a level dtype that is not LSQ_ELTWISE_W8_U8 / _I8; a mid_dtype that is not LSQ_F32 /
 * LSQ_BF16 / LSQ_F16; a floating y that is not element-aligned; B, C, H or W < 1; an extent beyond 29 bits; shapes beyond 64-bit
 * offsets; an output range that is empty or lies neither within 0..255 nor within -128..127; y overlapping x or g; a NULL out8.
 */
#ifndef LSQ_HIP_ELTWISE_W8_H_
#define LSQ_HIP_ELTWISE_W8_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_ELTWISE_W8_ABI_VERSION 1
#define LSQ_ELTWISE_W8_U8 0
#define LSQ_ELTWISE_W8_I8 1
/* out8[0] of the plans */
#define LSQ_ELTWISE_W8_GENERIC 0         /* one lane per byte */
#define LSQ_ELTWISE_W8_PACKETS 1         /* 16-byte packets */

/* The shape of one gate multiply: x and y [B, H, W, C], g [B, C]. */
typedef struct lsq_eltwise_w8_shape {
    int64_t B, C, H, W;
} lsq_eltwise_w8_shape;

/* The gate multiply's constants: `s_x`, `s_g` one float32 and `zx`, `zg` one int32 each ON THE DEVICE, read in the kernel as
 * they are; `out_scale` and `out_shift` one float32 each on the device, or both NULL for a floating y of mid_dtype. */
typedef struct lsq_eltwise_w8_mul {
    const void* s_x;
    const void* zx;
    const void* s_g;
    const void* zg;
    const void* out_scale;
    const void* out_shift;
    int64_t quant_min, quant_max, type_min, type_max, mid_dtype;
} lsq_eltwise_w8_mul;

/* LSQ_ELTWISE_W8_ABI_VERSION the library was built with. */
int lsq_eltwise_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_eltwise_w8_last_error(void);

/* The table op: y[i] = table[x[i]] for i < n. */
int lsq_eltwise_w8_lut(const void* x, const void* table, int64_t n, void* y, void* stream);

/* The gate multiply: y [B, H, W, C] bytes (uint8 for an output range in 0..255, int8 for one in -128..127) or mid_dtype floats. */
int lsq_eltwise_w8_mul_gate(int x_dtype, const void* x_levels, int g_dtype, const void* g_levels, const lsq_eltwise_w8_shape* shape,
                            const lsq_eltwise_w8_mul* mul, void* y, void* stream);

/* Host only, nothing is launched.  `aligned`: x and y are 16-byte aligned.
 * out8[0] = the kernel family (LSQ_ELTWISE_W8_*): PACKETS needs `aligned` and n >= 16, every other legal call is GENERIC;
 * out8[1] = workgroups, out8[2] = threads per workgroup, out8[3] = 16-byte packets per lane P (PACKETS: 2, halved while the grid
 * holds fewer than two workgroups per compute unit; the n % 16 last bytes are served by the first workgroup of the same launch),
 * out8[4] = LDS bytes (PACKETS: the table, 256), out8[5] = packets (n / 16), out8[6] = tail bytes (n % 16), out8[7] = 0. */
int lsq_eltwise_w8_plan_lut(int64_t n, int aligned, int32_t* out8);

/* The same for the gate multiply.  `aligned`: x, g and y are 16-byte aligned.  PACKETS needs C % 16 == 0 and `aligned`: a lane
 * owns one 16-channel packet position (b, c0), dequantizes its 16 gate values once and walks out8[3] pixels with them (4,
 * halved while the grid holds fewer than two workgroups per compute unit, and never more than H W); GENERIC: one lane per
 * element.  out8[1] = workgroups, out8[2] = threads per workgroup, out8[3] = pixels per lane, out8[4] = LDS bytes (0),
 * out8[5] = lanes per image (PACKETS: C / 16 * ceil(H W / pixels per lane); at most 2^31 - 1 is reported), out8[6] = out8[7] = 0. */
int lsq_eltwise_w8_plan_mul(const lsq_eltwise_w8_shape* shape, int aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
