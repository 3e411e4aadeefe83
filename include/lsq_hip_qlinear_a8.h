/* include/lsq_hip_qlinear_a8.h -- W4A8 / W2A8 decode linear on gfx950: 8-bit activation LEVELS times packed 4- / 2-bit
 * group-wise weight codes, summed in integers.
 *
 * Exported by `liblsq_hip_qlinear_a8.so` (built from lsqfakequantize-pytorch_amd/csrc/qlinear_a8/ for gfx950), the fifth
 * companion of `liblsq_hip.so`: the ABIs of include/lsq_hip.h, lsq_hip_group.h, lsq_hip_pack.h and lsq_hip_qlinear.h are
 * unchanged, this header only borrows the dtype codes and the status codes of lsq_hip.h, and the library imports no symbol
 * of the other four.  Same contract as lsq_hip.h: caller-owned device buffers, kernels enqueued on `stream` (a hipStream_t
 * as void*, NULL = the default stream), no allocation, no synchronisation, no environment variables, 0 / negative LSQ_E* /
 * positive hipError_t returns, never throws, everything is validated before anything is enqueued;
 * lsq_qlinear_a8_last_error() describes the calling thread's last failure.
 *
 * THE OP
 *     I[m, n, g] = sum_{k in group g} (lx[m, k] - zx) * (code[n, k] - qzero[n, g])          an exact integer
 *     y[m, n]    = s_x * sum_g qscale[n, g] * float(I[m, n, g])  (+ bias[n])
 * lx[m, k] is the integer level of an activation, zx its integer zero point, s_x = max(|scale|, eps) its sanitised
 * per-tensor scale (make_qparams / sanitize_scale_per_tensor of the per-tensor forward).  The weight is in THE FORMAT of
 * include/lsq_hip_pack.h: `bits` is 4 or 2, K % G == 0, G % (8 / bits) == 0, codes row-major and little-endian inside the
 * byte (N * K * bits / 8 bytes, any byte offset), qscale float32 and qzero int32 (within +-2^23) of [N, K / G].
 * y is [M, N] in LSQ_BF16, LSQ_F16 or LSQ_F32; bias is NULL or N values of LSQ_F32 or of y's type.
 * 1 <= M <= LSQ_QLINEAR_A8_MAX_ROWS; larger M is the caller's business.
 *
 * THE ARITHMETIC
 *  - I is exact for every input the two formats allow: levels and zx anywhere in -128..255, codes in 0..2^bits - 1, qzero
 *    within +-2^23, any legal G (64-bit integers where 32 do not suffice).
 *  - I is converted to fp32 with ONE rounding and multiplied by qscale in fp32; the sum over g runs in fp32.  Then one
 *    multiply by s_x, then the bias in fp32, then the one rounding to the type of y.
 *  - No atomics.  The order of the sum over the groups depends on (K, G, bits, the form) alone -- never on M, on the data,
 *    or on whether the levels came from memory or were formed in the kernel.  Repeated launches are bit-identical, and row
 *    m of an M-row call is bit for bit the 1-row call on row m.
 *  - Exact when the arithmetic is: if every qscale[n, g] * I and every partial sum is representable in fp32, y is the exact
 *    result rounded once.
 *
 * TWO ENTRY FORMS OVER ONE KERNEL
 *  - lsq_qlinear_a8_forward_levels: the levels as bytes (LSQ_A8_U8: 0..255, LSQ_A8_I8: -128..127), s_x and zx as one
 *    float32 / int32 value each ON THE DEVICE (read in the kernel; nothing is read back).
 *  - lsq_qlinear_a8_forward (fused): floating x; while staging x the kernel forms each element's level with lsq_math.hpp's
 *    make_qparams / level(), the forward's own code, from the quantizer's scale and shift (one float32 value each on the
 *    device) and its four range integers.  y has x's type.  The result is bit for bit the levels form on the bytes the
 *    per-tensor levels forward writes for the same x and constants; a NaN in x goes to quant_min as in the forward.
 */
#ifndef LSQ_HIP_QLINEAR_A8_H_
#define LSQ_HIP_QLINEAR_A8_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_QLINEAR_A8_ABI_VERSION 1
#define LSQ_QLINEAR_A8_MAX_ROWS 16
/* level_dtype of lsq_qlinear_a8_forward_levels */
#define LSQ_A8_U8 0
#define LSQ_A8_I8 1

/* LSQ_QLINEAR_A8_ABI_VERSION the library was built with. */
int lsq_qlinear_a8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_qlinear_a8_last_error(void);

/* Levels in.  `x_levels` is [M, K] bytes of `level_dtype`; `s_x` points to one float32 and `zx` to one int32 on the device
 * (zx within -128..255).  `bias` may be NULL (bias_dtype is then ignored); otherwise bias_dtype is LSQ_F32 or `y_dtype`.
 * y, qscale, qzero, s_x, zx and bias must be element-aligned.  A `codes` pointer that is not 16-byte aligned takes the
 * generic form (see lsq_qlinear_a8_plan). */
int lsq_qlinear_a8_forward_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx,
                                  const void* codes, int64_t N, int64_t K, int64_t group_size, int bits, const void* qscale,
                                  const void* qzero, const void* bias, int bias_dtype, void* y, int y_dtype, void* stream);

/* Floating x in (fused).  x and y are [M, K] / [M, N] of `dtype` (LSQ_BF16, LSQ_F16 or LSQ_F32), element-aligned; `scale`
 * and `shift` point to one float32 each on the device.  [quant_min, quant_max] and [type_min, type_max] must lie within
 * 0..255 or within -128..127. */
int lsq_qlinear_a8_forward(int dtype, const void* x, int64_t M, const void* scale, const void* shift, int64_t quant_min,
                           int64_t quant_max, int64_t type_min, int64_t type_max, const void* codes, int64_t N, int64_t K,
                           int64_t group_size, int bits, const void* qscale, const void* qzero, const void* bias,
                           int bias_dtype, void* y, void* stream);

/* Host only, nothing is launched: the launch of either entry form for (M, N, K, group_size, bits) on the current device
 * (256 compute units are assumed when there is none) with a 16-byte aligned `codes`; the types of x and y do not enter.
 * out8 = [form, grid, workgroup size, rows served natively (LSQ_QLINEAR_A8_MAX_ROWS), bytes of LDS, elements of K per LDS
 * chunk of x (0 in the generic form), waves that share one output tile, output columns per tile].
 * form 1 = matrix cores: G a multiple of the 128 / bits elements of one 16-byte code packet and lcm(G, 4 packets) <= 4096
 *          elements; a 16 x 16 output tile per workgroup, K split over its 16 waves in runs of whole groups, 16-byte code
 *          loads, x staged in LDS as the int8 operand, mfma_i32_16x16x64_i8 on the codes as unsigned nibbles, the two zero
 *          points as integer corrections per group, one fp32 multiply by qscale per group.
 * form 0 = generic: one wave per output column, 64-bit integer multiply-adds, a butterfly sum over the lanes of a group
 *          (small or odd G, very large G, misaligned codes). */
int lsq_qlinear_a8_plan(int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
