/* include/lsq_hip_qlinear_w8.h -- W8A8 linear on gfx950: 8-bit activation LEVELS times 8-bit weight LEVELS with one (scale,
 * zero point) per output row, summed in integers over all of K.
 *
 * Exported by `liblsq_hip_qlinear_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/qlinear_w8/ for gfx950), the eighth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header only borrows the dtype codes and
 * the status codes of lsq_hip.h, and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned
 * device buffers, kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no
 * synchronisation, no environment variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is
 * validated before anything is enqueued; lsq_qlinear_w8_last_error() describes the calling thread's last failure.
 *
 * THE OP
 *     I[m, n] = sum_k (lx[m, k] - zx) * (lw[n, k] - zw[n])                      an exact integer
 *     y[m, n] = round_to_y( ((s_w[n] * float(I)) * s_x) + bias[n] )
 * lx[m, k] is the integer level of an activation (bytes of LSQ_W8_U8: 0..255 or LSQ_W8_I8: -128..127), zx its integer zero
 * point (within -128..255) and s_x = max(|scale|, eps) its sanitised per-tensor scale, one int32 / float32 value each ON THE
 * DEVICE.  lw is [N, K] weight levels, one byte each, row-major, of `w_level_dtype` (LSQ_W8_U8 or LSQ_W8_I8); s_w[n]
 * (float32) and zw[n] (int32, within the level type's range) are per output row: max(|scale|, eps) and
 * round(clamp(-shift * (1 / s))) of the weight quantizer -- what a per-channel quantized tensor holds.  A per-tensor weight
 * quantizer is served by repeating its one pair N times.  y is [M, N] in LSQ_BF16, LSQ_F16 or LSQ_F32; bias is NULL or N
 * values of LSQ_F32 or of y's type.  Any M >= 1 (64-bit offsets).
 *
 * THE ARITHMETIC
 *  - I is exact for every legal input: |lx - zx| and |lw - zw| reach 255, so |I| passes 2^31 from K of about 33 000; I is
 *    formed in 64 bits.  The kernels multiply the BYTE OPERANDS a = lx - off_x, w = lw - off_w (off = 128 for a 0..255
 *    range, else 0), |a w| <= 2^14, so the raw sum fits 32 bits for K <= 65536, and the zero points enter as integer
 *    corrections: I = sum a w - z_a sum_k w - z_w[n] sum_k a + K z_a z_w[n] with z_a = zx - off_x, z_w = zw - off_w.
 *  - float(I) takes ONE rounding; then a rounded multiply by s_w[n], a rounded multiply by s_x, a rounded add of the bias
 *    (in fp32) and the one rounding to y's type.  No fused multiply-add.
 *  - No atomics.  Launches repeat bit for bit.  A row's bits depend on that row of x, the weight and the constants alone:
 *    not on M, on the row's position, on the tile shape or on how K is split (an integer sum has no order).  The GPU result
 *    equals the package's CPU path (one int64 matrix product, the same fp32 steps) bit for bit.
 *
 * TWO ENTRY FORMS
 *  - lsq_qlinear_w8_forward_levels: the activation levels as bytes.
 *  - lsq_qlinear_w8_forward (fused): floating x (LSQ_BF16, LSQ_F16 or LSQ_F32) and the activation quantizer's scale and shift
 *    (one float32 each on the device) plus its four range integers; a pre-pass forms each element's level with lsq_math.hpp's
 *    make_qparams / level(), the per-tensor forward's own code, into the caller-owned `levels_ws` (M * K bytes, 16-byte
 *    aligned).  y has x's type.  The result is bit for bit the levels form on the bytes the per-tensor levels forward writes
 *    for the same x and constants; a NaN in x goes to quant_min as in the forward.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): an unknown or float64 dtype code; a level_dtype or w_level_dtype
 * that is neither LSQ_W8_U8 nor LSQ_W8_I8; M < 1; negative N or K; shapes beyond 64-bit offsets or a 31-bit grid; a NULL
 * x, s_x / zx (scale / shift), w_levels, w_scale, w_zero or y; a bias dtype that is neither float32 nor y's; a misaligned
 * y, x, s_x, zx, scale, shift, w_scale, w_zero or bias (element alignment); ranges outside 0..255 and outside -128..127 or
 * empty; a NULL or misaligned levels_ws (fused form); a NULL out8.
 */
#ifndef LSQ_HIP_QLINEAR_W8_H_
#define LSQ_HIP_QLINEAR_W8_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_QLINEAR_W8_ABI_VERSION 1
/* level_dtype and w_level_dtype */
#define LSQ_W8_U8 0
#define LSQ_W8_I8 1
/* out8[1] of lsq_qlinear_w8_plan */
#define LSQ_W8_SHAPE_GENERIC 0
#define LSQ_W8_SHAPE_DECODE 1
#define LSQ_W8_SHAPE_TILES 2
#define LSQ_W8_SHAPE_TILES_SPLIT_K 3

/* LSQ_QLINEAR_W8_ABI_VERSION the library was built with. */
int lsq_qlinear_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_qlinear_w8_last_error(void);

/* Levels in.  `x_levels` is [M, K] bytes of `level_dtype`, any byte offset. */
int lsq_qlinear_w8_forward_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx,
                                  int w_level_dtype, const void* w_levels, int64_t N, int64_t K, const void* w_scale,
                                  const void* w_zero, const void* bias, int bias_dtype, void* y, int y_dtype, void* stream);

/* Floating x in (fused).  x and y are [M, K] / [M, N] of `dtype`.  [quant_min, quant_max] and [type_min, type_max] must lie
 * within 0..255 or within -128..127.  `levels_ws`: M * K bytes on the device, 16-byte aligned. */
int lsq_qlinear_w8_forward(int dtype, const void* x, int64_t M, const void* scale, const void* shift, int64_t quant_min,
                           int64_t quant_max, int64_t type_min, int64_t type_max, int w_level_dtype, const void* w_levels,
                           int64_t N, int64_t K, const void* w_scale, const void* w_zero, const void* bias, int bias_dtype,
                           void* y, void* levels_ws, void* stream);

/* Host only, nothing is launched: the launch of either entry form for (M, N, K) on the current device (256 compute units
 * are assumed when there is none); `w_aligned`: whether w_levels is 16-byte aligned.
 * out8 = [form, launch shape (LSQ_W8_SHAPE_*), grid, workgroup size, rows of x per workgroup, output columns per workgroup,
 * bytes of LDS, waves of a workgroup that split K].
 * form 1 = matrix cores (K % 16 == 0, K <= 65536, w_levels 16-byte aligned): v_mfma_i32_16x16x64_i8 with the weight bytes
 *          as the B operand straight from memory (16-byte non-temporal loads), x staged in LDS as the byte operand.
 *          DECODE (M <= 16): a 16-column tile per workgroup, K split over its 16 waves, their int32 tiles summed through
 *          LDS.  TILES: 32 / 64 / 128 rows by 64 columns, four waves of 16 columns each.  TILES_SPLIT_K, while the 64-column
 *          tiles would not give every compute unit one: the same rows by 16 columns, K split over the four waves.
 * form 0 = generic (every other legal call): one wave per output column, 64-bit integer multiply-adds, a butterfly. */
int lsq_qlinear_w8_plan(int64_t M, int64_t N, int64_t K, int w_aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
