/* include/lsq_hip_requant_w8.h -- W8A8 linear and conv2d on gfx950 with an 8-bit OUTPUT: the integer sum of
 * lsq_hip_qlinear_w8.h / lsq_hip_qconv_w8.h, their fp32 steps, then (ReLU and) the NEXT layer's per-tensor quantizer in the
 * epilogue.  Levels in, the next quantizer's levels out: one launch per layer, one byte written per activation.
 *
 * Exported by `liblsq_hip_requant_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/requant_w8/ for gfx950), the tenth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes
 * of lsq_hip.h and the geometry struct of lsq_hip_qconv_w8.h, and the library imports no symbol of the others.  Same contract
 * as lsq_hip.h: caller-owned device buffers, kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default stream),
 * no allocation, no synchronisation, no environment variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws,
 * everything is validated before anything is enqueued; lsq_requant_w8_last_error() describes the calling thread's last failure.
 *
 * THE OP.  With the exact integer I, s_x, zx, s_w[n], zw[n] and bias[n] of lsq_hip_qlinear_w8.h (linear) or
 * lsq_hip_qconv_w8.h (conv2d; channels-last operands, a padded tap holds the level zx):
 *     v = ((s_w[n] * float(I)) * s_x) + bias[n]      each step rounded once, fp32, no fused multiply-add
 *     u = float(round_to(mid_dtype, v))              mid_dtype: LSQ_F32 (identity), LSQ_BF16 or LSQ_F16
 *     r = relu ? (u < 0 ? 0 : u) : u                 a select: a NaN stays a NaN
 *     q = rne(med3(r * inv_s_o + zp_o, quant_min, quant_max))       lsq_math.hpp's level() with
 *                                                    make_qparams(sanitize_scale_per_tensor(out_scale[0]), out_shift[0], range);
 *                                                    a NaN goes to quant_min
 *     y = q mod 256                                  one byte per output: uint8 levels when the ranges lie in 0..255, int8
 *                                                    levels when they lie in -128..127
 * That is, bit for bit, the existing op writing a `mid_dtype` y, the select, and the per-tensor levels forward on the result:
 * `mid_dtype` is the dtype in which the unfused model hands y from one layer to the next quantizer.  y is [M, N] bytes
 * (conv2d: [B, OH, OW, Cout], channels-last), dense, at any byte offset: the A operand of the next layer as it lies.
 * No atomics; launches repeat bit for bit; an output's bits depend on its row (receptive field), the weight and the constants
 * alone; the GPU result equals the package's CPU path bit for bit.
 *
 * FOUR ENTRY FORMS: linear / conv2d, each with the activation levels as bytes (`_levels`) or a floating x and the INPUT
 * quantizer's constants (fused: the flat pre-pass of the other two libraries writes level(x) - off into `levels_ws`; `mid_dtype`
 * must be x's dtype, as y of the unfused op has x's dtype).
 *
 * NOT HERE: the 16-wave decode kernel of lsq_hip_qlinear_w8.h.  A chain of levels is a prefill and convolution concern; a
 * linear call with M <= 16 takes the 32-row tile, as the convolution does.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): everything lsq_hip_qlinear_w8.h / lsq_hip_qconv_w8.h refuse (with
 * `mid_dtype` in the place of y's dtype); a NULL `out`, out_scale or out_shift, or a misaligned one; an output range outside
 * 0..255 and outside -128..127, or empty; a mid_dtype that is not LSQ_F32, LSQ_BF16 or LSQ_F16; in the fused forms a mid_dtype
 * that is not x's dtype; a NULL out9.
 */
#ifndef LSQ_HIP_REQUANT_W8_H_
#define LSQ_HIP_REQUANT_W8_H_

#include "lsq_hip.h"
#include "lsq_hip_qconv_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_REQUANT_W8_ABI_VERSION 1
/* level_dtype and w_level_dtype */
#define LSQ_REQUANT_W8_U8 0
#define LSQ_REQUANT_W8_I8 1
/* out9[1] of the plans */
#define LSQ_REQUANT_W8_SHAPE_GENERIC 0
#define LSQ_REQUANT_W8_SHAPE_TILES 1
#define LSQ_REQUANT_W8_SHAPE_TILES_SPLIT_K 2
/* out9[8] of the plans */
#define LSQ_REQUANT_W8_STORE_BYTES 0
#define LSQ_REQUANT_W8_STORE_PACKETS 1

/* The output quantizer of one call: `out_scale` and `out_shift` are one float32 each ON THE DEVICE, read in the kernel. */
typedef struct lsq_requant_w8_out {
    const void* out_scale;
    const void* out_shift;
    int64_t quant_min, quant_max, type_min, type_max;
    int64_t relu;       /* 0 or not 0 */
    int64_t mid_dtype;  /* LSQ_F32, LSQ_BF16 or LSQ_F16 */
} lsq_requant_w8_out;

/* LSQ_REQUANT_W8_ABI_VERSION the library was built with. */
int lsq_requant_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_requant_w8_last_error(void);

/* Linear, levels in.  `x_levels` is [M, K] bytes of `level_dtype`, any byte offset; y is [M, N] bytes, any byte offset. */
int lsq_requant_w8_linear_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx,
                                 int w_level_dtype, const void* w_levels, int64_t N, int64_t K, const void* w_scale,
                                 const void* w_zero, const void* bias, int bias_dtype, const lsq_requant_w8_out* out, void* y,
                                 void* stream);

/* Linear, floating x in (fused).  x is [M, K] of `dtype` == out->mid_dtype.  `levels_ws`: M * K bytes, 16-byte aligned. */
int lsq_requant_w8_linear(int dtype, const void* x, int64_t M, const void* scale, const void* shift, int64_t quant_min,
                          int64_t quant_max, int64_t type_min, int64_t type_max, int w_level_dtype, const void* w_levels,
                          int64_t N, int64_t K, const void* w_scale, const void* w_zero, const void* bias, int bias_dtype,
                          const lsq_requant_w8_out* out, void* y, void* levels_ws, void* stream);

/* Conv2d, levels in.  `x_levels` is [B, H, W, Cin] bytes of `level_dtype`, any byte offset; y is [B, OH, OW, Cout] bytes. */
int lsq_requant_w8_conv_levels(int level_dtype, const void* x_levels, const void* s_x, const void* zx,
                               const lsq_qconv_w8_geom* geom, int w_level_dtype, const void* w_levels, const void* w_scale,
                               const void* w_zero, const void* bias, int bias_dtype, const lsq_requant_w8_out* out, void* y,
                               void* stream);

/* Conv2d, floating x in (fused).  x is [B, H, W, Cin] of `dtype` == out->mid_dtype.  `levels_ws`: B H W Cin bytes, 16-byte
 * aligned. */
int lsq_requant_w8_conv(int dtype, const void* x, const void* scale, const void* shift, int64_t quant_min, int64_t quant_max,
                        int64_t type_min, int64_t type_max, const lsq_qconv_w8_geom* geom, int w_level_dtype,
                        const void* w_levels, const void* w_scale, const void* w_zero, const void* bias, int bias_dtype,
                        const lsq_requant_w8_out* out, void* y, void* levels_ws, void* stream);

/* Host only, nothing is launched: the launch of either linear form for (M, N, K) on the current device (256 compute units
 * are assumed when there is none).  `aligned`: whether w_levels AND the activation levels are 16-byte aligned (the fused
 * form's workspace always is); `y_aligned`: whether y is.
 * out9 = [form, launch shape (LSQ_REQUANT_W8_SHAPE_*), grid, workgroup size, rows per workgroup, output columns per
 * workgroup, bytes of LDS, waves of a workgroup that split K, store (LSQ_REQUANT_W8_STORE_*)].
 * form 1 = matrix cores (K % 16 == 0, K <= 65536, `aligned`): the TILES kernels of lsq_hip_qconv_w8.h's plan -- 32 / 64 / 128
 *          rows (M <= 32 / <= 64 / more) by 64 columns, or by 16 columns with K split over the four waves while the wide
 *          tiles would not give every compute unit one.  The bytes of a tile are gathered in LDS and stored as 16-byte
 *          packets along n (STORE_PACKETS: N % 16 == 0 and `y_aligned`), else byte by byte (STORE_BYTES).
 * form 0 = generic (every other legal call): the generic kernels' integer sum, the same epilogue, byte stores. */
int lsq_requant_w8_plan_linear(int64_t M, int64_t N, int64_t K, int aligned, int y_aligned, int32_t* out9);

/* The same for a convolution (lsq_hip_qconv_w8.h's plan: form 1 needs Cin % 16 == 0, K = kh kw Cin <= 65536, `aligned`). */
int lsq_requant_w8_plan_conv(const lsq_qconv_w8_geom* geom, int aligned, int y_aligned, int32_t* out9);

#ifdef __cplusplus
}
#endif
#endif
