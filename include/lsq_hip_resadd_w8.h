/* include/lsq_hip_resadd_w8.h -- the W8A8 linear and conv2d on gfx950 that CLOSE A RESIDUAL BLOCK: the integer sum and the fp32
 * steps of lsq_hip_requant_w8.h, then a residual given as 8-bit LEVELS added in the epilogue, (ReLU and) the add's per-tensor
 * quantizer.  `out = relu(q_add(conv_last(h) + identity))` in one launch, one byte read and one byte written per activation.
 *
 * Exported by `liblsq_hip_resadd_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/resadd_w8/ for gfx950), the eleventh
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes
 * of lsq_hip.h, the geometry struct of lsq_hip_qconv_w8.h and the output quantizer struct and level codes of
 * lsq_hip_requant_w8.h, and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device
 * buffers, kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation,
 * no environment variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is validated before
 * anything is enqueued; lsq_resadd_w8_last_error() describes the calling thread's last failure.
 *
 * THE OP.  With the exact integer I, s_x, zx, s_w[n], zw[n] and bias[n] of lsq_hip_qlinear_w8.h (linear) or
 * lsq_hip_qconv_w8.h (conv2d), `mid` = out->mid_dtype, l_r the residual's level at the same (m, n), s_r = res->scale[0] and
 * z_r = res->zero_point[0]:
 *     v = ((s_w[n] * float(I)) * s_x) + bias[n]                  fp32, each step rounded once, no fused multiply-add
 *     u = float(round_to(mid, v))                                mid: LSQ_F32 (identity), LSQ_BF16 or LSQ_F16
 *     p = pre ? float(round_to(mid, dequant(level(u; pre), pre))) : u
 *                                                                OPTIONAL: the layer's own output fake-quantizer, lsq_math.hpp's
 *                                                                level() and dequant() with make_qparams(
 *                                                                sanitize_scale_per_tensor(pre->scale[0]), pre->shift[0], range)
 *     d = float(round_to(mid, (float(l_r) - float(z_r)) * s_r))  s_r and z_r as they are, not sanitised
 *     t = float(round_to(mid, p + d))                            one fp32 add, one rounding; d and the add are NOT one fma
 *     r = relu ? (t < 0 ? 0 : t) : t                             a select: a NaN stays a NaN
 *     q = level(r; out),  y = q mod 256                          as lsq_hip_requant_w8.h; a NaN goes to quant_min
 * That is, bit for bit, the composition of existing ops: the float-output op writing a `mid` y; with `pre` the per-tensor
 * fake-quantize forward on that y; plus the residual dequantized to `mid`; the select; the per-tensor levels forward.
 * y is [M, N] bytes (conv2d: [B, OH, OW, Cout], channels-last), dense, at any byte offset, and so is the residual.
 * No atomics; launches repeat bit for bit; an output's bits depend on its row (receptive field), its residual byte, the weight
 * and the constants alone; the GPU result equals the package's CPU path bit for bit.
 *
 * TWO ENTRY FORMS, both with the activation levels as bytes: a block's last layer always reads levels.  Without `pre` and
 * without a residual the op is lsq_hip_requant_w8.h's and is not offered here.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): everything lsq_hip_requant_w8.h refuses; a NULL `res` or res->levels;
 * a NULL or misaligned res->scale / res->zero_point; a res->level_dtype that is not LSQ_REQUANT_W8_U8 / _I8; a `pre` with a NULL
 * or misaligned scale or shift, or whose range is empty or lies neither within 0..255 nor within -128..127; a residual whose
 * M * N bytes overlap y's (an in-place add is not served); a NULL out10.
 */
#ifndef LSQ_HIP_RESADD_W8_H_
#define LSQ_HIP_RESADD_W8_H_

#include "lsq_hip.h"
#include "lsq_hip_qconv_w8.h"
#include "lsq_hip_requant_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_RESADD_W8_ABI_VERSION 1
/* out10[9] of the plans */
#define LSQ_RESADD_W8_LOAD_BYTES 0
#define LSQ_RESADD_W8_LOAD_PACKETS 1

/* The residual of one call: `levels` is [M, N] bytes (conv2d: [B, OH, OW, Cout]) of `level_dtype` (LSQ_REQUANT_W8_U8 / _I8),
 * dense, at any byte offset; `scale` is one float32 and `zero_point` one int32 ON THE DEVICE, read in the kernel as they are. */
typedef struct lsq_resadd_w8_res {
    const void* levels;
    int64_t level_dtype;
    const void* scale;
    const void* zero_point;
} lsq_resadd_w8_res;

/* The layer's own output fake-quantizer: `scale` and `shift` are one float32 each ON THE DEVICE. */
typedef struct lsq_resadd_w8_pre {
    const void* scale;
    const void* shift;
    int64_t quant_min, quant_max, type_min, type_max;
} lsq_resadd_w8_pre;

/* LSQ_RESADD_W8_ABI_VERSION the library was built with. */
int lsq_resadd_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_resadd_w8_last_error(void);

/* Linear, levels in: lsq_requant_w8_linear_levels' arguments, the residual `res` and the optional `pre` (NULL: none). */
int lsq_resadd_w8_linear_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx,
                                int w_level_dtype, const void* w_levels, int64_t N, int64_t K, const void* w_scale,
                                const void* w_zero, const void* bias, int bias_dtype, const lsq_requant_w8_out* out,
                                const lsq_resadd_w8_res* res, const lsq_resadd_w8_pre* pre, void* y, void* stream);

/* Conv2d, levels in: lsq_requant_w8_conv_levels' arguments, `res` ([B, OH, OW, Cout] bytes) and the optional `pre`. */
int lsq_resadd_w8_conv_levels(int level_dtype, const void* x_levels, const void* s_x, const void* zx,
                              const lsq_qconv_w8_geom* geom, int w_level_dtype, const void* w_levels, const void* w_scale,
                              const void* w_zero, const void* bias, int bias_dtype, const lsq_requant_w8_out* out,
                              const lsq_resadd_w8_res* res, const lsq_resadd_w8_pre* pre, void* y, void* stream);

/* Host only, nothing is launched: lsq_requant_w8_plan_linear's nine fields, with the same thresholds, and a tenth:
 * out10[9] = how the residual tile is read (LSQ_RESADD_W8_LOAD_*): form 1 loads it as 16-byte packets along n during the last
 * K step and keeps it in the LDS region of the output byte tile (LOAD_PACKETS: N % 16 == 0 and `res_aligned`, the residual
 * 16-byte aligned), else fills that region byte by byte after the loop (LOAD_BYTES); form 0 loads one byte per output.
 * The choice is independent of y's store. */
int lsq_resadd_w8_plan_linear(int64_t M, int64_t N, int64_t K, int aligned, int y_aligned, int res_aligned, int32_t* out10);

/* The same for a convolution. */
int lsq_resadd_w8_plan_conv(const lsq_qconv_w8_geom* geom, int aligned, int y_aligned, int res_aligned, int32_t* out10);

#ifdef __cplusplus
}
#endif
#endif
