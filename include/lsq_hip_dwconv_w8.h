/* include/lsq_hip_dwconv_w8.h -- W8A8 DEPTHWISE conv2d (groups == C, channel multiplier 1) on gfx950: 8-bit activation LEVELS
 * times 8-bit weight LEVELS with one (scale, zero point) per channel, summed in integers over the taps of ONE channel, then the
 * epilogue of lsq_hip_requant_w8.h (with ReLU6 besides ReLU): levels in, the next quantizer's levels -- or floats -- out.
 *
 * Exported by `liblsq_hip_dwconv_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/dwconv_w8/ for gfx950), the thirteenth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h and the geometry struct of lsq_hip_qconv_w8.h (with Cout == Cin == C), and the library imports no symbol of the
 * others.  Same contract as lsq_hip.h: caller-owned device buffers, kernels enqueued on `stream` (a hipStream_t as void*, NULL =
 * the default stream), no allocation, no synchronisation, no environment variables, 0 / negative LSQ_E* / positive hipError_t
 * returns, never throws, everything is validated before anything is enqueued; lsq_dwconv_w8_last_error() describes the calling
 * thread's last failure.
 *
 * OPERANDS.  x_levels is [B, H, W, C] bytes (channels-last) of `level_dtype`, at any byte offset.  w_levels is [kh, kw, C] bytes
 * of `w_level_dtype`, TAP-MAJOR: the 16 channels of a packet of one tap are 16 adjacent bytes.  w_scale is C float32 and w_zero
 * C int32, s_x one float32 and zx one int32, all on the device and read in the kernel.  bias is NULL or C values of float32 or
 * of `mid_dtype`.  y is [B, OH, OW, C]: bytes at any offset (out->out_scale given), or `mid_dtype` elements (out->out_scale
 * NULL), element-aligned.  OH = (H + 2 ph - dh (kh - 1) - 1) / sh + 1, OW alike.
 *
 * THE OP
 *     I[b, c, oh, ow] = sum over the taps (i, j) inside x of (lx[b, oh sh - ph + i dh, ow sw - pw + j dw, c] - zx) * (lw[i, j, c] - zw[c])
 *                       an exact integer: a padded tap holds the level zx and contributes 0
 *     v = ((s_w[c] * float(I)) * s_x) + bias[c]      each step rounded once, fp32, no fused multiply-add
 *     u = float(round_to(mid_dtype, v))              mid_dtype: LSQ_F32 (identity), LSQ_BF16 or LSQ_F16
 *     r = act == 0 ? u : act == 1 ? (u < 0 ? 0 : u) : (u < 0 ? 0 : (u > 6 ? 6 : u))        selects: a NaN stays a NaN
 *     with out_scale:  y = level(r) mod 256          lsq_math.hpp's level() with make_qparams(sanitize_scale_per_tensor(
 *                                                    out_scale[0]), out_shift[0], range); a NaN goes to quant_min; uint8 levels
 *                                                    for ranges in 0..255, int8 levels for ranges in -128..127
 *     without:         y = r, stored as mid_dtype
 * kh kw <= 4096, so |I| <= 4096 * 255^2 < 2^31 and 32-bit sums are exact.  act: LSQ_DWCONV_W8_ACT_NONE / _RELU / _RELU6 (6 is
 * exact in all three mid dtypes).  No atomics; launches repeat bit for bit; an output depends on its receptive field, its
 * channel's weights and the constants alone; the GPU result equals the package's CPU path (one int64 grouped convolution of
 * lx - zx with lw - zw, then the same fp32 steps) bit for bit.
 *
 * PRECONDITION (as lsq_hip_qconv_w8.h's): zx lies within the level type's range.  The packet kernels with a window known at
 * compile time put the byte zx in the place of a tap outside x; zx lives on the device and cannot be validated.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): everything lsq_hip_requant_w8.h refuses for its conv form (a level type
 * code that is neither U8 nor I8; a NULL x, s_x, zx, w_levels, w_scale, w_zero, y or `out`; a bias dtype that is neither float32
 * nor mid_dtype; element misalignment of s_x, zx, w_scale, w_zero, bias, out_scale or out_shift; a mid_dtype that is not LSQ_F32,
 * LSQ_BF16 or LSQ_F16; an output range outside 0..255 and outside -128..127, or empty; a NULL geometry; B, C, H or W < 1; a
 * non-positive kernel, stride or dilation; negative padding; an empty output; a padded extent, stride or dilation beyond 31
 * bits; shapes beyond 64-bit offsets or a 31-bit grid); out_scale without out_shift or the reverse; a floating y that is not
 * element-aligned; Cout != Cin (a channel multiplier); kh kw > 4096; act outside 0..2; y overlapping x; a NULL out8.
 */
#ifndef LSQ_HIP_DWCONV_W8_H_
#define LSQ_HIP_DWCONV_W8_H_

#include "lsq_hip.h"
#include "lsq_hip_qconv_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_DWCONV_W8_ABI_VERSION 1
/* level_dtype and w_level_dtype */
#define LSQ_DWCONV_W8_U8 0
#define LSQ_DWCONV_W8_I8 1
/* out->act */
#define LSQ_DWCONV_W8_ACT_NONE 0
#define LSQ_DWCONV_W8_ACT_RELU 1
#define LSQ_DWCONV_W8_ACT_RELU6 2
/* out8[0] of lsq_dwconv_w8_plan */
#define LSQ_DWCONV_W8_GENERIC 0
#define LSQ_DWCONV_W8_PACKETS 1
#define LSQ_DWCONV_W8_MAX_TAPS 4096

/* The output of one call: `out_scale` and `out_shift` are one float32 each ON THE DEVICE, read in the kernel; both NULL: y is
 * `mid_dtype` floats and the four range integers are not read. */
typedef struct lsq_dwconv_w8_out {
    const void* out_scale;
    const void* out_shift;
    int64_t quant_min, quant_max, type_min, type_max;
    int64_t act;        /* LSQ_DWCONV_W8_ACT_* */
    int64_t mid_dtype;  /* LSQ_F32, LSQ_BF16 or LSQ_F16 */
} lsq_dwconv_w8_out;

/* LSQ_DWCONV_W8_ABI_VERSION the library was built with. */
int lsq_dwconv_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_dwconv_w8_last_error(void);

/* Levels in.  geom->Cout == geom->Cin == C. */
int lsq_dwconv_w8_forward_levels(int level_dtype, const void* x_levels, const void* s_x, const void* zx,
                                 const lsq_qconv_w8_geom* geom, int w_level_dtype, const void* w_levels, const void* w_scale,
                                 const void* w_zero, const void* bias, int bias_dtype, const lsq_dwconv_w8_out* out, void* y,
                                 void* stream);

/* Host only, nothing is launched: the launch for `geom` on the current device (256 compute units are assumed when there is
 * none).  `aligned`: x_levels, w_levels, w_scale AND w_zero are 16-byte aligned (the packet kernels read the two vectors in
 * 16-byte packets as well); `y_aligned`: y is.
 * out8 = [family (LSQ_DWCONV_W8_*), workgroups, threads per workgroup, adjacent output pixels along ow per lane, OH, OW,
 *         K where the packet kernel has the K x K window without dilation unrolled (3) else 0, the stride that kernel was
 *         compiled for (1 or 2) else 0].
 * PACKETS (C % 16 == 0, `aligned` and `y_aligned`): a lane owns one 16-channel packet of P adjacent output pixels; 3 x 3
 *         without dilation at stride (1, 1) and (2, 2) is unrolled, every other window (5 x 5 included) walks its taps in a
 *         loop with P = 1.  P is the library's choice for the stride (1 at both strides as shipped), halved while the grid
 *         would hold fewer than two workgroups per compute unit.
 * GENERIC (every other legal call): one lane per output element, byte loads.  Correct, not tuned. */
int lsq_dwconv_w8_plan(const lsq_qconv_w8_geom* geom, int aligned, int y_aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
