/* include/lsq_hip_qconv_w8.h -- W8A8 conv2d on gfx950: 8-bit activation LEVELS times 8-bit weight LEVELS with one (scale, zero
 * point) per output channel, summed in integers over all taps and input channels; channels-last operands.
 *
 * Exported by `liblsq_hip_qconv_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/qconv_w8/ for gfx950), the ninth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header only borrows the dtype codes and
 * the status codes of lsq_hip.h, and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned
 * device buffers, kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no
 * synchronisation, no environment variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is
 * validated before anything is enqueued; lsq_qconv_w8_last_error() describes the calling thread's last failure.
 *
 * THE OP (include/lsq_hip_qlinear_w8.h's, with k running over tap row i, tap column j and input channel c)
 *     I[b, n, oh, ow] = sum_{i, j, c} (lx[b, c, oh sh - ph + i dh, ow sw - pw + j dw] - zx) * (lw[n, c, i, j] - zw[n])
 *                       an exact integer; a tap outside x contributes 0
 *     y[b, n, oh, ow] = round_to_y( ((s_w[n] * float(I)) * s_x) + bias[n] )
 * groups == 1, zero padding, any stride, padding and dilation per axis, OH = (H + 2 ph - dh (kh - 1) - 1) / sh + 1 (OW alike).
 * lx, zx, s_x, lw, s_w, zw, bias and y are what they are in lsq_hip_qlinear_w8.h (the level type codes LSQ_QCONV_W8_U8 / _I8
 * have the values of LSQ_W8_U8 / _I8).
 *
 * MEMORY.  Channels-last throughout: the activation levels (or the floating x of the fused form) are [B, H, W, Cin], the weight
 * levels [Cout, kh, kw, Cin] -- a row-major [N, K] byte matrix with N = Cout, K = kh kw Cin -- and y is [B, OH, OW, Cout],
 * the row-major [M, N] output of that GEMM with M = B OH OW.  All dense.
 *
 * PADDING.  "Contributes 0" means that a padded tap holds the LEVEL zx (the real value 0), not the byte 0.  The matrix-core
 * kernels stage the byte operand zx - off for such a tap (off = 128 for a 0..255 range, else 0), so that sum a w, sum_k a and
 * the zero-point corrections of lsq_hip_qlinear_w8.h need no special case.  PRECONDITION: zx lies within the level type's
 * range (0..255 for LSQ_QCONV_W8_U8, -128..127 for LSQ_QCONV_W8_I8; the fused form: the zero point of make_qparams lies within
 * [type_min, type_max], which the entry point checks to lie in one such range).  A quantized tensor guarantees it; zx lives on
 * the device and cannot be validated.  With a zx outside it the padded taps of the matrix-core form are wrong.
 *
 * THE ARITHMETIC is the linear's: I formed in 64 bits, float(I) rounded once, a rounded multiply by s_w[n], a rounded multiply
 * by s_x, a rounded add of the bias in fp32, one rounding to y's type; no fused multiply-add; no atomics; launches repeat bit
 * for bit; an output's bits depend on its receptive field, the weight and the constants alone, not on B, on the tile shape or
 * on how K is split.  The GPU result equals the package's CPU path (one int64 convolution of lx - zx with lw - zw, zero
 * padded, then the same fp32 steps) bit for bit.
 *
 * TWO ENTRY FORMS
 *  - lsq_qconv_w8_forward_levels: the activation levels as bytes.
 *  - lsq_qconv_w8_forward (fused): floating channels-last x (LSQ_BF16, LSQ_F16 or LSQ_F32) and the activation quantizer's scale
 *    and shift (one float32 each on the device) plus its four range integers; a pre-pass -- one flat pass, the linear's --
 *    writes level(x) - off of every element into the caller-owned `levels_ws` (B H W Cin bytes, 16-byte aligned).  y has
 *    x's type.  The result is bit for bit the levels form on the bytes the per-tensor levels forward writes.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): everything lsq_hip_qlinear_w8.h refuses (an unknown or float64 dtype
 * code; a level type code that is neither U8 nor I8; a NULL x, s_x / zx (scale / shift), w_levels, w_scale, w_zero or y; a
 * bias dtype that is neither float32 nor y's; element misalignment of y, x, s_x, zx, scale, shift, w_scale, w_zero or bias;
 * ranges outside 0..255 and outside -128..127 or empty; a NULL or misaligned levels_ws; a NULL out8); a NULL geometry; B, Cin,
 * H or W < 1; a negative Cout; a non-positive kernel, stride or dilation; negative padding; an empty output (OH or OW < 1); a
 * padded extent (H + 2 ph, W + 2 pw), stride or dilation beyond 31 bits; shapes beyond 64-bit offsets or a 31-bit grid.
 */
#ifndef LSQ_HIP_QCONV_W8_H_
#define LSQ_HIP_QCONV_W8_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_QCONV_W8_ABI_VERSION 1
/* level_dtype and w_level_dtype */
#define LSQ_QCONV_W8_U8 0
#define LSQ_QCONV_W8_I8 1
/* out8[1] of lsq_qconv_w8_plan */
#define LSQ_QCONV_W8_SHAPE_GENERIC 0
#define LSQ_QCONV_W8_SHAPE_TILES 1
#define LSQ_QCONV_W8_SHAPE_TILES_SPLIT_K 2

/* The geometry of one call: x is [B, H, W, Cin], the weight [Cout, kh, kw, Cin]; stride (sh, sw), zero padding (ph, pw) on
 * both sides of an axis, dilation (dh, dw). */
typedef struct lsq_qconv_w8_geom {
    int64_t B, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw;
} lsq_qconv_w8_geom;

/* LSQ_QCONV_W8_ABI_VERSION the library was built with. */
int lsq_qconv_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_qconv_w8_last_error(void);

/* Levels in.  `x_levels` is [B, H, W, Cin] bytes of `level_dtype`, any byte offset. */
int lsq_qconv_w8_forward_levels(int level_dtype, const void* x_levels, const void* s_x, const void* zx,
                                const lsq_qconv_w8_geom* geom, int w_level_dtype, const void* w_levels, const void* w_scale,
                                const void* w_zero, const void* bias, int bias_dtype, void* y, int y_dtype, void* stream);

/* Floating x in (fused).  x is [B, H, W, Cin] and y [B, OH, OW, Cout] of `dtype`.  [quant_min, quant_max] and [type_min,
 * type_max] must lie within 0..255 or within -128..127.  `levels_ws`: B H W Cin bytes on the device, 16-byte aligned. */
int lsq_qconv_w8_forward(int dtype, const void* x, const void* scale, const void* shift, int64_t quant_min, int64_t quant_max,
                         int64_t type_min, int64_t type_max, const lsq_qconv_w8_geom* geom, int w_level_dtype,
                         const void* w_levels, const void* w_scale, const void* w_zero, const void* bias, int bias_dtype,
                         void* y, void* levels_ws, void* stream);

/* Host only, nothing is launched: the launch of either entry form for `geom` on the current device (256 compute units are
 * assumed when there is none); `aligned`: whether w_levels AND the activation levels are 16-byte aligned (the fused form's
 * workspace always is).
 * out8 = [form, launch shape (LSQ_QCONV_W8_SHAPE_*), grid, workgroup size, output pixels (rows of the implicit matrix) per
 * workgroup, output channels per workgroup, bytes of LDS, waves of a workgroup that split K].
 * form 1 = matrix cores (Cin % 16 == 0, K = kh kw Cin <= 65536, both 16-byte aligned): the TILES kernel of
 *          lsq_hip_qlinear_w8.h on the implicit [B OH OW, K] matrix -- every 16-byte packet of a row lies inside one tap and
 *          is one aligned load of x or one padding packet.  32 / 64 / 128 rows (M <= 32 / <= 64 / more; M <= 16 takes 32) by
 *          64 columns of four waves; TILES_SPLIT_K, while the 64-column tiles would not give every compute unit one: the same
 *          rows by 16 columns, K split over the four waves.
 * form 0 = generic (every other legal call: Cin % 16 != 0, K > 65536, a misaligned buffer): one wave per output channel
 *          and four output pixels, 64-bit integer multiply-adds over the in-bounds taps, a butterfly.  Correct, not tuned. */
int lsq_qconv_w8_plan(const lsq_qconv_w8_geom* geom, int aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
