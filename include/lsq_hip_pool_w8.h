/* include/lsq_hip_pool_w8.h -- 2-D max and average pooling on 8-bit LEVELS on gfx950: what keeps a converted network in
 * levels between its W8A8 layers (the max pool after the stem, the global average pool before the classifier).
 *
 * Exported by `liblsq_hip_pool_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/pool_w8/ for gfx950), the twelfth companion
 * of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of lsq_hip.h,
 * and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device buffers, kernels enqueued
 * on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation, no environment
 * variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is validated before anything is
 * enqueued; lsq_pool_w8_last_error() describes the calling thread's last failure.
 *
 * OPERANDS.  x is [B, H, W, C] bytes (channels-last) of `level_dtype` (LSQ_POOL_W8_U8: 0..255, LSQ_POOL_W8_I8: -128..127),
 * y is [B, OH, OW, C]; both dense, at any byte offset (a floating y: element-aligned).  OH and OW follow
 * torch.nn.functional: out = floor_or_ceil((in + 2 p - d (k - 1) - 1) / s) + 1, and with ceil_mode one less when the last
 * window would start beyond the input and its left padding ((out - 1) s >= in + p).
 *
 * MAX POOL: levels in, levels of the SAME quantizer out; no constants are read.
 *     y[b, oh, ow, c] = max over the window's taps (oh sh - ph + i dh, ow sw - pw + j dw) that lie inside the input of x[b, ih, iw, c]
 * an unsigned or a signed byte max according to level_dtype.  A tap in the padding does not take part (torch's -inf, not a
 * level).  That is F.max_pool2d on the levels as integers and, dequantize being non-decreasing for a positive scale, also
 * F.max_pool2d of the dequantized values re-expressed as levels.
 *
 * AVERAGE POOL (no dilation): levels in; the levels of an output quantizer out, or floats.  With s_x = avg->s_x[0] and
 * z_x = avg->zx[0] as they are, `mid` = avg->mid_dtype:
 *     S = sum over the window's taps inside the input of (l - z_x)      exact integer (a padded tap holds z_x: it adds 0)
 *     a = float(S) * s_x                                                fp32, rounded once
 *     v = a / float(D)                                                  fp32 IEEE division, rounded once; no reciprocal, no fma
 *     u = float(round_to(mid, v))                                       mid: LSQ_F32 (identity), LSQ_BF16 or LSQ_F16
 *     with out_scale:  q = level(u; out),  y = q mod 256                lsq_math.hpp's level() with make_qparams(
 *                                                                       sanitize_scale_per_tensor(out_scale[0]), out_shift[0],
 *                                                                       range); a NaN goes to quant_min
 *     without:         y = round_to(mid, v), stored as mid
 * D is ATen's divisor: divisor_override if has_divisor; else with count_include_pad the window clipped to the PADDED extent,
 * (min(h0 + kh, H + ph) - h0) (min(w0 + kw, W + pw) - w0); else the number of taps inside the input.  Global and adaptive
 * pooling is kh = sh = H / OH, kw = sw = W / OW (lsq_pool_w8_adaptive fills that in where both divide evenly).
 * No atomics; launches repeat bit for bit; an output depends on its window and the constants alone; the GPU result equals the
 * package's CPU path (an exact integer window sum, then the same fp32 steps) bit for bit.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): a NULL geometry, x or y; NULL or misaligned s_x, zx, out_scale,
 * out_shift (out_scale and out_shift come together); a level_dtype that is not LSQ_POOL_W8_U8 / _I8; a mid_dtype that is not
 * LSQ_F32 / LSQ_BF16 / LSQ_F16; a floating y that is not element-aligned; B, C, H or W < 1; an empty output; k, s or d < 1;
 * negative padding or padding > k / 2; an extent beyond 29 bits; a window of more than 2^23 taps (the 32-bit sum stays exact);
 * a dilated window that may miss the input altogether (p > 0 and d > the extent); dilation in the average pool;
 * has_divisor with divisor_override < 1; an output range that is empty or lies neither within 0..255 nor within -128..127;
 * an adaptive size that does not divide H or W; y overlapping x; a NULL out8.
 */
#ifndef LSQ_HIP_POOL_W8_H_
#define LSQ_HIP_POOL_W8_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_POOL_W8_ABI_VERSION 1
#define LSQ_POOL_W8_U8 0
#define LSQ_POOL_W8_I8 1
/* out8[0] of the plans */
#define LSQ_POOL_W8_GENERIC 0
#define LSQ_POOL_W8_PACKETS 1            /* max pool, and the average pool with one window per lane */
#define LSQ_POOL_W8_PACKETS_SHARED 2     /* average pool: several lanes of a workgroup share a window */

/* The geometry of one call. */
typedef struct lsq_pool_w8_geom {
    int64_t B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, ceil_mode;
} lsq_pool_w8_geom;

/* The average pool's constants: `s_x` is one float32 and `zx` one int32 ON THE DEVICE, read in the kernel as they are;
 * `out_scale` and `out_shift` one float32 each on the device, or both NULL for a floating y of mid_dtype. */
typedef struct lsq_pool_w8_avg {
    const void* s_x;
    const void* zx;
    const void* out_scale;
    const void* out_shift;
    int64_t quant_min, quant_max, type_min, type_max, mid_dtype, count_include_pad, has_divisor, divisor_override;
} lsq_pool_w8_avg;

/* LSQ_POOL_W8_ABI_VERSION the library was built with. */
int lsq_pool_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_pool_w8_last_error(void);

/* Max pool: y [B, OH, OW, C] bytes of level_dtype. */
int lsq_pool_w8_max(int level_dtype, const void* x_levels, const lsq_pool_w8_geom* geom, void* y, void* stream);

/* Average pool: y [B, OH, OW, C] bytes (uint8 for an output range in 0..255, int8 for one in -128..127) or mid_dtype floats. */
int lsq_pool_w8_avg_forward(int level_dtype, const void* x_levels, const lsq_pool_w8_geom* geom, const lsq_pool_w8_avg* avg, void* y,
                            void* stream);

/* Host only: kh = sh = H / out_h, kw = sw = W / out_w, no padding, no dilation, no ceil_mode into `geom` (whose B, C, H, W are
 * set); refused where out_h does not divide H or out_w does not divide W. */
int lsq_pool_w8_adaptive(int64_t out_h, int64_t out_w, lsq_pool_w8_geom* geom);

/* Host only, nothing is launched.  `aligned`: x and y are 16-byte aligned.
 * out8[0] = the kernel family (LSQ_POOL_W8_*): PACKETS needs C % 16 == 0 and `aligned`, every other legal call is GENERIC (one
 * lane per output element); out8[1] = workgroups, out8[2] = threads per workgroup, out8[3] = adjacent output pixels per lane
 * (max pool) or lanes that share a window (average pool), out8[4] = OH, out8[5] = OW, out8[6] = LDS bytes,
 * out8[7] = 16-channel packets per workgroup (PACKETS_SHARED); K where the kernel has the K x K window without dilation unrolled,
 * all its loads issued at once (PACKETS: K = 2 or 3, else 0); 0 (GENERIC). */
int lsq_pool_w8_plan_max(const lsq_pool_w8_geom* geom, int aligned, int32_t* out8);

/* The same for the average pool.  A lane owns a window's 16-channel packet (PACKETS) while the window has fewer than 10 taps
 * or the grid fills the chip anyway; else L lanes of a workgroup share it (PACKETS_SHARED), L the smallest power of two with
 * which the grid has two workgroups per compute unit, at most the largest power of two within the taps and 256. */
int lsq_pool_w8_plan_avg(const lsq_pool_w8_geom* geom, int aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
