/* include/lsq_hip_norm_w8.h -- LayerNorm and RMSNorm on 8-bit LEVELS on gfx950: exact integer row statistics, one byte read and
 * one written per activation.  What keeps a converted ConvNeXt block (depthwise 7x7 -> LayerNorm over C -> 1x1) and a converted
 * token block (residual add -> LayerNorm -> qkv / fc1) in levels at the norm.
 *
 * Exported by `liblsq_hip_norm_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/norm_w8/ for gfx950), the fifteenth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h, and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device buffers, kernels
 * enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation, no environment
 * variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is validated before anything is
 * enqueued; lsq_norm_w8_last_error() describes the calling thread's last failure.
 *
 * THE DEFINITION.  x is R rows of C bytes, dense, at any byte offset: levels of x_dtype (LSQ_NORM_W8_U8: 0..255, LSQ_NORM_W8_I8:
 * -128..127) of ONE per-tensor quantizer whose s_x (float32) and zx (int32) are one value each on the device, read in the kernel
 * as they are.  Every integer quantity is exact; every fp32 step is ONE correctly rounded operation, never contracted; float() of
 * an integer is one round-to-nearest-even conversion.  With b_i the level as an integer:
 *     LSQ_NORM_W8_LAYER (zero-point free: zx is not read)
 *         S1 = sum b_i        S2 = sum b_i^2        V = C S2 - S1^2            (>= 0, up to 2^48: 64 bits)
 *         n_i = C b_i - S1                                                      (|n_i| < 2^24: 32 bits)
 *         var = float(V) / (float(C) * float(C))                                the variance in level^2 units
 *         e = eps / (s_x * s_x)      r = 1.0f / sqrt(var + e)      rc = r / float(C)
 *         t_i = float(n_i) * rc
 *     LSQ_NORM_W8_RMS
 *         d_i = b_i - zx      Q = sum d_i^2         var = float(Q) / float(C)   e, r as above
 *         t_i = float(d_i) * r                                                  (zx within -32768..32767; beyond that the
 *                                                                                result is not specified)
 *     both
 *         a_i = (t_i * w[c]) + bias[c]        a multiply, then an add; `weight` and / or `bias` may be NULL: that step is left out.
 *                                             w and bias hold C values of param_dtype (LSQ_F32 / LSQ_BF16 / LSQ_F16), widened exactly
 *         u_i = round_to(mid, a_i)            mid = mid_dtype: LSQ_F32 (identity), LSQ_BF16, LSQ_F16
 *         with out_scale:  y_i = level(u_i; out) mod 256     lsq_math.hpp's level() with make_qparams(sanitize_scale_per_tensor(
 *                                                            out_scale[0]), out_shift[0], range); a NaN goes to quant_min
 *         without:         y_i = u_i, stored as mid
 * A constant row has V = 0, hence t = 0 and y = level(bias); with eps = 0 such a row gives 0 * inf = NaN, which goes to quant_min.
 * No atomics; launches repeat bit for bit; a row's outputs depend on that row and the constants alone; the GPU result equals
 * the package's CPU path (int64 torch sums, torch float32 ops one at a time, the existing levels op) bit for bit.
 * THIS IS NOT ATen's layer_norm: against F.layer_norm of the dequantized values taken to levels, outputs differ by at most one
 * level in a small share of positions.  Against LayerNorm in real arithmetic of (b - zx) s_x, with s_x, eps, w
 * and bias taken as the float32 numbers given: |a - a_exact| <= 2^-20 (|t w| + |bias|).
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): a NULL geometry, constants, x or y; NULL or misaligned s_x, zx,
 * out_scale, out_shift (out_scale and out_shift come together); a weight or bias that is not element-aligned; a kind that is not
 * LSQ_NORM_W8_LAYER / _RMS; a level dtype that is not LSQ_NORM_W8_U8 / _I8; a param_dtype or mid_dtype that is not LSQ_F32 /
 * LSQ_BF16 / LSQ_F16; R or C < 1; C > 65536 (what keeps sum b^2 and n_i in 32 bits); R beyond 29 bits; eps negative or NaN; a
 * floating y that is not element-aligned; an output range that is empty or lies neither within 0..255 nor within -128..127; y
 * overlapping x, weight or bias; a NULL out8.
 */
#ifndef LSQ_HIP_NORM_W8_H_
#define LSQ_HIP_NORM_W8_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_NORM_W8_ABI_VERSION 1
#define LSQ_NORM_W8_U8 0
#define LSQ_NORM_W8_I8 1
#define LSQ_NORM_W8_LAYER 0
#define LSQ_NORM_W8_RMS 1
#define LSQ_NORM_W8_MAX_C 65536
/* out8[0] of the plan */
#define LSQ_NORM_W8_GENERIC 0           /* one wave per row, two passes over its bytes */
#define LSQ_NORM_W8_PACKETS 1           /* a row in the registers of a group of lanes, read once as 16-byte packets */
/* out8[6] of the plan: where a lane's w and bias values live */
#define LSQ_NORM_W8_PARAMS_NONE 0       /* neither weight nor bias (PACKETS), or read from memory as they are needed (GENERIC) */
#define LSQ_NORM_W8_PARAMS_REGS 1       /* loaded once per lane into registers */
#define LSQ_NORM_W8_PARAMS_LDS 2        /* staged once per workgroup into LDS as float32 */

/* The geometry of one call: x and y are R rows of C elements. */
typedef struct lsq_norm_w8_geom {
    int64_t R, C;
    int64_t kind;           /* LSQ_NORM_W8_LAYER / LSQ_NORM_W8_RMS */
    int64_t x_dtype;        /* LSQ_NORM_W8_U8 / LSQ_NORM_W8_I8 */
} lsq_norm_w8_geom;

/* The constants: `s_x` one float32 and `zx` one int32 ON THE DEVICE, read in the kernel as they are; `weight` and `bias` C values of
 * param_dtype each on the device, or NULL; `out_scale` and `out_shift` one float32 each on the device, or both NULL for a floating
 * y of mid_dtype. */
typedef struct lsq_norm_w8_consts {
    const void* s_x;
    const void* zx;
    const void* weight;
    const void* bias;
    const void* out_scale;
    const void* out_shift;
    int64_t param_dtype, quant_min, quant_max, type_min, type_max, mid_dtype;
    float eps;
} lsq_norm_w8_consts;

/* LSQ_NORM_W8_ABI_VERSION the library was built with. */
int lsq_norm_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_norm_w8_last_error(void);

/* The norm: y R rows of C bytes (uint8 for an output range in 0..255, int8 for one in -128..127) or of C mid_dtype floats. */
int lsq_norm_w8(const lsq_norm_w8_geom* geom, const lsq_norm_w8_consts* consts, const void* x_levels, void* y, void* stream);

/* Host only, nothing is launched; without a GPU 256 compute units are assumed.  `aligned`: x is 16-byte aligned and so is y.
 * out8[0] = the kernel family (LSQ_NORM_W8_*): PACKETS needs C % 16 == 0, C <= 8192 and `aligned`; every other legal call is
 *           GENERIC;
 * out8[1] = workgroups, out8[2] = threads per workgroup (256);
 * out8[3] = L, the lanes of a row's group, and out8[4] = P, the 16-byte packets per lane.  PACKETS: of all P in 1..8 with
 *           L = the power of two in 4..64 that holds ceil(C / 16 / P) lanes, the pair with the fewest masked lanes
 *           L - ceil(C / 16 / P), then the smallest P; lane l takes the row's packets l, l + L, ...  GENERIC: 64 and 0;
 * out8[5] = rows per workgroup: (256 / L) groups times K rows each (K = 8, halved while the grid holds fewer than two workgroups
 *           per compute unit); group g of workgroup b takes the rows b out8[5] + g + k 256 / L, k < K.  GENERIC: 4, one per wave;
 * out8[6] = where w and bias live (LSQ_NORM_W8_PARAMS_*): REGS for P == 1, LDS above; `has_weight` / `has_bias`: given or not;
 * out8[7] = LDS bytes: 4 C for each of weight and bias with PARAMS_LDS, else 0. */
int lsq_norm_w8_plan(const lsq_norm_w8_geom* geom, int aligned, int has_weight, int has_bias, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
