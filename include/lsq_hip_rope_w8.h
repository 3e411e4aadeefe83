/* include/lsq_hip_rope_w8.h -- ROTARY POSITION EMBEDDING and the KV-CACHE APPEND on 8-bit LEVELS on gfx950: what stands between the
 * qkv projection and q k^T in a Llama-style block, and what puts a step's k and v into a [B, H, Tmax, D] cache at positions that
 * live on the device.  One launch, one byte read and one written per element (plus the tables), no float round trip.
 *
 * Exported by `liblsq_hip_rope_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/rope_w8/ for gfx950), the nineteenth companion
 * of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the status and dtype codes of lsq_hip.h, and
 * the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device buffers, kernels enqueued on
 * `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation, no atomics, no workspace, no
 * environment variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is validated before anything
 * is enqueued; lsq_rope_w8_last_error() describes the calling thread's last failure.  Launches repeat bit for bit.
 *
 * THE DEFINITION.  x is [B, T, H, D] levels, uint8 or int8, innermost stride 1, the three other strides x_sb, x_st, x_sh in
 * elements (a q, k or v view of a qkv buffer is read in place); y is [B, Tout, H, D] through y_sb, y_st, y_sh in elements of y
 * (a [B, H, Tmax, D] cache is y with y_sh = Tmax D and y_st = D).  `cos` and `sin` are float32 [P, R / 2] on the device, dense,
 * and hold VALUES OF mid_dtype; R, the rotary dimension, is even with 2 <= R <= D.  `positions` is int32 [B] on the device, or
 * NULL for zeros; it is read in the kernel and never on the host.  Token (b, t) has the position p = positions[b] + t.
 * With mid in {float32, bfloat16, float16}; every fp32 step is one correctly rounded operation and no multiply is ever fused with
 * the add or subtract that follows it:
 *     d(l)  = float(round_to(mid, (float(l) - float(zx)) * s_x))
 *     pair (i, j), table column col:   LSQ_ROPE_W8_HALF         j = i + R / 2,  i < R / 2,  col = i
 *                                      LSQ_ROPE_W8_INTERLEAVED  (i, j) = (2 col, 2 col + 1),  col < R / 2
 *     c = cos[p, col],  s = sin[p, col]
 *     u_i = round_to(mid, float(round_to(mid, d(l_i) * c)) - float(round_to(mid, d(l_j) * s)))
 *     u_j = round_to(mid, float(round_to(mid, d(l_j) * c)) + float(round_to(mid, d(l_i) * s)))
 *     features R .. D - 1 (partial rotary):  u = d(l)
 *     y = level(u; out) mod 256 (a NaN goes to quant_min), or u itself stored as mid
 *
 * WHERE A TOKEN GOES.  scatter = 0: token (b, t) is written at output token t (Tout >= T).  scatter = 1: at output token p.
 * A token is NOT WRITTEN AT ALL -- no byte of y changes, no byte of x or of the tables is read for it -- where p < 0 or p >= P,
 * and, with scatter, where p >= Tout: device values cannot be refused on the host.  Bytes outside the logical y are never written.
 *
 * LSQ_ROPE_W8_COPY (for v, and for a k that is rotated already): no tables, no input or output side and no arithmetic, y byte =
 * x byte; the same placement with P replaced by Tout.  x and y are both one byte per element.
 *
 * THE BOUND.  Against the rotation in real arithmetic of the real values x = (l - zx) s_x with the float64 cos and sin that the
 * tables were rounded from (once to float32, once to mid), where nothing underflows: each of x, the table entry, the product and
 * the sum is rounded once in fp32 and once to mid, so with u the unit roundoff of mid (2^-24, 2^-8, 2^-11)
 *     |u_i - (x_i c - x_j s)| <= ((1 + u)^4 (1 + 2^-24)^4 - 1) (|x_i c| + |x_j s|)        and the same for u_j,
 *     |u - x| <= ((1 + u)(1 + 2^-24) - 1) |x|                                             for a feature beyond R.
 *
 * The GPU result equals the package's CPU path (LevelsTensor.dequantize(mid), torch.mul, torch.sub / torch.add on mid tensors, the
 * existing levels op) bit for bit.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): a NULL geometry, x, y or out8; ROTATE: a NULL input side, s_x, zx,
 * output description, cos or sin; s_x, zx, out_scale, out_shift, cos, sin or positions not 4-byte aligned; a floating y not
 * element-aligned; an extent below 1 or beyond 29 bits; more than 2^40 elements; a negative stride or one that takes an offset
 * beyond 2^58; R odd, below 2 or above D; P below 1 or beyond 29 bits; scatter = 0 with Tout < T; a y stride pattern under which
 * two (b, token, h) rows overlap; y overlapping x, the tables or positions; x_dtype not U8 / I8; style, scatter or mode not 0 / 1;
 * a mid_dtype that is not LSQ_F32 / LSQ_BF16 / LSQ_F16; NULL out_scale or out_shift alone; an output range that is empty or lies
 * neither within 0..255 nor within -128..127; COPY with an input side, an output side, cos or sin given; a grid beyond 2^24 - 1
 * workgroups; in the plan, `aligned` not 0, 1, 2 or 4 (COPY: not 0 or 1).
 */
#ifndef LSQ_HIP_ROPE_W8_H_
#define LSQ_HIP_ROPE_W8_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_ROPE_W8_ABI_VERSION 1

#define LSQ_ROPE_W8_U8 0
#define LSQ_ROPE_W8_I8 1
#define LSQ_ROPE_W8_HALF 0          /* pairs (i, i + R / 2): HF's rotate_half */
#define LSQ_ROPE_W8_INTERLEAVED 1   /* pairs (2 i, 2 i + 1) */
#define LSQ_ROPE_W8_ROTATE 0
#define LSQ_ROPE_W8_COPY 1
#define LSQ_ROPE_W8_GENERIC 0
#define LSQ_ROPE_W8_PACKETS 1

typedef struct lsq_rope_w8_geom {
    int64_t B, T, H, D, R, P, Tout;
    int64_t x_sb, x_st, x_sh;   /* the strides of x's B, T and H axes, in elements */
    int64_t y_sb, y_st, y_sh;   /* the strides of y's B, Tout and H axes, in elements of y */
    int64_t x_dtype;            /* LSQ_ROPE_W8_U8 / LSQ_ROPE_W8_I8 */
    int64_t style;              /* LSQ_ROPE_W8_HALF / LSQ_ROPE_W8_INTERLEAVED */
    int64_t scatter;            /* 0: token t goes to output token t; 1: to output token p */
    int64_t mode;               /* LSQ_ROPE_W8_ROTATE / LSQ_ROPE_W8_COPY (R, P, style are not read) */
} lsq_rope_w8_geom;

typedef struct lsq_rope_w8_in {     /* x's per-tensor constants on the device */
    const void* s_x;                /* float32 [1] */
    const void* zx;                 /* int32 [1] */
} lsq_rope_w8_in;

typedef struct lsq_rope_w8_out {    /* the output side: both pointers NULL for a floating y of mid_dtype */
    const void* out_scale;          /* float32 [1] */
    const void* out_shift;          /* float32 [1] */
    int64_t quant_min, quant_max, type_min, type_max;
    int64_t mid_dtype;              /* LSQ_F32 / LSQ_BF16 / LSQ_F16 */
} lsq_rope_w8_out;

/* LSQ_ROPE_W8_ABI_VERSION the library was built with. */
int lsq_rope_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_rope_w8_last_error(void);

/* ROTATE: y = the rotated x through the output side.  COPY: `in`, `out`, `cos` and `sin` must be NULL.  `positions`: int32 [B] on
 * the device or NULL. */
int lsq_rope_w8(const lsq_rope_w8_geom* geom, const lsq_rope_w8_in* in, const lsq_rope_w8_out* out, const void* cos, const void* sin,
                const void* positions, const void* x_levels, void* y, void* stream);

/* Host only, nothing is launched.  `aligned`: 0, or -- where x, y and the tables are 16-byte aligned -- the bytes of one element of
 * y (1: levels, 2 or 4: floats; COPY: 1).
 * out8[0] = the family.  LSQ_ROPE_W8_PACKETS needs `aligned`, D % 16 == 0, x strides that are multiples of 16, y strides that are
 *           multiples of 16 bytes, and for ROTATE R % 32 == 0 (HALF) or R % 16 == 0 (INTERLEAVED); every other legal call is
 *           LSQ_ROPE_W8_GENERIC (one lane per pair, per feature beyond R, or per byte in COPY);
 * out8[1] = workgroups; out8[2] = threads per workgroup (256);
 * out8[3] = heads per lane (PACKETS ROTATE: a lane keeps its cos and sin values and walks that many heads of its token with them:
 *           min(H, 4), halved while the grid holds fewer than two workgroups per compute unit; else 1);
 * out8[4] = work units per token and head (PACKETS HALF: R / 32 pairs of packets + (D - R) / 16 packets beyond R; INTERLEAVED and
 *           COPY: D / 16 packets; GENERIC: R / 2 + D - R lanes, COPY: D);
 * out8[5] = the units of them that rotate (COPY: 0);
 * out8[6] = LDS bytes (0);  out8[7] = the kernel: 0 generic, 1 packets HALF, 2 packets INTERLEAVED, 3 copy packets, 4 copy generic. */
int lsq_rope_w8_plan(const lsq_rope_w8_geom* geom, int aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
