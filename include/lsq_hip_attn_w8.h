/* include/lsq_hip_attn_w8.h -- the attention core on 8-bit LEVELS on gfx950: a batched matmul of two per-tensor level tensors and a
 * softmax whose exponential is a 256-entry integer table.  What keeps softmax(q k^T) v of a converted token block in levels between
 * its qkv and its proj layer.
 *
 * Exported by `liblsq_hip_attn_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/attn_w8/ for gfx950), the sixteenth companion
 * of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of lsq_hip.h,
 * and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device buffers, kernels enqueued on
 * `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation, no atomics, no environment
 * variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is validated before anything is
 * enqueued; lsq_attn_w8_last_error() describes the calling thread's last failure.  Launches repeat bit for bit.
 *
 * BATCHED MATMUL (lsq_bmm_w8).  A is levels [B0, B1, M, K]; B is levels [B0, B1, N, K] (LSQ_ATTN_W8_NT: q k^T, both contiguous
 * along K) or [B0, B1, K, N] (LSQ_ATTN_W8_NN: p v, B contiguous along N); y is [B0, B1, M, N].  Each operand is uint8 or int8 on its
 * own, with one (scale float32, zero point int32) ON THE DEVICE, read in the kernel.  All three tensors are strided: the innermost
 * stride is 1, the row stride `ld` and the two batch strides (in elements) are given per tensor.  With la, lb the levels:
 *     I = sum_k (la - za) (lb - zb)                 exact (|I| may pass 2^31: 64 bits; K <= 65536)
 *     v = (s_b * float(I)) * s_a                    fp32, two rounded multiplies, never contracted: lsq_linear_w8a8's steps with B
 *                                                   in the weight's role and no bias
 *     u = round_to(mid, v)                          mid = mid_dtype: LSQ_F32 (identity), LSQ_BF16, LSQ_F16
 *     with out_scale:  y = level(u; out) mod 256    lsq_math.hpp's level() with make_qparams(sanitize_scale_per_tensor(out_scale[0]),
 *                                                   out_shift[0], range); a NaN goes to quant_min; uint8 / int8 by the range
 *     without:         y = u, stored as mid
 * Bytes outside the logical y (between rows, between batches) are never written.
 * The zero points are expected within -32768..32767 (a quantizer's lies inside its type's range).  Beyond that the result is not
 * specified where I leaves 64 bits, but nothing faults and no signed step overflows: they are widened to 64 bits before the first
 * subtraction and the sums wrap.  A's and B's rows and batches may overlap or repeat (a batch stride of 0); y's may not.
 *
 * SOFTMAX (lsq_softmax_w8).  x is R rows of C level bytes with row stride ldx >= C, y R rows with row stride ldy >= C (elements);
 * `table` is int32 [256] on the device with 0 <= table[d] <= 2^24 and table[0] >= 1.  Per row, b_i the level as an integer:
 *     m = max_i b_i      d_i = m - b_i  (0..255)      E_i = table[d_i]      S = sum_i E_i   (an exact integer <= 2^40, >= 1)
 *     r = 1.0f / float(S)                           one conversion (round to nearest even), one IEEE division per row
 *     p_i = float(E_i) * r                          float(E_i) is exact; one rounded multiply
 *     u_i = round_to(mid, p_i)      y_i = level(u_i; out) mod 256, or u_i stored as mid
 * Neither the scale nor the zero point of x is read: they live in the table (torchlsq.functional.lsq_softmax_table:
 * table[d] = rint(exp(-(s_x alpha) d) 2^24) in float64).  There is no summation order, no exp and no NaN.  A table outside its
 * contract gives unspecified numbers and no fault: the index is always a byte.
 * THE BOUND.  Let t = s_x alpha, e_d = exp(-t d), p*_i = e_{d_i} / sum_j e_{d_j} the softmax in real arithmetic of alpha s_x b.
 * table[d] = 2^24 e_d + h_d with |h_d| <= 1/2 (+ the float64 exp's last place, < 2^-28 of a unit).  Then E_i / S differs from
 * p*_i by at most (1/2 + p*_i C / 2) / S' <= (1 + C p*_i) / (2 S), S' the exact 2^24 sum e: half a table unit relative to S for the
 * numerator and p*_i times the C half units of the denominator.  float(S) and the division and the multiply are three roundings
 * of relative 2^-24 each: |p_i - E_i / S| <= 3 * 2^-24 p_i (1 + 2^-23) < 2^-22 p_i.  Together
 *     |p_i - p*_i| <= 2^-22 p_i + (1 + C p*_i) / (2 S),     S >= table[0] = 2^24.
 * THIS IS NOT ATen's softmax: against F.softmax of the dequantized values taken to levels, outputs differ by at most one level
 * (DESIGN.md 9.15).
 *
 * Both ops' GPU results equal the package's CPU path (int64 torch ops, torch float32 ops one at a time, the existing levels op)
 * bit for bit, the softmax for the same table.
 *
 * THE PACKET FAMILIES READ WHOLE 16-BYTE PACKETS.  With bases and strides that are multiples of 16 the contiguous extent (K of
 * A; K of an NT B, N of an NN B; C of x) need not be one: the bytes of a row's last packet beyond the extent are read and masked in
 * registers, so what they hold never matters -- but they must be readable: ld >= the extent and ld % 16 == 0 put them inside the
 * row's stride, also for the last row.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): a NULL geometry, constants or buffer; NULL or misaligned scales, zero
 * points, out_scale, out_shift (the last two come together), table; a form that is not NT / NN; a level dtype that is not U8 / I8;
 * a mid_dtype that is not LSQ_F32 / LSQ_BF16 / LSQ_F16; an extent < 1; K or C > 65536; M, N or B0 * B1 > 2^20, R beyond 29 bits, a
 * grid beyond 2^24 - 1 workgroups (of 256 threads: the launch stays below 2^32 threads, which every runtime accepts); a row stride smaller than the row; a negative batch stride; a y whose rows or batches overlap
 * each other (strides sorted, each must clear the span below it), or that overlaps an operand, or that is not element-aligned;
 * an output range that is empty or lies neither within 0..255 nor within -128..127; a NULL out8.
 */
#ifndef LSQ_HIP_ATTN_W8_H_
#define LSQ_HIP_ATTN_W8_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_ATTN_W8_ABI_VERSION 1
#define LSQ_ATTN_W8_U8 0
#define LSQ_ATTN_W8_I8 1
#define LSQ_ATTN_W8_NN 0                /* B is [.., K, N] */
#define LSQ_ATTN_W8_NT 1                /* B is [.., N, K] */
#define LSQ_ATTN_W8_MAX_K 65536
#define LSQ_ATTN_W8_MAX_C 65536
/* out8[0] of both plans */
#define LSQ_ATTN_W8_GENERIC 0           /* bmm: a thread per output, 64-bit integers; softmax: a wave per row, three passes */
#define LSQ_ATTN_W8_MFMA 1              /* bmm: v_mfma_i32_16x16x64_i8 on 64 x 64 output tiles */
#define LSQ_ATTN_W8_PACKETS 1           /* softmax: a row in the registers of a group of lanes, read once as 16-byte packets */
/* out8[7] of the bmm plan: how y is stored */
#define LSQ_ATTN_W8_STORE_ELEMS 0       /* element by element (floats; levels into a y that is not packet-aligned) */
#define LSQ_ATTN_W8_STORE_PACKETS 1     /* the level tile through LDS as 16-byte packets; a row's last partial packet byte by byte */

/* One strided [B0, B1, rows, cols] tensor: the innermost stride is 1; `ld` between rows, `s0`, `s1` between batches, in elements. */
typedef struct lsq_attn_w8_strides {
    int64_t s0, s1, ld;
} lsq_attn_w8_strides;

typedef struct lsq_bmm_w8_geom {
    int64_t B0, B1, M, N, K;
    int64_t form;           /* LSQ_ATTN_W8_NN / LSQ_ATTN_W8_NT */
    int64_t a_dtype, b_dtype;   /* LSQ_ATTN_W8_U8 / LSQ_ATTN_W8_I8 */
    lsq_attn_w8_strides a, b, y;
} lsq_bmm_w8_geom;

/* The output side of both ops: `out_scale` and `out_shift` one float32 each on the device, or both NULL for a floating y of mid_dtype. */
typedef struct lsq_attn_w8_out {
    const void* out_scale;
    const void* out_shift;
    int64_t quant_min, quant_max, type_min, type_max, mid_dtype;
} lsq_attn_w8_out;

/* The operands' constants: one float32 and one int32 each ON THE DEVICE. */
typedef struct lsq_bmm_w8_consts {
    const void* s_a;
    const void* z_a;
    const void* s_b;
    const void* z_b;
} lsq_bmm_w8_consts;

typedef struct lsq_softmax_w8_geom {
    int64_t R, C, ldx, ldy;
    int64_t x_dtype;        /* LSQ_ATTN_W8_U8 / LSQ_ATTN_W8_I8 */
} lsq_softmax_w8_geom;

/* LSQ_ATTN_W8_ABI_VERSION the library was built with. */
int lsq_attn_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_attn_w8_last_error(void);

/* y = A B^T (NT) or A B (NN) per batch: bytes (uint8 for an output range in 0..255, int8 for one in -128..127) or mid_dtype floats. */
int lsq_bmm_w8(const lsq_bmm_w8_geom* geom, const lsq_bmm_w8_consts* consts, const lsq_attn_w8_out* out, const void* a_levels,
               const void* b_levels, void* y, void* stream);

/* Host only, nothing is launched.  `ab_aligned`: the bases of A and B are 16-byte aligned; `y_aligned`: y's is.
 * out8[0] = the family: MFMA needs `ab_aligned` and every stride of A and B a multiple of 16; every other legal call is GENERIC;
 * out8[1] = the form; out8[2] = workgroups; out8[3] = threads per workgroup (256);
 * out8[4] = rows of a workgroup's tile (MFMA: 64, four waves of 16; a workgroup takes one batch, 64 rows and 64 columns; GENERIC: 0,
 *           a thread per output);
 * out8[5] = columns of that tile (MFMA: 64);
 * out8[6] = static LDS bytes (MFMA: 5120: NN stages 64 x 64 bytes of B transposed in rows of 80; the level tile is 4096);
 * out8[7] = the store kind (LSQ_ATTN_W8_STORE_*): PACKETS for MFMA with `levels_out`, `y_aligned` and y's strides multiples of 16. */
int lsq_bmm_w8_plan(const lsq_bmm_w8_geom* geom, int ab_aligned, int y_aligned, int levels_out, int32_t* out8);

/* Softmax over the C bytes of each row; table int32 [256] on the device. */
int lsq_softmax_w8(const lsq_softmax_w8_geom* geom, const lsq_attn_w8_out* out, const void* table, const void* x_levels, void* y,
                   void* stream);

/* Host only.  `aligned`: x and y are 16-byte aligned.
 * out8[0] = the family: PACKETS needs `aligned`, ldx % 16 == 0, ldy % 16 == 0 and C <= 8192; every other legal call is GENERIC;
 * out8[1] = workgroups; out8[2] = threads per workgroup (256);
 * out8[3] = L, the lanes of a row's group, and out8[4] = P, the 16-byte packets per lane.  PACKETS: with n = ceil(C / 16) packets,
 *           P = the smallest of 1, 2, 4, 8 with ceil(n / P) <= 64 and L = the power of two in 4..64 that holds ceil(n / P) lanes;
 *           lane l takes the row's packets l, l + L, ...  GENERIC: 64 and 0;
 * out8[5] = rows per workgroup: (256 / L) groups times K rows each, K = 4 where that still leaves 512 workgroups, else 1; group g
 *           of workgroup b takes the rows b out8[5] + g + k 256 / L, k < K.  GENERIC: 4, one per wave;
 * out8[6] = LDS bytes (PACKETS: 1024, the table; GENERIC: 0);  out8[7] = 0. */
int lsq_softmax_w8_plan(const lsq_softmax_w8_geom* geom, int aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
