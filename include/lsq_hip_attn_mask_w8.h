/* include/lsq_hip_attn_mask_w8.h -- the MASKED softmax on 8-bit LEVELS on gfx950: the integer-table softmax of lsq_hip_attn_w8.h
 * applied to a PREFIX of every row.  A causal mask and a right-padded key mask both say "row r sees its first n_r keys"; that is
 * what decoder blocks, decode against a KV cache (Tq = 1, Tk keys written so far) and padded encoder batches need.
 *
 * Exported by `liblsq_hip_attn_mask_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/attn_mask_w8/ for gfx950), the eighteenth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows `lsq_attn_w8_out`, the level dtype
 * and family codes of lsq_hip_attn_w8.h and the status codes of lsq_hip.h, and the library imports no symbol of the others.  Same
 * contract as lsq_hip.h: caller-owned device buffers, kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default
 * stream), no allocation, no synchronisation, no atomics, no workspace, no environment variables, 0 / negative LSQ_E* / positive
 * hipError_t returns, never throws, everything is validated before anything is enqueued; lsq_attn_mask_w8_last_error() describes
 * the calling thread's last failure.  Launches repeat bit for bit.
 *
 * THE DEFINITION.  x is [.., Tq, Tk] levels, uint8 or int8, collapsed to R rows of C = Tk bytes with row stride ldx >= C, y R rows
 * with row stride ldy >= C (elements), as in lsq_softmax_w8; `table` is int32 [256] on the device with 0 <= table[d] <= 2^24 and
 * table[0] >= 1.  Row r has a prefix length
 *     t   = r mod Tq                                  the row's index inside its [Tq, Tk] matrix
 *     n_r = C
 *           causal:       n_r = min(n_r, t + 1 + causal_offset)                   causal_offset >= 0
 *           key_lengths:  n_r = min(n_r, max(key_lengths[r / rows_per_length], 0))
 * `key_lengths` is int32 [R / rows_per_length] ON THE DEVICE, read in the kernel and never on the host; values below 0 or above C
 * are clamped as shown.  (causal_offset = Tk - Tq is the KV-cache convention: the last query sees every key; it is the diagonal
 * for Tq == Tk.)  For i < n_r, b_i the level as an integer:
 *     m = max of b_i over the prefix      E_i = table[m - b_i]      S = sum of E_i over the prefix   (an exact integer)
 *     r = 1.0f / float(S)                 p_i = float(E_i) * r
 * and for i >= n_r, p_i = +0.0f.  The rest is lsq_softmax_w8's: u_i = round_to(mid, p_i), y_i = level(u_i; out) mod 256, or u_i
 * stored as mid.  A ROW WITH n_r = 0 IS ALL p = 0 AND NOTHING IS DIVIDED: a stated difference from ATen, which gives NaN.
 * Hence, bit for bit: y[r, :n_r] equals lsq_softmax_w8 of x[r, :n_r] with the same table and output side; y[r, n_r:] is the
 * output side's level of 0.0 (+0.0 for a floating y); with no mask active y equals lsq_softmax_w8's.
 *
 * BYTES OF x AT i >= n_r NEVER INFLUENCE THE RESULT: they may be uninitialised (unwritten KV-cache slots).  The packet kernels read
 * the 16-byte packet that contains byte n_r - 1 whole (its bytes from n_r on are masked in registers), so that packet must be
 * readable -- ldx >= C and ldx % 16 == 0 put it inside the row's stride --, and load no packet that lies wholly beyond n_r.
 *
 * THE BOUND of lsq_hip_attn_w8.h carries over with C replaced by n_r: for i < n_r,
 *     |p_i - p*_i| <= 2^-22 p_i + (1 + n_r p*_i) / (2 S),     S >= table[0] = 2^24,
 * p* the softmax in real arithmetic of alpha s_x b over the prefix; against F.softmax of the dequantized scores with -inf added
 * beyond the prefix, taken to levels, outputs differ by at most one level (rows with n_r >= 1).
 *
 * The GPU result equals the package's CPU path (int64 torch ops, torch float32 ops one at a time, the existing levels op) bit for
 * bit for the same table.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): everything lsq_softmax_w8 refuses (a NULL geometry, output description or
 * buffer; NULL or misaligned out_scale, out_shift (they come together), table; a level dtype that is not U8 / I8; a mid_dtype that
 * is not LSQ_F32 / LSQ_BF16 / LSQ_F16; R or C < 1; C > 65536; R beyond 29 bits; a grid beyond 2^24 - 1 workgroups; a row stride
 * smaller than the row; a y that overlaps x or the table or is not element-aligned; an output range that is empty or lies
 * neither within 0..255 nor within -128..127; a NULL out8); Tq < 1 or R % Tq != 0; with lengths: rows_per_length < 1,
 * rows_per_length % Tq != 0 or R % rows_per_length != 0, a key_lengths pointer that is not 4-byte aligned, a y that overlaps
 * key_lengths; causal not 0 or 1; causal_offset < 0 or beyond 31 bits.
 */
#ifndef LSQ_HIP_ATTN_MASK_W8_H_
#define LSQ_HIP_ATTN_MASK_W8_H_

#include "lsq_hip_attn_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_ATTN_MASK_W8_ABI_VERSION 1

typedef struct lsq_softmax_mask_w8_geom {
    int64_t R, C, ldx, ldy;
    int64_t x_dtype;            /* LSQ_ATTN_W8_U8 / LSQ_ATTN_W8_I8 */
    int64_t Tq;                 /* rows of one [Tq, Tk] matrix: t = r mod Tq */
    int64_t rows_per_length;    /* rows that share one entry of key_lengths (read with lengths only) */
    int64_t causal;             /* 0 / 1 */
    int64_t causal_offset;      /* row t sees its first t + 1 + causal_offset keys */
} lsq_softmax_mask_w8_geom;

/* LSQ_ATTN_MASK_W8_ABI_VERSION the library was built with. */
int lsq_attn_mask_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_attn_mask_w8_last_error(void);

/* Softmax over the first n_r of the C bytes of each row; table int32 [256] and key_lengths int32 [R / rows_per_length] (or NULL:
 * no lengths) on the device. */
int lsq_softmax_mask_w8(const lsq_softmax_mask_w8_geom* geom, const lsq_attn_w8_out* out, const void* table, const void* key_lengths,
                        const void* x_levels, void* y, void* stream);

/* Host only, nothing is launched.  `aligned`: x and y are 16-byte aligned; `has_lengths`: the call will come with key_lengths.
 * out8 has lsq_softmax_w8_plan's layout and, for the same C, strides and alignment, its values:
 * out8[0] = the family: LSQ_ATTN_W8_PACKETS needs `aligned`, ldx % 16 == 0, ldy % 16 == 0 and C <= 8192; every other legal call is
 *           LSQ_ATTN_W8_GENERIC (a wave per row, three passes over i < n_r, then the zero tail);
 * out8[1] = workgroups; out8[2] = threads per workgroup (256);
 * out8[3] = L, the lanes of a row's group, and out8[4] = P, the 16-byte packets per lane, by lsq_softmax_w8_plan's rule applied
 *           to C (not to n_r, which the host never knows); GENERIC: 64 and 0;
 * out8[5] = rows per workgroup: (256 / L) groups times K rows each, K = 4 where that still leaves 512 workgroups, else 1; group g
 *           of workgroup b takes the rows b out8[5] + g + k 256 / L, k < K.  GENERIC: 4, one per wave;
 * out8[6] = LDS bytes (PACKETS: 1024, the table; GENERIC: 0);  out8[7] = 0. */
int lsq_softmax_mask_w8_plan(const lsq_softmax_mask_w8_geom* geom, int aligned, int has_lengths, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
