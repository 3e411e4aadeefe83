/* include/lsq_hip_attn_decode_split_w8.h -- SPLIT-KEY decode attention on 8-bit LEVELS on gfx950: the definition of
 * lsq_hip_attn_decode_w8.h, word for word, with one kv head's keys dealt to SEVERAL workgroups -- for small batches against long
 * caches, where one workgroup per (b, kv head) leaves most of the part idle, and for caches beyond that kernel's 8192 keys.
 *
 * Exported by `liblsq_hip_attn_decode_split_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/attn_decode_split_w8/ for gfx950), the
 * twenty-second companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the structs
 * `lsq_attn_decode_w8_geom` and `lsq_attn_decode_w8_consts` of lsq_hip_attn_decode_w8.h and `lsq_attn_w8_out` of lsq_hip_attn_w8.h,
 * and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device buffers -- the WORKSPACE
 * included --, the kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no
 * synchronisation, no atomics, no environment variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws,
 * everything is validated before anything is enqueued; lsq_attn_decode_split_w8_last_error() describes the calling thread's last
 * failure.  Launches repeat bit for bit, and the result never depends on what the workspace held before the call.
 *
 * THE DEFINITION is lsq_hip_attn_decode_w8.h's: q [B, H, Tq, D], k and v [B, Hkv, Tk, D], n(b, t) the same function of `causal`
 * and `key_lengths`, keys at or beyond n take no part and are never read.  Every intermediate of that definition is a defined byte
 * or an exact integer without a summation order -- the score byte s_j, the row's byte maximum, S = sum table[m - s_j], the
 * probability byte p_j, I = sum (p_j - z_p)(lv_j - z_v) -- so a partition of the keys changes none of them: the bytes are the
 * decode kernel's and the CPU path's, BIT FOR BIT, for every number of splits.  There is no rescaling and no tolerance.
 *
 * THREE LAUNCHES on one stream, no grid-wide synchronisation.  With a chunk C, a multiple of 64 keys, and S = ceil(Tk / C) splits,
 * workgroup (b, kv head, s) of launches 1 and 2 owns the keys [s C, min((s + 1) C, nmax)), nmax = n(b, Tq - 1) read on the device;
 * a workgroup whose chunk starts at or beyond nmax returns at once.
 *   1 SCORES   the R = G Tq <= 16 rows are one row tile of the matrix core, k's rows the B operand straight from memory; the score
 *              bytes of the rows < R go to the workspace [B Hkv][R][ldw], ldw = 16 ceil(Tk / 16), as 16-byte packets through LDS.
 *   2 CONTEXT  per row the byte maximum and the exact sum S over the row's WHOLE prefix, read from that workspace (the same for
 *              every split of a head: an exact 64-bit integer, order-free); then per 64-key step of the chunk the probability
 *              bytes (the byte z_p in [n_r, chunk end)) into LDS, times v's rows staged transposed and double buffered; the
 *              chunk's exact integer I_c[r][d], zero-point corrected with the chunk's own key count, goes to the workspace
 *              [B Hkv][S][R][D] as int64.
 *   3 REDUCE   one workgroup per (b, kv head): I = sum of I_c over the chunks that START BELOW nmax and only those -- unwritten
 *              workspace is never read --, float(I) correctly rounded, the context side's two multiplies, mid, level, store
 *              (packets where y allows, bytes otherwise).  n = 0 gives the context quantizer's level of 0.0.
 * LDS does not scale with Tk or with the chunk: 4352 bytes in launch 1, 3840 + 160 D in launch 2, 16 D in launch 3.
 *     workspace bytes = B Hkv R ldw  +  8 B Hkv S R D
 *
 * `splits`: 0 = the library's own choice; s >= 1 asks for AT MOST s splits: C = 64 ceil(ceil(Tk / 64) / s) and S = ceil(Tk / C),
 * which is s wherever s divides ceil(Tk / 64) and never more.  The plan reports C and S.  The library's own choice: that C for the
 * fewest splits s with B Hkv s >= LSQ_ATTN_DECODE_SPLIT_W8_WG_PER_CU * LSQ_ATTN_DECODE_SPLIT_W8_CUS workgroups, at most
 * LSQ_ATTN_DECODE_SPLIT_W8_MAX_SPLITS, taken into [LSQ_ATTN_DECODE_SPLIT_W8_MIN_CHUNK, LSQ_ATTN_DECODE_SPLIT_W8_MAX_CHUNK] (host
 * only: the CU count is the MI355X's, no device is asked).
 *
 * SERVED (plan family LSQ_ATTN_DECODE_SPLIT_W8_SPLIT): R = G Tq <= 16; D % 16 == 0 and 16 <= D <= 128; Tk <= 65536, the API's own
 * limit; the bases of q, k and v 16-byte aligned and every stride of theirs a multiple of 16; for lsq_attn_decode_split_w8 a
 * workspace that is 16-byte aligned and at least the reported size.  Every other legal call has the plan family
 * LSQ_ATTN_DECODE_SPLIT_W8_COMPOSITION: lsq_attn_decode_split_w8 REFUSES it and the caller composes lsq_hip_attn_w8.h and
 * lsq_hip_attn_mask_w8.h.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): those of lsq_attn_decode_w8, and: `splits` < 0 or > ceil(Tk / 64); a NULL
 * `bytes`; a NULL or misaligned workspace, or one smaller than lsq_attn_decode_split_w8_workspace reports; a workspace that overlaps
 * q, k, v, y, the table or key_lengths.
 */
#ifndef LSQ_HIP_ATTN_DECODE_SPLIT_W8_H_
#define LSQ_HIP_ATTN_DECODE_SPLIT_W8_H_

#include "lsq_hip_attn_decode_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_ATTN_DECODE_SPLIT_W8_ABI_VERSION 1
/* out8[0] of the plan */
#define LSQ_ATTN_DECODE_SPLIT_W8_COMPOSITION 0      /* legal, not served: the caller composes the existing ops */
#define LSQ_ATTN_DECODE_SPLIT_W8_SPLIT 1            /* three launches, S workgroups per (b, kv head) in the first two */
#define LSQ_ATTN_DECODE_SPLIT_W8_MAX_ROWS 16
#define LSQ_ATTN_DECODE_SPLIT_W8_MAX_TK 65536
#define LSQ_ATTN_DECODE_SPLIT_W8_MAX_D 128
#define LSQ_ATTN_DECODE_SPLIT_W8_THREADS 256
/* the library's own choice of the chunk (splits = 0): the constants of the chunk sweeps in profiles/r30_attn_decode_split_w8_ab.txt */
#define LSQ_ATTN_DECODE_SPLIT_W8_MIN_CHUNK 256
#define LSQ_ATTN_DECODE_SPLIT_W8_MAX_CHUNK 2048
#define LSQ_ATTN_DECODE_SPLIT_W8_WG_PER_CU 4
#define LSQ_ATTN_DECODE_SPLIT_W8_MAX_SPLITS 64        /* every split sums its rows' whole prefix again */
#define LSQ_ATTN_DECODE_SPLIT_W8_CUS 256

/* LSQ_ATTN_DECODE_SPLIT_W8_ABI_VERSION the library was built with. */
int lsq_attn_decode_split_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_attn_decode_split_w8_last_error(void);

/* Host only.  *bytes = the workspace lsq_attn_decode_split_w8 needs for this geometry and `splits` (B Hkv R ldw + 8 B Hkv S R D);
 * 0 for a geometry whose extents alone make it COMPOSITION (R > 16, D not served). */
int lsq_attn_decode_split_w8_workspace(const lsq_attn_decode_w8_geom* geom, int64_t splits, int64_t* bytes);

/* y = the context's levels of lsq_attn_decode_w8, same arguments; `workspace`: `workspace_bytes` bytes on the device, 16-byte
 * aligned, at least what lsq_attn_decode_split_w8_workspace reports for (geom, splits), overlapping no operand; its contents before
 * the call do not matter and are undefined after it. */
int lsq_attn_decode_split_w8(const lsq_attn_decode_w8_geom* geom, const lsq_attn_decode_w8_consts* consts, const lsq_attn_w8_out* scores_out,
                             const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out, const void* table, const void* key_lengths,
                             const void* q_levels, const void* k_levels, const void* v_levels, void* y, void* workspace,
                             int64_t workspace_bytes, int64_t splits, void* stream);

/* Host only, nothing is launched.  `qkv_aligned`: the bases of q, k and v are 16-byte aligned; `y_aligned`: y's is.
 * out8[0] = the family (LSQ_ATTN_DECODE_SPLIT_W8_*); for COMPOSITION the other slots are 0;
 * out8[1] = workgroups of launches 1 and 2 each = B Hkv S (launch 3 has B Hkv = out8[1] / out8[5]);
 * out8[2] = threads per workgroup (256 in all three); out8[3] = R = G Tq, the query rows of a workgroup;
 * out8[4] = the chunk C in keys; out8[5] = the splits S = ceil(Tk / C);
 * out8[6] = LDS bytes of launch 2, the largest of the three = 3840 + 160 D;
 * out8[7] = the store kind (LSQ_ATTN_W8_STORE_*): PACKETS with `y_aligned` and y's strides multiples of 16. */
int lsq_attn_decode_split_w8_plan(const lsq_attn_decode_w8_geom* geom, int qkv_aligned, int y_aligned, int64_t splits, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
