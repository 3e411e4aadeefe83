/* include/lsq_hip_attn_chunk_w8.h -- CHUNKED PREFILL attention on 8-bit LEVELS on gfx950: the definition of lsq_hip_attn_decode_w8.h,
 * word for word, for ANY number of query rows against a cache of up to 65536 keys, dense or paged, plus a mask mode that counts
 * every row's keys back from `key_lengths` on the device -- a prompt fed in pieces into a growing cache with no host read-back.
 *
 * Exported by `liblsq_hip_attn_chunk_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/attn_chunk_w8/ for gfx950), the twenty-fourth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the structs
 * `lsq_attn_decode_w8_geom` and `lsq_attn_decode_w8_consts` of lsq_hip_attn_decode_w8.h, `lsq_attn_w8_out` of lsq_hip_attn_w8.h and
 * `lsq_attn_paged_w8_pages` of lsq_hip_attn_paged_w8.h, and the library imports no symbol of the others.  Same contract as lsq_hip.h:
 * caller-owned device buffers -- the WORKSPACE included --, the kernels enqueued on `stream` (a hipStream_t as void*, NULL = the
 * default stream), no allocation, no synchronisation, no atomics, no environment variables, 0 / negative LSQ_E* / positive
 * hipError_t returns, never throws, everything is validated before anything is enqueued; lsq_attn_chunk_w8_last_error() describes
 * the calling thread's last failure.  Launches repeat bit for bit, and the result never depends on what the workspace held.
 *
 * THE DEFINITION is lsq_hip_attn_decode_w8.h's: q [B, H, Tq, D], k and v [B, Hkv, Tk, D] with H = G Hkv, the score bytes, the
 * probability bytes of each row's prefix, I = sum over j < n of (p_j - z_p)(lv_j - z_v) and the context level unchanged; keys at or
 * beyond n take no part and their bytes are never read; n = 0 gives the context quantizer's level of 0.0.  The paged form
 * (lsq_attn_chunk_paged_w8) is that definition on the cache lsq_hip_attn_paged_w8.h's layout names: READS CLAMP, Tk = Mp ps.
 * geom->causal selects n(b, t):
 *     0   n = min(Tk, max(key_lengths[b], 0) where given)
 *     1   n = min(Tk, t + 1 + causal_offset, max(key_lengths[b], 0) where given)
 *     2   LSQ_ATTN_CHUNK_W8_CAUSAL_LENGTHS; needs key_lengths; causal_offset must be 0:
 *             L_b = min(Tk, max(key_lengths[b], 0)),    n(b, t) = max(0, L_b - (Tq - 1 - t))
 *         the last query row of batch entry b sees its L_b keys, the row before it one fewer, a row whose count would be negative
 *         none.  With Tq = 1 this is mode 1 with causal_offset = Tk - 1 and key_lengths.  It is what a prompt chunk appended to a
 *         cache wants: `key_lengths` = the lengths AFTER the append.
 * key_lengths is read in the kernels and never on the host.  Every intermediate of the definition is a byte or an exact integer
 * without a summation order, so neither a partition of the keys nor one of the query rows changes a bit: the bytes are the decode
 * kernel's, the prefill kernel's, the split kernels' and the CPU path's.  No rescaling, no tolerance.
 *
 * THREE LAUNCHES, those of lsq_hip_attn_decode_split_w8.h (one kernel text: csrc/attn_decode_split_w8/lsq_attn_split_core.hpp) with
 * the R = G Tq query rows of a kv head (r = g Tq + t) dealt to NT = ceil(R / 16) ROW TILES of 16, the tile a grid coordinate.  Tile i
 * holds the rows 16 i .. min(16 i + 15, R - 1); it may straddle two query heads.  With a chunk C (a multiple of 64 keys) and
 * S = ceil(Tk / C): launches 1 and 2 run B Hkv NT S workgroups, launch 3 B Hkv NT.  A tile's key loops end at
 *     nmax_tile = the largest n of the tile's live rows
 * (n is non-decreasing in t: n(b, Tq - 1) where the tile straddles a head border, else n of its last live row): a workgroup whose
 * chunk starts at or beyond nmax_tile returns before its first barrier, so the early tiles of a causal prompt skip the late chunks
 * and nothing above the diagonal is scored beyond chunk granularity; launch 2 reads a row's prefix only below
 * 16 ceil(n_r / 16) <= 16 ceil(nmax_tile / 16), which the same tile's launch-1 workgroups wrote; launch 3 sums only the chunks that
 * start below nmax_tile.  Unwritten workspace is never read.  LDS does not scale with Tk or Tq: 4352 bytes, then 3840 + 160 D, then
 * 2048.  No atomics, no flags, no scratch: the stream orders the launches.
 *     workspace bytes = B Hkv R ldw  +  8 B Hkv S R D,      ldw = 16 ceil(Tk / 16)   (paged: Mp ps)
 * which is LARGE in R: 512 tokens x G 4 x Tk 32768 are 64 MB of score bytes per kv head.
 *
 * `splits`: 0 = the library's own choice; s >= 1 asks for AT MOST s splits: C = 64 ceil(ceil(Tk / 64) / s), S = ceil(Tk / C).  The
 * library's own choice (row tiles already supply parallelism): that C for the fewest s with B Hkv NT s >=
 * LSQ_ATTN_CHUNK_W8_WG_PER_CU * LSQ_ATTN_CHUNK_W8_CUS workgroups, at most LSQ_ATTN_CHUNK_W8_MAX_SPLITS, C at least
 * LSQ_ATTN_CHUNK_W8_MIN_CHUNK and with NO upper bound: S = 1 is the normal case of a real prompt chunk, and launch 2 walks any chunk
 * in 64-key steps.  (Host only: the CU count is the MI355X's.)  The constants are what the sweep of the forced split count in
 * profiles/r33_attn_chunk_w8_ab.txt gave (H 32 on Hkv 8, D 128, 8192 and 32768 keys).  Where the rule splits (a
 * 16-token chunk at B 1: 32 tile workgroups) 4 workgroups per CU, S = 32, was the fastest at 32768 keys (388.9 us; 2 per CU 406.4,
 * 8 per CU 585.9); at 8192 keys the design's starting chunk floor of 256 keys (S = 32, 174.7 us in the earlier run that the profile
 * ends with) was 14 % behind chunks of 512 (S = 16, 150.6 us), so the floor ships as 512, which moves no other swept case; 64 and
 * 128 splits were 51 to 215 % behind the rule's choice.  Where the tiles fill the part (a 512-token chunk, B 1 and B 4) the rule
 * gives S = 1, and the fastest forced count (1, 4, 2, 2) was at most 4.7 % ahead of it.
 *
 * SERVED (plan family LSQ_ATTN_CHUNK_W8_CHUNK): any R >= 1; D % 16 == 0 and 16 <= D <= 128; Tk <= 65536; the bases of q, k and v
 * (the pools) 16-byte aligned and every stride of theirs a multiple of 16; paged: ps a power of two >= 16 and Mp ps <= 65536; at
 * most 2^24 - 1 workgroups (beyond that: refused, below); a workspace that is 16-byte aligned and at least the reported size.
 * Every other legal call has the family LSQ_ATTN_CHUNK_W8_COMPOSITION: the entries REFUSE it with LSQ_EINVAL, enqueue nothing, and
 * the caller (gathers the pages and) composes lsq_hip_attn_w8.h and lsq_hip_attn_mask_w8.h with per-row key counts.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): those of lsq_attn_decode_split_w8 and of lsq_attn_paged_w8_decode, said the
 * same way, and: geom->causal other than 0, 1 or 2; causal == 2 without key_lengths (has_lengths = 0); causal == 2 with a non-zero
 * causal_offset.  A GRID BEYOND 2^24 - 1 WORKGROUPS (B Hkv NT S) IS A REFUSAL, NOT A FAMILY, as in the split and the paged library:
 * the two entries, the two plans and the two workspace functions all return LSQ_EINVAL for it, so a caller -- the Python host, on
 * the GPU and on the CPU -- raises instead of composing a call of that size; fewer splits or a shorter chunk of the prompt is served.
 */
#ifndef LSQ_HIP_ATTN_CHUNK_W8_H_
#define LSQ_HIP_ATTN_CHUNK_W8_H_

#include "lsq_hip_attn_decode_w8.h"
#include "lsq_hip_attn_paged_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_ATTN_CHUNK_W8_ABI_VERSION 1
/* out9[0] of the plans */
#define LSQ_ATTN_CHUNK_W8_COMPOSITION 0         /* legal, not served: the caller composes the existing ops */
#define LSQ_ATTN_CHUNK_W8_CHUNK 1               /* three launches, NT S workgroups per (b, kv head) in the first two */
/* geom->causal: the third mask mode */
#define LSQ_ATTN_CHUNK_W8_CAUSAL_LENGTHS 2
#define LSQ_ATTN_CHUNK_W8_ROW_TILE 16
#define LSQ_ATTN_CHUNK_W8_MAX_TK 65536
#define LSQ_ATTN_CHUNK_W8_MAX_D 128
#define LSQ_ATTN_CHUNK_W8_MIN_PAGE 16
#define LSQ_ATTN_CHUNK_W8_THREADS 256
/* the library's own choice of the chunk (splits = 0); no upper bound on the chunk */
#define LSQ_ATTN_CHUNK_W8_MIN_CHUNK 512
#define LSQ_ATTN_CHUNK_W8_WG_PER_CU 4
#define LSQ_ATTN_CHUNK_W8_MAX_SPLITS 64
#define LSQ_ATTN_CHUNK_W8_CUS 256

/* LSQ_ATTN_CHUNK_W8_ABI_VERSION the library was built with. */
int lsq_attn_chunk_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_attn_chunk_w8_last_error(void);

/* Host only.  *bytes = the workspace the entry needs for this geometry and `splits` (B Hkv R ldw + 8 B Hkv S R D); 0 for a geometry
 * whose extents alone make it COMPOSITION (D or ps not served). */
int lsq_attn_chunk_w8_workspace(const lsq_attn_decode_w8_geom* geom, int64_t splits, int64_t* bytes);
int lsq_attn_chunk_paged_w8_workspace(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, int64_t splits, int64_t* bytes);

/* y = the context's levels of the definition above: lsq_attn_decode_split_w8's argument list.  `workspace`: `workspace_bytes` bytes
 * on the device, 16-byte aligned, at least what lsq_attn_chunk_w8_workspace reports for (geom, splits), overlapping no operand; its
 * contents before the call do not matter and are undefined after it. */
int lsq_attn_chunk_w8(const lsq_attn_decode_w8_geom* geom, const lsq_attn_decode_w8_consts* consts, const lsq_attn_w8_out* scores_out,
                      const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out, const void* table, const void* key_lengths,
                      const void* q_levels, const void* k_levels, const void* v_levels, void* y, void* workspace, int64_t workspace_bytes,
                      int64_t splits, void* stream);

/* The same on pools read through `block_table` (int32 [B, Mp] on the device): lsq_attn_paged_w8_decode's argument list; geom->Tk is
 * Mp ps and geom's k and v strides are the pools' (page, head, slot). */
int lsq_attn_chunk_paged_w8(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, const lsq_attn_decode_w8_consts* consts,
                            const lsq_attn_w8_out* scores_out, const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out,
                            const void* table, const void* key_lengths, const void* block_table, const void* q_levels, const void* k_pool,
                            const void* v_pool, void* y, void* workspace, int64_t workspace_bytes, int64_t splits, void* stream);

/* Host only, nothing is launched, runs without a GPU.  `qkv_aligned`: the bases of q, k and v (the pools) are 16-byte aligned;
 * `y_aligned`: y's is.  out9[0] = the family (LSQ_ATTN_CHUNK_W8_*); for COMPOSITION the other slots are 0;
 * out9[1] = workgroups of launches 1 and 2 each = B Hkv NT S (launch 3 has B Hkv NT); out9[2] = threads per workgroup (256);
 * out9[3] = R = G Tq; out9[4] = the row tiles NT = ceil(R / 16); out9[5] = the chunk C in keys; out9[6] = the splits S = ceil(Tk / C);
 * out9[7] = LDS bytes of launch 2 = 3840 + 160 D; out9[8] = the store kind (LSQ_ATTN_W8_STORE_*). */
int lsq_attn_chunk_w8_plan(const lsq_attn_decode_w8_geom* geom, int qkv_aligned, int y_aligned, int64_t splits, int32_t* out9);
int lsq_attn_chunk_paged_w8_plan(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, int qkv_aligned, int y_aligned,
                                 int64_t splits, int32_t* out9);

#ifdef __cplusplus
}
#endif
#endif
