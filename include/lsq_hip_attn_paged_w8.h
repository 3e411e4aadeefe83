/* include/lsq_hip_attn_paged_w8.h -- a PAGED KV cache on 8-bit LEVELS on gfx950: the append that writes a step's k and v into pages of
 * one pool, and the split-key decode attention of lsq_hip_attn_decode_split_w8.h reading that pool through a block table -- no dense
 * [B, Hkv, Tmax, D] copy of a sequence's pages is ever made.
 *
 * Exported by `liblsq_hip_attn_paged_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/attn_paged_w8/ for gfx950), the twenty-third
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the structs
 * `lsq_attn_decode_w8_geom` and `lsq_attn_decode_w8_consts` of lsq_hip_attn_decode_w8.h and `lsq_attn_w8_out` of lsq_hip_attn_w8.h,
 * and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device buffers -- the WORKSPACE
 * included --, the kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no
 * synchronisation, no atomics, no environment variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws,
 * everything is validated before anything is enqueued; lsq_attn_paged_w8_last_error() describes the calling thread's last
 * failure.  Launches repeat bit for bit, and the result never depends on what the workspace held before the call.
 *
 * THE PAGED LAYOUT.  `k_pool` and `v_pool` hold levels (uint8 or int8 each), logically [Np, Hkv, ps, D]: Np pages of ps slots for
 * each of the Hkv kv heads, addressed through THREE strides in elements -- page, head, slot -- with the innermost stride 1.  Both
 * storage orders [Np, Hkv, ps, D] and [Np, ps, Hkv, D] are views of that.  Each pool has one (scale, zero point) on the device.
 * `block_table` is int32 [B, Mp] on the device, 4-byte aligned, its rows `bt_ld` >= Mp elements apart; it is read in the kernels
 * and never on the host.  The logical capacity of a sequence is Tk = Mp ps <= 65536 keys, and key j of batch entry b lies in
 *     page e = clamp(block_table[b, j / ps], 0, Np - 1)   at slot j % ps.
 * READS CLAMP: device values cannot be refused on the host, and a wrong entry must never become an access outside the pool.
 * WRITES SKIP (the append, below): a wrong entry must not land in another sequence's page.
 *
 * THE DEFINITION OF THE DECODE.  K[b, hkv, j, :] = k_pool[clamp(block_table[b, j / ps]), hkv, j % ps, :] for j < Tk, V likewise; y is
 * lsq_attn_decode_w8's result on (q, K, V): q [B, H, Tq, D], the same table, sides, mid_dtype, `causal` and `key_lengths`, and
 *     n(b, t) = min(Tk,  t + 1 + causal_offset  where causal,  max(key_lengths[b], 0)  where given)
 * with this Tk.  With nmax(b) = n(b, Tq - 1): table entries at logical pages >= ceil(nmax(b) / ps) are NEVER READ, and pool bytes
 * at keys >= nmax(b) are NEVER READ.  Every intermediate of the definition is a byte or an exact integer, so paging changes no
 * bit: the bytes are the decode kernel's, the split kernels' and the CPU path's.
 *
 * THE DECODE'S GEOMETRY is a `lsq_attn_decode_w8_geom` whose Tk is Mp ps and whose k and v strides describe the POOLS:
 * s0 = the page stride, s1 = the head stride, ld = the slot stride; plus a `lsq_attn_paged_w8_pages` {Np, ps, Mp, bt_ld}.
 *
 * THREE LAUNCHES, those of lsq_hip_attn_decode_split_w8.h with the same chunk rule (C a multiple of 64 keys, S = ceil(Tk / C);
 * `splits` = 0: the library's choice with the constants below, s >= 1: at most s splits): workgroup (b, kv head, s) of launches 1
 * and 2 owns the keys [s C, min((s + 1) C, nmax)) and returns before its first barrier where s C >= nmax.
 *   1 SCORES   the 16 keys of a sub-tile share one table entry (ps is a multiple of 16; the clamped last key lies in the same
 *              sub-tile); a wave fetches the entries of a round's four sub-tiles BEFORE that round's k packets and the next
 *              round's entries while this round's matrix-core instructions run.
 *   2 CONTEXT  the 4 keys of a v group share one entry; v's rows are loaded one step ahead and their entries two steps ahead, issued
 *              in front of the previous step's row loads, so that no v row load waits for an entry load issued just in front of it.
 *   (the entry loads carry no branch: an index at or beyond the chunk's end is clamped to the chunk's last sub-tile or key)
 *   3 REDUCE   as in the split library.
 * No atomics.  LDS does not scale with Tk: 4352 bytes in launch 1, 3840 + 160 D in launch 2, 16 D in launch 3.
 *     workspace bytes = B Hkv R ldw  +  8 B Hkv S R D,      ldw = Mp ps
 *
 * SERVED (plan family LSQ_ATTN_PAGED_W8_PAGED): R = G Tq <= 16; D % 16 == 0 and 16 <= D <= 128; ps a power of two >= 16;
 * Mp ps <= 65536; the bases of q and of both pools 16-byte aligned and every stride of theirs a multiple of 16; for
 * lsq_attn_paged_w8_decode a workspace that is 16-byte aligned and at least the reported size.  Every other legal call (ps 8 or 24,
 * R 17, D 24, a misaligned pool) has the family LSQ_ATTN_PAGED_W8_COMPOSITION: lsq_attn_paged_w8_decode REFUSES it with LSQ_EINVAL,
 * enqueues nothing, and the caller gathers the pages and composes lsq_hip_attn_w8.h and lsq_hip_attn_mask_w8.h.
 *
 * REFUSALS OF THE DECODE (LSQ_EINVAL, a message, nothing is enqueued): those of lsq_attn_decode_split_w8, said the same way, and:
 * NULL pages; ps < 1, Mp < 1, Np < 1; Mp ps > 65536; geom->Tk != Mp ps; Np beyond 2^31 - 1; a NULL or misaligned block table;
 * bt_ld < Mp; pages (or heads, or slots) of a pool that overlap each other; a pool, the block table or the workspace overlapping
 * y or -- table and workspace -- each other or a pool.
 *
 * THE APPEND, lsq_kv_append_paged_w8: k and v in ONE launch, no arithmetic.  The sources are [B, T, Hkv, D] levels with the three
 * outer strides of lsq_hip_rope_w8.h's x (batch, token, head; innermost 1; views of a qkv buffer are read in place); `positions`
 * is int32 [B] on the device, or NULL for zeros.  Token (b, t) goes to p = positions[b] + t: page block_table[b, p / ps], slot
 * p % ps (ANY ps >= 1).  A token is NOT WRITTEN AT ALL where p < 0, where p >= Mp ps, or where its entry lies outside [0, Np).
 * TWO TOKENS OF ONE CALL THAT NAME THE SAME PHYSICAL SLOT ARE THE CALLER'S ERROR: which bytes win is undefined.  16-byte packets
 * where D % 16 == 0 and every base and stride is a multiple of 16 (LSQ_ATTN_PAGED_W8_APPEND_PACKETS), a byte path otherwise.
 * REFUSALS: a NULL geometry, source, pool or block table; an extent below 1 or beyond 2^29, more than 2^40 elements, Np beyond 2^31 - 1; a negative
 * stride; a source token or slot stride below D; bt_ld < Mp; a misaligned block table or positions; pages of a pool that overlap
 * each other; a pool overlapping a source, the table, positions or the other pool; a grid beyond 2^24 - 1 workgroups.
 */
#ifndef LSQ_HIP_ATTN_PAGED_W8_H_
#define LSQ_HIP_ATTN_PAGED_W8_H_

#include "lsq_hip_attn_decode_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_ATTN_PAGED_W8_ABI_VERSION 1
/* out8[0] of the decode's plan */
#define LSQ_ATTN_PAGED_W8_COMPOSITION 0         /* legal, not served: the caller gathers and composes the existing ops */
#define LSQ_ATTN_PAGED_W8_PAGED 1               /* three launches, S workgroups per (b, kv head) in the first two */
#define LSQ_ATTN_PAGED_W8_MAX_ROWS 16
#define LSQ_ATTN_PAGED_W8_MAX_TK 65536
#define LSQ_ATTN_PAGED_W8_MAX_D 128
#define LSQ_ATTN_PAGED_W8_MIN_PAGE 16
#define LSQ_ATTN_PAGED_W8_THREADS 256
/* the library's own choice of the chunk (splits = 0): the constants of lsq_hip_attn_decode_split_w8.h, confirmed for the paged form by
 * the chunk sweep in profiles/r31_attn_paged_w8_ab.txt */
#define LSQ_ATTN_PAGED_W8_MIN_CHUNK 256
#define LSQ_ATTN_PAGED_W8_MAX_CHUNK 2048
#define LSQ_ATTN_PAGED_W8_WG_PER_CU 4
#define LSQ_ATTN_PAGED_W8_MAX_SPLITS 64
#define LSQ_ATTN_PAGED_W8_CUS 256
/* out8[0] and out8[7] of the append's plan */
#define LSQ_ATTN_PAGED_W8_APPEND_GENERIC 0
#define LSQ_ATTN_PAGED_W8_APPEND_PACKETS 1

typedef struct lsq_attn_paged_w8_pages {
    int64_t Np;         /* pages of a pool */
    int64_t ps;         /* slots of a page */
    int64_t Mp;         /* entries of a block table row: the logical capacity is Mp ps keys */
    int64_t bt_ld;      /* elements between the rows of the block table, >= Mp */
} lsq_attn_paged_w8_pages;

typedef struct lsq_kv_append_paged_w8_geom {
    int64_t B, T, Hkv, D;
    lsq_attn_paged_w8_pages pages;
    int64_t k_sb, k_st, k_sh;       /* the strides of the k source's B, T and Hkv axes, in elements */
    int64_t v_sb, v_st, v_sh;
    int64_t kp_sp, kp_sh, kp_ss;    /* the k pool's page, head and slot strides, in elements */
    int64_t vp_sp, vp_sh, vp_ss;
} lsq_kv_append_paged_w8_geom;

/* LSQ_ATTN_PAGED_W8_ABI_VERSION the library was built with. */
int lsq_attn_paged_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_attn_paged_w8_last_error(void);

/* Host only.  *bytes = the workspace lsq_attn_paged_w8_decode needs (B Hkv R Mp ps + 8 B Hkv S R D); 0 for a geometry whose extents
 * alone make it COMPOSITION (R > 16, D or ps not served). */
int lsq_attn_paged_w8_workspace(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, int64_t splits, int64_t* bytes);

/* y = the context's levels of the definition above.  `block_table`: int32 [B, Mp] on the device; `workspace`: `workspace_bytes` bytes
 * on the device, 16-byte aligned, at least what lsq_attn_paged_w8_workspace reports, overlapping no operand; its contents before the
 * call do not matter and are undefined after it. */
int lsq_attn_paged_w8_decode(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, const lsq_attn_decode_w8_consts* consts,
                             const lsq_attn_w8_out* scores_out, const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out,
                             const void* table, const void* key_lengths, const void* block_table, const void* q_levels, const void* k_pool,
                             const void* v_pool, void* y, void* workspace, int64_t workspace_bytes, int64_t splits, void* stream);

/* Host only, nothing is launched, runs without a GPU.  `qkv_aligned`: the bases of q and of both pools are 16-byte aligned;
 * `y_aligned`: y's is.  out8[0] = the family (LSQ_ATTN_PAGED_W8_*); for COMPOSITION the other slots are 0;
 * out8[1] = workgroups of launches 1 and 2 each = B Hkv S; out8[2] = threads per workgroup (256); out8[3] = R = G Tq;
 * out8[4] = the chunk C in keys; out8[5] = the splits S = ceil(Mp ps / C); out8[6] = LDS bytes of launch 2 = 3840 + 160 D;
 * out8[7] = the store kind (LSQ_ATTN_W8_STORE_*). */
int lsq_attn_paged_w8_plan(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, int qkv_aligned, int y_aligned,
                           int64_t splits, int32_t* out8);

/* The append of the step's k and v [B, T, Hkv, D] into the pools, one launch.  `positions`: int32 [B] on the device or NULL. */
int lsq_kv_append_paged_w8(const lsq_kv_append_paged_w8_geom* geom, const void* block_table, const void* positions, const void* k_levels,
                           const void* v_levels, void* k_pool, void* v_pool, void* stream);

/* Host only.  `aligned`: the bases of both sources and both pools are 16-byte aligned.
 * out8[0] = the family (LSQ_ATTN_PAGED_W8_APPEND_*); out8[1] = workgroups; out8[2] = threads per workgroup (256);
 * out8[3] = work units per (token, head) of one of k and v (PACKETS: D / 16; GENERIC: D); out8[4 .. 6] = 0;
 * out8[7] = the kernel: 0 append generic, 1 append packets. */
int lsq_kv_append_paged_w8_plan(const lsq_kv_append_paged_w8_geom* geom, int aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
