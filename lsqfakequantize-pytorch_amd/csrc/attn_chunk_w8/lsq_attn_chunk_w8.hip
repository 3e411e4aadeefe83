// lsq_attn_chunk_w8.hip -- chunked prefill attention on 8-bit levels on gfx950 (include/lsq_hip_attn_chunk_w8.h, which states the
// contract): liblsq_hip_attn_chunk_w8.so.
//
// The three launches, their constants, the chunk rule, the plan and the launch sequence are
// ../attn_decode_split_w8/lsq_attn_split_core.hpp with kTiled = true -- the query rows of a kv head dealt to row tiles of 16, the tile a
// grid coordinate, every key loop ended at the tile's largest key count --; the geometry, constants, sides and key_lengths are
// checked by ../attn_w8/lsq_attn_decode_checks.hpp, the pages by ../attn_paged_w8/lsq_attn_paged_keys.hpp, which also holds the
// PagedKeys policy.  What is left here: the six kernels as the core's tiled bodies on DenseKeys and on PagedKeys, this library's
// split rule and mask modes, the refusals about the buffers and the C ABI.
#include "../lsq_companion_abi.hpp"
#include "../attn_w8/lsq_attn_decode_checks.hpp"
#include "../attn_decode_split_w8/lsq_attn_split_core.hpp"
#include "../attn_paged_w8/lsq_attn_paged_keys.hpp"
#include "../../../include/lsq_hip_attn_chunk_w8.h"

namespace lsq {

// the core is written on the split header's constants
static_assert(LSQ_ATTN_CHUNK_W8_ROW_TILE == LSQ_ATTN_DECODE_SPLIT_W8_MAX_ROWS && LSQ_ATTN_CHUNK_W8_MAX_D == LSQ_ATTN_DECODE_SPLIT_W8_MAX_D &&
                  LSQ_ATTN_CHUNK_W8_MAX_TK == LSQ_ATTN_DECODE_SPLIT_W8_MAX_TK && LSQ_ATTN_CHUNK_W8_THREADS == LSQ_ATTN_DECODE_SPLIT_W8_THREADS &&
                  LSQ_ATTN_CHUNK_W8_MIN_PAGE == LSQ_ATTN_PAGED_W8_MIN_PAGE && LSQ_ATTN_CHUNK_W8_MIN_CHUNK % kSplStep == 0,
              "the chunk header's limits are the split and the paged header's");

#define LSQ_CHUNK_KERNELS(name, Keys)                                                                                                          \
    __global__ __launch_bounds__(kSplThreads) void attn_chunk_##name##scores_kernel(                                                           \
        SplGeom g, SplArg a, AttnOut so, const int32_t* __restrict__ lens, const uint8_t* __restrict__ Q, const uint8_t* __restrict__ K,       \
        uint8_t* __restrict__ ws, Keys keys) {                                                                                                 \
        attn_split_scores<Keys, true>(g, a, so, lens, Q, K, ws, keys);                                                                         \
    }                                                                                                                                          \
    __global__ __launch_bounds__(kSplThreads) void attn_chunk_##name##context_kernel(                                                          \
        SplGeom g, SplArg a, AttnOut po, const int32_t* __restrict__ table, const int32_t* __restrict__ lens, const uint8_t* __restrict__ V,   \
        const uint8_t* __restrict__ ws, int64_t* __restrict__ wi, Keys keys) {                                                                 \
        attn_split_context<Keys, true>(g, a, po, table, lens, V, ws, wi, keys);                                                                \
    }
LSQ_CHUNK_KERNELS(, DenseKeys)
LSQ_CHUNK_KERNELS(paged_, PagedKeys)
#undef LSQ_CHUNK_KERNELS

// launch 3 does not read a key: one kernel for both
__global__ __launch_bounds__(kSplThreads) void attn_chunk_reduce_kernel(SplGeom g, SplArg a, AttnOut co, const int32_t* __restrict__ lens,
                                                                        const int64_t* __restrict__ wi, uint8_t* __restrict__ y) {
    attn_split_reduce<true>(g, a, co, lens, wi, y);
}

// row tiles, and this library's own choice of the chunk: no upper bound
constexpr SplRule kChunkRule = {true, static_cast<int64_t>(LSQ_ATTN_CHUNK_W8_WG_PER_CU) * LSQ_ATTN_CHUNK_W8_CUS, LSQ_ATTN_CHUNK_W8_MAX_SPLITS,
                                LSQ_ATTN_CHUNK_W8_MIN_CHUNK, 0};

// `pages` NULL: a dense cache, the workspace's score rows 16 ceil(Tk / 16) bytes apart; else pools, Tk = Mp ps apart
inline SplPlan plan_chunk(const lsq_attn_decode_w8_geom& ge, const lsq_attn_paged_w8_pages* pages, bool qkv_aligned, bool y_aligned, int64_t splits) {
    if (pages) return plan_split_core(ge, qkv_aligned && paged_page_served(*pages), y_aligned, splits, ge.Tk, kChunkRule);
    return plan_split_core(ge, qkv_aligned, y_aligned, splits, 16 * ((ge.Tk + 15) / 16), kChunkRule);
}

}  // namespace lsq

namespace {

// the geometry (with `pages`: of pools), then the mask mode: 0, 1 or 2, and what mode 2 needs
int check_chunk_geom(const char* what, const lsq_attn_decode_w8_geom* g, const lsq_attn_paged_w8_pages* pages, bool paged) {
    if (int rc = paged ? check_paged_geom(what, g, pages) : check_decode_geom(what, g)) return rc;
    if (g->causal < 0 || g->causal > LSQ_ATTN_CHUNK_W8_CAUSAL_LENGTHS)
        return fail(LSQ_EINVAL, "%s: causal = %lld must be 0 (off), 1 (t + 1 + causal_offset keys) or 2 (counted back from key_lengths)", what,
                    static_cast<ll>(g->causal));
    if (g->causal == LSQ_ATTN_CHUNK_W8_CAUSAL_LENGTHS && !g->has_lengths)
        return fail(LSQ_EINVAL, "%s: causal = 2 counts every row's keys back from key_lengths and needs them (has_lengths = 0)", what);
    if (g->causal == LSQ_ATTN_CHUNK_W8_CAUSAL_LENGTHS && g->causal_offset != 0)
        return fail(LSQ_EINVAL, "%s: causal = 2 takes no offset, causal_offset = %lld must be 0", what, static_cast<ll>(g->causal_offset));
    return LSQ_OK;
}

int chunk_workspace(const char* what, const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, bool paged, int64_t splits,
                    int64_t* bytes) {
    if (int rc = check_chunk_geom(what, geom, pages, paged)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (!bytes) return fail(LSQ_EINVAL, "%s: NULL bytes", what);
    lsq_attn_decode_w8_geom dense = *geom;                              // the size does not depend on bases or strides
    dense.q = dense.k = dense.v = lsq_attn_w8_strides{0, 0, 16 * ((geom->D + 15) / 16)};
    const lsq::SplPlan pl = lsq::plan_chunk(dense, pages, true, true, splits);
    if (int rc = check_grid(what, pl.grid)) return rc;
    *bytes = pl.ws_bytes;                                               // 0 where the plan is the composition
    return LSQ_OK;
}

int chunk_plan(const char* what, const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, bool paged, int qkv_aligned,
               int y_aligned, int64_t splits, int32_t* out9) {
    if (int rc = check_chunk_geom(what, geom, pages, paged)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (!out9) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::SplPlan pl = lsq::plan_chunk(*geom, pages, qkv_aligned != 0, y_aligned != 0, splits);
    if (int rc = check_grid(what, pl.grid)) return rc;
    out9[0] = pl.served ? LSQ_ATTN_CHUNK_W8_CHUNK : LSQ_ATTN_CHUNK_W8_COMPOSITION;      // COMPOSITION: all else 0
    out9[1] = static_cast<int32_t>(pl.grid);
    out9[2] = pl.served ? lsq::kSplThreads : 0;
    out9[3] = pl.rows;
    out9[4] = pl.tiles;
    out9[5] = pl.chunk;
    out9[6] = pl.splits;
    out9[7] = pl.lds;
    out9[8] = pl.store;
    return LSQ_OK;
}

// both entries: `pages` and `block_table` NULL for a dense cache (k, v) and given for pools
int chunk_call(const char* what, const char* ws_entry, bool paged, const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages,
               const lsq_attn_decode_w8_consts* consts, const lsq_attn_w8_out* scores_out, const lsq_attn_w8_out* probs_out,
               const lsq_attn_w8_out* ctx_out, const void* table, const void* key_lengths, const void* block_table, const void* q_levels,
               const void* k, const void* v, void* y, void* workspace, int64_t workspace_bytes, int64_t splits, void* stream) {
    lsq::AttnOut so{}, po{}, co{};
    if (int rc = check_chunk_geom(what, geom, pages, paged)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (int rc = check_decode_consts(what, consts)) return rc;
    if (int rc = check_decode_sides(what, scores_out, probs_out, ctx_out, so, po, co)) return rc;
    if (!table || !q_levels || !k || !v || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(table, 4)) return fail(LSQ_EINVAL, "%s: the table must be element-aligned", what);
    if (paged && !block_table) return fail(LSQ_EINVAL, "%s: NULL block table", what);
    if (paged && !aligned_to(block_table, 4)) return fail(LSQ_EINVAL, "%s: the block table must be 4-byte aligned", what);
    if (int rc = check_key_lengths(what, geom, key_lengths)) return rc;
    const int64_t q_span = span_of(geom->q, geom->B, geom->H, geom->Tq, geom->D), y_bytes = span_of(geom->y, geom->B, geom->H, geom->Tq, geom->D);
    const int64_t k_span = paged ? span_of(geom->k, pages->Np, geom->Hkv, pages->ps, geom->D) : span_of(geom->k, geom->B, geom->Hkv, geom->Tk, geom->D);
    const int64_t v_span = paged ? span_of(geom->v, pages->Np, geom->Hkv, pages->ps, geom->D) : span_of(geom->v, geom->B, geom->Hkv, geom->Tk, geom->D);
    const int64_t bt_bytes = paged ? 4 * ((geom->B - 1) * pages->bt_ld + pages->Mp) : 0;
    const char* kv = paged ? "the k pool's %lld, the v pool's %lld, the table, the block table or key_lengths" : "k's %lld, v's %lld, the table or key_lengths";
    if (overlap(y, y_bytes, q_levels, q_span) || overlap(y, y_bytes, k, k_span) || overlap(y, y_bytes, v, v_span) ||
        overlap(y, y_bytes, table, 1024) || (paged && overlap(y, y_bytes, block_table, bt_bytes)) ||
        (key_lengths && overlap(y, y_bytes, key_lengths, 4 * geom->B))) {
        char rest[160];
        snprintf(rest, sizeof rest, kv, static_cast<ll>(k_span), static_cast<ll>(v_span));
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap q's %lld, %s", what, static_cast<ll>(y_bytes), static_cast<ll>(q_span), rest);
    }
    const lsq::SplPlan pl = lsq::plan_chunk(*geom, pages, aligned_to(q_levels, 16) && aligned_to(k, 16) && aligned_to(v, 16), aligned_to(y, 16), splits);
    if (!pl.served)
        return fail(LSQ_EINVAL, "%s: [B, H, Hkv, Tq, Tk, D] = [%lld, %lld, %lld, %lld, %lld, %lld]%s with these bases and strides is not served "
                    "by the chunk kernels (q, k, v 16-byte aligned with strides that are multiples of 16, D %% 16 == 0, 16 <= D <= %d, "
                    "Tk <= %d, ps a power of two >= %d): %scompose lsq_hip_attn_w8.h and lsq_hip_attn_mask_w8.h", what, static_cast<ll>(geom->B),
                    static_cast<ll>(geom->H), static_cast<ll>(geom->Hkv), static_cast<ll>(geom->Tq), static_cast<ll>(geom->Tk),
                    static_cast<ll>(geom->D), paged ? " on pages" : "", LSQ_ATTN_CHUNK_W8_MAX_D, LSQ_ATTN_CHUNK_W8_MAX_TK,
                    LSQ_ATTN_CHUNK_W8_MIN_PAGE, paged ? "gather the pages and " : "");
    if (int rc = check_grid(what, pl.grid)) return rc;
    if (!workspace) return fail(LSQ_EINVAL, "%s: NULL workspace (%lld bytes are needed: %s)", what, static_cast<ll>(pl.ws_bytes), ws_entry);
    if (!aligned_to(workspace, 16)) return fail(LSQ_EINVAL, "%s: the workspace must be 16-byte aligned", what);
    if (workspace_bytes < pl.ws_bytes)
        return fail(LSQ_EINVAL, "%s: the workspace has %lld bytes, %lld are needed (%s)", what, static_cast<ll>(workspace_bytes),
                    static_cast<ll>(pl.ws_bytes), ws_entry);
    if (overlap(workspace, pl.ws_bytes, q_levels, q_span) || overlap(workspace, pl.ws_bytes, k, k_span) ||
        overlap(workspace, pl.ws_bytes, v, v_span) || overlap(workspace, pl.ws_bytes, y, y_bytes) ||
        overlap(workspace, pl.ws_bytes, table, 1024) || (paged && overlap(workspace, pl.ws_bytes, block_table, bt_bytes)) ||
        (key_lengths && overlap(workspace, pl.ws_bytes, key_lengths, 4 * geom->B)))
        return fail(LSQ_EINVAL, "%s: the workspace's %lld bytes overlap q, %s, y, the table%s or key_lengths", what, static_cast<ll>(pl.ws_bytes),
                    paged ? "a pool" : "k, v", paged ? ", the block table" : "");
    if (paged && (overlap(block_table, bt_bytes, k, k_span) || overlap(block_table, bt_bytes, v, v_span)))
        return fail(LSQ_EINVAL, "%s: the block table's %lld bytes overlap a pool", what, static_cast<ll>(bt_bytes));
    if (paged)
        return split_launch<lsq::attn_chunk_paged_scores_kernel, lsq::attn_chunk_paged_context_kernel, lsq::attn_chunk_reduce_kernel>(
            what, pl, geom, consts, scores_out, probs_out, so, po, co, table, key_lengths, q_levels, k, v, y, workspace, stream,
            lsq::paged_keys(*pages, block_table));
    return split_launch<lsq::attn_chunk_scores_kernel, lsq::attn_chunk_context_kernel, lsq::attn_chunk_reduce_kernel>(
        what, pl, geom, consts, scores_out, probs_out, so, po, co, table, key_lengths, q_levels, k, v, y, workspace, stream, lsq::DenseKeys{});
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_attn_chunk_w8.h
// ------------------------------------------------------------------------------------------------
extern "C" {

int lsq_attn_chunk_w8_abi_version(void) { return LSQ_ATTN_CHUNK_W8_ABI_VERSION; }

const char* lsq_attn_chunk_w8_last_error(void) { return g_last_error; }

int lsq_attn_chunk_w8_workspace(const lsq_attn_decode_w8_geom* geom, int64_t splits, int64_t* bytes) {
    return chunk_workspace("lsq_attn_chunk_w8_workspace", geom, nullptr, false, splits, bytes);
}

int lsq_attn_chunk_paged_w8_workspace(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, int64_t splits, int64_t* bytes) {
    return chunk_workspace("lsq_attn_chunk_paged_w8_workspace", geom, pages, true, splits, bytes);
}

int lsq_attn_chunk_w8(const lsq_attn_decode_w8_geom* geom, const lsq_attn_decode_w8_consts* consts, const lsq_attn_w8_out* scores_out,
                      const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out, const void* table, const void* key_lengths,
                      const void* q_levels, const void* k_levels, const void* v_levels, void* y, void* workspace, int64_t workspace_bytes,
                      int64_t splits, void* stream) {
    return chunk_call("lsq_attn_chunk_w8", "lsq_attn_chunk_w8_workspace", false, geom, nullptr, consts, scores_out, probs_out, ctx_out, table,
                      key_lengths, nullptr, q_levels, k_levels, v_levels, y, workspace, workspace_bytes, splits, stream);
}

int lsq_attn_chunk_paged_w8(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, const lsq_attn_decode_w8_consts* consts,
                            const lsq_attn_w8_out* scores_out, const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out,
                            const void* table, const void* key_lengths, const void* block_table, const void* q_levels, const void* k_pool,
                            const void* v_pool, void* y, void* workspace, int64_t workspace_bytes, int64_t splits, void* stream) {
    return chunk_call("lsq_attn_chunk_paged_w8", "lsq_attn_chunk_paged_w8_workspace", true, geom, pages, consts, scores_out, probs_out, ctx_out,
                      table, key_lengths, block_table, q_levels, k_pool, v_pool, y, workspace, workspace_bytes, splits, stream);
}

int lsq_attn_chunk_w8_plan(const lsq_attn_decode_w8_geom* geom, int qkv_aligned, int y_aligned, int64_t splits, int32_t* out9) {
    return chunk_plan("lsq_attn_chunk_w8_plan", geom, nullptr, false, qkv_aligned, y_aligned, splits, out9);
}

int lsq_attn_chunk_paged_w8_plan(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, int qkv_aligned, int y_aligned,
                                 int64_t splits, int32_t* out9) {
    return chunk_plan("lsq_attn_chunk_paged_w8_plan", geom, pages, true, qkv_aligned, y_aligned, splits, out9);
}

}  // extern "C"
