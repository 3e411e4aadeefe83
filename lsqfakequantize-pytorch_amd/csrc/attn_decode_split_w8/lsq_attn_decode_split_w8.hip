// lsq_attn_decode_split_w8.hip -- split-key decode attention on 8-bit levels on gfx950 (include/lsq_hip_attn_decode_split_w8.h, which
// states the contract): liblsq_hip_attn_decode_split_w8.so.
//
// The three launches, their constants, the chunk rule, the plan and the launch sequence are lsq_attn_split_core.hpp, which says what
// they do; the geometry, constants, sides and key_lengths are checked by ../attn_w8/lsq_attn_decode_checks.hpp.  What is left here:
// the kernels as that core's bodies on its DenseKeys policy (k and v are a dense cache: row(b, hkv, j) = T + b s0 + hkv s1 + j ld),
// the plan with this library's workspace row stride, the refusals about the workspace and the C ABI.
#include "../lsq_companion_abi.hpp"
#include "../attn_w8/lsq_attn_decode_checks.hpp"
#include "lsq_attn_split_core.hpp"

namespace lsq {

__global__ __launch_bounds__(kSplThreads) void attn_split_scores_kernel(SplGeom g, SplArg a, AttnOut so, const int32_t* __restrict__ lens,
                                                                        const uint8_t* __restrict__ Q, const uint8_t* __restrict__ K,
                                                                        uint8_t* __restrict__ ws, DenseKeys keys) {
    attn_split_scores(g, a, so, lens, Q, K, ws, keys);
}

__global__ __launch_bounds__(kSplThreads) void attn_split_context_kernel(SplGeom g, SplArg a, AttnOut po, const int32_t* __restrict__ table,
                                                                         const int32_t* __restrict__ lens, const uint8_t* __restrict__ V,
                                                                         const uint8_t* __restrict__ ws, int64_t* __restrict__ wi,
                                                                         DenseKeys keys) {
    attn_split_context(g, a, po, table, lens, V, ws, wi, keys);
}

__global__ __launch_bounds__(kSplThreads) void attn_split_reduce_kernel(SplGeom g, SplArg a, AttnOut co, const int32_t* __restrict__ lens,
                                                                        const int64_t* __restrict__ wi, uint8_t* __restrict__ y) {
    attn_split_reduce(g, a, co, lens, wi, y);
}

// the workspace's score rows are 16 ceil(Tk / 16) bytes apart
inline SplPlan plan_split(const lsq_attn_decode_w8_geom& ge, bool qkv_aligned, bool y_aligned, int64_t splits) {
    return plan_split_core(ge, qkv_aligned, y_aligned, splits, 16 * ((ge.Tk + 15) / 16));
}

inline int split_family(const SplPlan& pl) { return pl.served ? LSQ_ATTN_DECODE_SPLIT_W8_SPLIT : LSQ_ATTN_DECODE_SPLIT_W8_COMPOSITION; }

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_attn_decode_split_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
extern "C" {

int lsq_attn_decode_split_w8_abi_version(void) { return LSQ_ATTN_DECODE_SPLIT_W8_ABI_VERSION; }

const char* lsq_attn_decode_split_w8_last_error(void) { return g_last_error; }

int lsq_attn_decode_split_w8_workspace(const lsq_attn_decode_w8_geom* geom, int64_t splits, int64_t* bytes) {
    const char* what = "lsq_attn_decode_split_w8_workspace";
    if (int rc = check_decode_geom(what, geom)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (!bytes) return fail(LSQ_EINVAL, "%s: NULL bytes", what);
    lsq_attn_decode_w8_geom dense = *geom;                              // the size does not depend on bases or strides
    dense.q = dense.k = dense.v = lsq_attn_w8_strides{0, 0, 16 * ((geom->D + 15) / 16)};
    const lsq::SplPlan pl = lsq::plan_split(dense, true, true, splits);
    if (int rc = check_grid(what, pl.grid)) return rc;
    *bytes = pl.ws_bytes;                                               // 0 where the plan is the composition
    return LSQ_OK;
}

int lsq_attn_decode_split_w8(const lsq_attn_decode_w8_geom* geom, const lsq_attn_decode_w8_consts* consts, const lsq_attn_w8_out* scores_out,
                             const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out, const void* table, const void* key_lengths,
                             const void* q_levels, const void* k_levels, const void* v_levels, void* y, void* workspace,
                             int64_t workspace_bytes, int64_t splits, void* stream) {
    const char* what = "lsq_attn_decode_split_w8";
    lsq::AttnOut so{}, po{}, co{};
    if (int rc = check_decode_geom(what, geom)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (int rc = check_decode_consts(what, consts)) return rc;
    if (int rc = check_decode_sides(what, scores_out, probs_out, ctx_out, so, po, co)) return rc;
    if (!table || !q_levels || !k_levels || !v_levels || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(table, 4)) return fail(LSQ_EINVAL, "%s: the table must be element-aligned", what);
    if (int rc = check_key_lengths(what, geom, key_lengths)) return rc;
    const int64_t q_span = span_of(geom->q, geom->B, geom->H, geom->Tq, geom->D), k_span = span_of(geom->k, geom->B, geom->Hkv, geom->Tk, geom->D);
    const int64_t v_span = span_of(geom->v, geom->B, geom->Hkv, geom->Tk, geom->D), y_bytes = span_of(geom->y, geom->B, geom->H, geom->Tq, geom->D);
    if (overlap(y, y_bytes, q_levels, q_span) || overlap(y, y_bytes, k_levels, k_span) || overlap(y, y_bytes, v_levels, v_span) ||
        overlap(y, y_bytes, table, 1024) || (key_lengths && overlap(y, y_bytes, key_lengths, 4 * geom->B)))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap q's %lld, k's %lld, v's %lld, the table or key_lengths", what,
                    static_cast<ll>(y_bytes), static_cast<ll>(q_span), static_cast<ll>(k_span), static_cast<ll>(v_span));
    const lsq::SplPlan pl = lsq::plan_split(*geom, aligned_to(q_levels, 16) && aligned_to(k_levels, 16) && aligned_to(v_levels, 16),
                                            aligned_to(y, 16), splits);
    if (!pl.served)
        return fail(LSQ_EINVAL, "%s: [B, H, Hkv, Tq, Tk, D] = [%lld, %lld, %lld, %lld, %lld, %lld] with these bases and strides is not served "
                    "by the split kernels (G Tq <= %d, q, k, v 16-byte aligned with strides that are multiples of 16, D %% 16 == 0, "
                    "16 <= D <= %d, Tk <= %d): compose lsq_hip_attn_w8.h and lsq_hip_attn_mask_w8.h", what, static_cast<ll>(geom->B),
                    static_cast<ll>(geom->H), static_cast<ll>(geom->Hkv), static_cast<ll>(geom->Tq), static_cast<ll>(geom->Tk),
                    static_cast<ll>(geom->D), LSQ_ATTN_DECODE_SPLIT_W8_MAX_ROWS, LSQ_ATTN_DECODE_SPLIT_W8_MAX_D, LSQ_ATTN_DECODE_SPLIT_W8_MAX_TK);
    if (int rc = check_grid(what, pl.grid)) return rc;
    if (!workspace) return fail(LSQ_EINVAL, "%s: NULL workspace (%lld bytes are needed: lsq_attn_decode_split_w8_workspace)", what, static_cast<ll>(pl.ws_bytes));
    if (!aligned_to(workspace, 16)) return fail(LSQ_EINVAL, "%s: the workspace must be 16-byte aligned", what);
    if (workspace_bytes < pl.ws_bytes)
        return fail(LSQ_EINVAL, "%s: the workspace has %lld bytes, %lld are needed (lsq_attn_decode_split_w8_workspace)", what,
                    static_cast<ll>(workspace_bytes), static_cast<ll>(pl.ws_bytes));
    if (overlap(workspace, pl.ws_bytes, q_levels, q_span) || overlap(workspace, pl.ws_bytes, k_levels, k_span) ||
        overlap(workspace, pl.ws_bytes, v_levels, v_span) || overlap(workspace, pl.ws_bytes, y, y_bytes) ||
        overlap(workspace, pl.ws_bytes, table, 1024) || (key_lengths && overlap(workspace, pl.ws_bytes, key_lengths, 4 * geom->B)))
        return fail(LSQ_EINVAL, "%s: the workspace's %lld bytes overlap q, k, v, y, the table or key_lengths", what, static_cast<ll>(pl.ws_bytes));
    return split_launch<lsq::attn_split_scores_kernel, lsq::attn_split_context_kernel, lsq::attn_split_reduce_kernel>(
        what, pl, geom, consts, scores_out, probs_out, so, po, co, table, key_lengths, q_levels, k_levels, v_levels, y, workspace, stream,
        lsq::DenseKeys{});
}

int lsq_attn_decode_split_w8_plan(const lsq_attn_decode_w8_geom* geom, int qkv_aligned, int y_aligned, int64_t splits, int32_t* out8) {
    const char* what = "lsq_attn_decode_split_w8_plan";
    if (int rc = check_decode_geom(what, geom)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::SplPlan pl = lsq::plan_split(*geom, qkv_aligned != 0, y_aligned != 0, splits);
    if (int rc = check_grid(what, pl.grid)) return rc;
    lsq::split_plan_out(pl, lsq::split_family(pl), out8);
    return LSQ_OK;
}

}  // extern "C"
