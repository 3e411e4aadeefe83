// lsq_attn_paged_w8.hip -- a paged KV cache on 8-bit levels on gfx950 (include/lsq_hip_attn_paged_w8.h, which states the contract):
// liblsq_hip_attn_paged_w8.so.
//
// The decode is the split library's: the three launches, their constants, the chunk rule, the plan and the launch sequence are
// ../attn_decode_split_w8/lsq_attn_split_core.hpp, and the geometry, constants, sides and key_lengths are checked by
// ../attn_w8/lsq_attn_decode_checks.hpp; the PagedKeys policy -- a key's row lies in the page the block table names, READS CLAMP --
// and the checks of the pages are lsq_attn_paged_keys.hpp, which the chunk library reads too.  What is left here: the kernels as the
// core's bodies on that policy, the plan with this library's workspace row stride and page rule, the checks of the buffers, the C
// ABI, and the append:
//
// kv_append_paged: one lane per 16-byte packet (or per byte) of k and of v; a token whose position or entry is out of range is
// skipped as a whole.
#include "../lsq_companion_abi.hpp"
#include "../attn_w8/lsq_attn_decode_checks.hpp"
#include "../attn_decode_split_w8/lsq_attn_split_core.hpp"
#include "lsq_attn_paged_keys.hpp"

namespace lsq {

// the core is written on the split header's constants
static_assert(LSQ_ATTN_PAGED_W8_MAX_ROWS == LSQ_ATTN_DECODE_SPLIT_W8_MAX_ROWS && LSQ_ATTN_PAGED_W8_MAX_D == LSQ_ATTN_DECODE_SPLIT_W8_MAX_D &&
                  LSQ_ATTN_PAGED_W8_MAX_TK == LSQ_ATTN_DECODE_SPLIT_W8_MAX_TK && LSQ_ATTN_PAGED_W8_THREADS == LSQ_ATTN_DECODE_SPLIT_W8_THREADS &&
                  LSQ_ATTN_PAGED_W8_MIN_CHUNK == LSQ_ATTN_DECODE_SPLIT_W8_MIN_CHUNK &&
                  LSQ_ATTN_PAGED_W8_MAX_CHUNK == LSQ_ATTN_DECODE_SPLIT_W8_MAX_CHUNK &&
                  LSQ_ATTN_PAGED_W8_WG_PER_CU == LSQ_ATTN_DECODE_SPLIT_W8_WG_PER_CU &&
                  LSQ_ATTN_PAGED_W8_MAX_SPLITS == LSQ_ATTN_DECODE_SPLIT_W8_MAX_SPLITS && LSQ_ATTN_PAGED_W8_CUS == LSQ_ATTN_DECODE_SPLIT_W8_CUS,
              "the paged header's constants are the split header's");

__global__ __launch_bounds__(kSplThreads) void attn_paged_scores_kernel(SplGeom g, SplArg a, AttnOut so, const int32_t* __restrict__ lens,
                                                                        const uint8_t* __restrict__ Q, const uint8_t* __restrict__ K,
                                                                        uint8_t* __restrict__ ws, PagedKeys keys) {
    attn_split_scores(g, a, so, lens, Q, K, ws, keys);
}

__global__ __launch_bounds__(kSplThreads) void attn_paged_context_kernel(SplGeom g, SplArg a, AttnOut po, const int32_t* __restrict__ table,
                                                                         const int32_t* __restrict__ lens, const uint8_t* __restrict__ V,
                                                                         const uint8_t* __restrict__ ws, int64_t* __restrict__ wi,
                                                                         PagedKeys keys) {
    attn_split_context(g, a, po, table, lens, V, ws, wi, keys);
}

__global__ __launch_bounds__(kSplThreads) void attn_paged_reduce_kernel(SplGeom g, SplArg a, AttnOut co, const int32_t* __restrict__ lens,
                                                                        const int64_t* __restrict__ wi, uint8_t* __restrict__ y) {
    attn_split_reduce(g, a, co, lens, wi, y);
}

// ------------------------------------------------------------------------------------------------ the append
struct ApGeom {             // kernel argument
    int64_t k_sb, k_st, k_sh, v_sb, v_st, v_sh, kp_sp, kp_sh, kp_ss, vp_sp, vp_sh, vp_ss;
    int64_t bt_ld;
    int64_t per;            // work units of one of k and v: B T Hkv units
    int64_t cap;            // Mp ps
    int T, Hkv, units, Np, ps;
};

// one lane per unit (a 16-byte packet, or a byte) of k and then of v; WRITES SKIP: a token outside the table's capacity or whose
// entry lies outside [0, Np) changes no byte
template <bool kPackets>
__global__ __launch_bounds__(kSplThreads) void kv_append_paged_kernel(ApGeom g, const int32_t* __restrict__ bt, const int32_t* __restrict__ pos,
                                                                     const uint8_t* __restrict__ k, const uint8_t* __restrict__ v,
                                                                     uint8_t* __restrict__ kp, uint8_t* __restrict__ vp) {
    int64_t i = static_cast<int64_t>(blockIdx.x) * kSplThreads + threadIdx.x;
    if (i >= 2 * g.per) return;
    const bool second = i >= g.per;
    if (second) i -= g.per;
    const int u = static_cast<int>(i % g.units);
    i /= g.units;
    const int h = static_cast<int>(i % g.Hkv);
    i /= g.Hkv;
    const int t = static_cast<int>(i % g.T);
    const int64_t b = i / g.T;
    const int64_t p = (pos ? static_cast<int64_t>(pos[b]) : 0) + t;
    if (p < 0 || p >= g.cap) return;
    const int64_t lp = p / g.ps;                                        // < Mp
    const int e = bt[b * g.bt_ld + lp];
    if (e < 0 || e >= g.Np) return;
    const int64_t slot = p - lp * g.ps;
    const int64_t o = (kPackets ? 16 : 1) * static_cast<int64_t>(u);
    const uint8_t* __restrict__ src = second ? v + b * g.v_sb + t * g.v_st + h * g.v_sh + o : k + b * g.k_sb + t * g.k_st + h * g.k_sh + o;
    uint8_t* __restrict__ dst = second ? vp + e * g.vp_sp + h * g.vp_sh + slot * g.vp_ss + o : kp + e * g.kp_sp + h * g.kp_sh + slot * g.kp_ss + o;
    if (kPackets) {
        *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
    } else {
        *dst = *src;
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plans
// ------------------------------------------------------------------------------------------------
// the workspace's score rows are Tk = Mp ps bytes apart (a multiple of 16); ps a power of two >= 16 (Mp ps <= 65536: the API's own limit)
inline SplPlan plan_paged(const lsq_attn_decode_w8_geom& ge, const lsq_attn_paged_w8_pages& pg, bool qkv_aligned, bool y_aligned, int64_t splits) {
    return plan_split_core(ge, qkv_aligned && paged_page_served(pg), y_aligned, splits, ge.Tk);
}

inline int paged_family(const SplPlan& pl) { return pl.served ? LSQ_ATTN_PAGED_W8_PAGED : LSQ_ATTN_PAGED_W8_COMPOSITION; }

struct ApPlan {
    int family, units;
    int64_t grid;
    ApGeom g;
};

inline ApPlan plan_append(const lsq_kv_append_paged_w8_geom& ge, bool aligned) {
    ApPlan pl = {};
    const int64_t st[12] = {ge.k_sb, ge.k_st, ge.k_sh, ge.v_sb, ge.v_st, ge.v_sh, ge.kp_sp, ge.kp_sh, ge.kp_ss, ge.vp_sp, ge.vp_sh, ge.vp_ss};
    bool packets = aligned && ge.D % 16 == 0;
    for (int64_t s : st) packets = packets && s % 16 == 0;
    pl.family = packets ? LSQ_ATTN_PAGED_W8_APPEND_PACKETS : LSQ_ATTN_PAGED_W8_APPEND_GENERIC;
    pl.units = static_cast<int>(packets ? ge.D / 16 : ge.D);
    const int64_t per = ge.B * ge.T * ge.Hkv * pl.units;                // at most 2^40: check_append_geom
    pl.grid = (2 * per + kSplThreads - 1) / kSplThreads;
    pl.g = ApGeom{ge.k_sb, ge.k_st, ge.k_sh, ge.v_sb, ge.v_st, ge.v_sh, ge.kp_sp, ge.kp_sh, ge.kp_ss, ge.vp_sp, ge.vp_sh, ge.vp_ss,
                  ge.pages.bt_ld, per, ge.pages.Mp * ge.pages.ps, static_cast<int>(ge.T), static_cast<int>(ge.Hkv), pl.units,
                  static_cast<int>(ge.pages.Np), static_cast<int>(ge.pages.ps)};
    return pl;
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_attn_paged_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

int check_append_geom(const char* what, const lsq_kv_append_paged_w8_geom* g) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (int rc = check_pages(what, &g->pages)) return rc;
    const int64_t lim = int64_t{1} << 29;
    if (g->B < 1 || g->T < 1 || g->Hkv < 1 || g->D < 1 || g->B > lim || g->T > lim || g->Hkv > lim || g->D > lim || g->pages.ps > lim ||
        g->pages.Mp > lim)
        return fail(LSQ_EINVAL, "%s: [B, T, Hkv, D] = [%lld, %lld, %lld, %lld] with ps = %lld and Mp = %lld, every extent must be 1 .. 2^29", what,
                    static_cast<ll>(g->B), static_cast<ll>(g->T), static_cast<ll>(g->Hkv), static_cast<ll>(g->D), static_cast<ll>(g->pages.ps),
                    static_cast<ll>(g->pages.Mp));
    int64_t elems = g->B;                                               // B T Hkv D without overflow: each factor is 2^29 at most
    for (int64_t n : {g->T, g->Hkv, g->D}) {
        if (elems > (int64_t{1} << 40) / n)
            return fail(LSQ_EINVAL, "%s: [B, T, Hkv, D] = [%lld, %lld, %lld, %lld] are more than 2^40 elements", what, static_cast<ll>(g->B),
                        static_cast<ll>(g->T), static_cast<ll>(g->Hkv), static_cast<ll>(g->D));
        elems *= n;
    }
    const int64_t st[12] = {g->k_sb, g->k_st, g->k_sh, g->v_sb, g->v_st, g->v_sh, g->kp_sp, g->kp_sh, g->kp_ss, g->vp_sp, g->vp_sh, g->vp_ss};
    for (int64_t s : st)
        if (s < 0 || s > (int64_t{1} << 40)) return fail(LSQ_EINVAL, "%s: a stride of %lld is negative or beyond 2^40", what, static_cast<ll>(s));
    if ((g->T > 1 && g->k_st < g->D) || (g->T > 1 && g->v_st < g->D) || (g->Hkv > 1 && (g->k_sh < g->D || g->v_sh < g->D)))
        return fail(LSQ_EINVAL, "%s: a source's token or head stride is smaller than its row of %lld", what, static_cast<ll>(g->D));
    if (g->kp_ss < g->D || g->vp_ss < g->D)
        return fail(LSQ_EINVAL, "%s: a pool's slot stride (%lld, %lld) is smaller than its row of %lld", what, static_cast<ll>(g->kp_ss),
                    static_cast<ll>(g->vp_ss), static_cast<ll>(g->D));
    const lsq_attn_w8_strides kp{g->kp_sp, g->kp_sh, g->kp_ss}, vp{g->vp_sp, g->vp_sh, g->vp_ss};
    if (self_overlap(kp, g->pages.Np, g->Hkv, g->pages.ps, g->D) || self_overlap(vp, g->pages.Np, g->Hkv, g->pages.ps, g->D))
        return fail(LSQ_EINVAL, "%s: pages, heads or slots of a pool overlap each other (k strides %lld, %lld, %lld; v strides %lld, %lld, "
                    "%lld for [%lld, %lld, %lld, %lld])", what, static_cast<ll>(g->kp_sp), static_cast<ll>(g->kp_sh), static_cast<ll>(g->kp_ss),
                    static_cast<ll>(g->vp_sp), static_cast<ll>(g->vp_sh), static_cast<ll>(g->vp_ss), static_cast<ll>(g->pages.Np),
                    static_cast<ll>(g->Hkv), static_cast<ll>(g->pages.ps), static_cast<ll>(g->D));
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_attn_paged_w8_abi_version(void) { return LSQ_ATTN_PAGED_W8_ABI_VERSION; }

const char* lsq_attn_paged_w8_last_error(void) { return g_last_error; }

int lsq_attn_paged_w8_workspace(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, int64_t splits, int64_t* bytes) {
    const char* what = "lsq_attn_paged_w8_workspace";
    if (int rc = check_paged_geom(what, geom, pages)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (!bytes) return fail(LSQ_EINVAL, "%s: NULL bytes", what);
    lsq_attn_decode_w8_geom dense = *geom;                              // the size does not depend on bases or strides
    dense.q = dense.k = dense.v = lsq_attn_w8_strides{0, 0, 16 * ((geom->D + 15) / 16)};
    const lsq::SplPlan pl = lsq::plan_paged(dense, *pages, true, true, splits);
    if (int rc = check_grid(what, pl.grid)) return rc;
    *bytes = pl.ws_bytes;                                               // 0 where the plan is the composition
    return LSQ_OK;
}

int lsq_attn_paged_w8_decode(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, const lsq_attn_decode_w8_consts* consts,
                             const lsq_attn_w8_out* scores_out, const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out,
                             const void* table, const void* key_lengths, const void* block_table, const void* q_levels, const void* k_pool,
                             const void* v_pool, void* y, void* workspace, int64_t workspace_bytes, int64_t splits, void* stream) {
    const char* what = "lsq_attn_paged_w8_decode";
    lsq::AttnOut so{}, po{}, co{};
    if (int rc = check_paged_geom(what, geom, pages)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (int rc = check_decode_consts(what, consts)) return rc;
    if (int rc = check_decode_sides(what, scores_out, probs_out, ctx_out, so, po, co)) return rc;
    if (!table || !q_levels || !k_pool || !v_pool || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(table, 4)) return fail(LSQ_EINVAL, "%s: the table must be element-aligned", what);
    if (!block_table) return fail(LSQ_EINVAL, "%s: NULL block table", what);
    if (!aligned_to(block_table, 4)) return fail(LSQ_EINVAL, "%s: the block table must be 4-byte aligned", what);
    if (int rc = check_key_lengths(what, geom, key_lengths)) return rc;
    const int64_t q_span = span_of(geom->q, geom->B, geom->H, geom->Tq, geom->D), y_bytes = span_of(geom->y, geom->B, geom->H, geom->Tq, geom->D);
    const int64_t k_span = span_of(geom->k, pages->Np, geom->Hkv, pages->ps, geom->D), v_span = span_of(geom->v, pages->Np, geom->Hkv, pages->ps, geom->D);
    const int64_t bt_bytes = 4 * ((geom->B - 1) * pages->bt_ld + pages->Mp);
    if (overlap(y, y_bytes, q_levels, q_span) || overlap(y, y_bytes, k_pool, k_span) || overlap(y, y_bytes, v_pool, v_span) ||
        overlap(y, y_bytes, table, 1024) || overlap(y, y_bytes, block_table, bt_bytes) ||
        (key_lengths && overlap(y, y_bytes, key_lengths, 4 * geom->B)))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap q's %lld, the k pool's %lld, the v pool's %lld, the table, the block table or "
                    "key_lengths", what, static_cast<ll>(y_bytes), static_cast<ll>(q_span), static_cast<ll>(k_span), static_cast<ll>(v_span));
    const lsq::SplPlan pl = lsq::plan_paged(*geom, *pages, aligned_to(q_levels, 16) && aligned_to(k_pool, 16) && aligned_to(v_pool, 16),
                                           aligned_to(y, 16), splits);
    if (!pl.served)
        return fail(LSQ_EINVAL, "%s: [B, H, Hkv, Tq, D] = [%lld, %lld, %lld, %lld, %lld] on pages of %lld slots with these bases and strides is "
                    "not served by the paged kernels (G Tq <= %d, q and the pools 16-byte aligned with strides that are multiples of 16, "
                    "D %% 16 == 0, 16 <= D <= %d, ps a power of two >= %d): gather the pages and compose lsq_hip_attn_w8.h and "
                    "lsq_hip_attn_mask_w8.h", what, static_cast<ll>(geom->B), static_cast<ll>(geom->H), static_cast<ll>(geom->Hkv),
                    static_cast<ll>(geom->Tq), static_cast<ll>(geom->D), static_cast<ll>(pages->ps), LSQ_ATTN_PAGED_W8_MAX_ROWS,
                    LSQ_ATTN_PAGED_W8_MAX_D, LSQ_ATTN_PAGED_W8_MIN_PAGE);
    if (int rc = check_grid(what, pl.grid)) return rc;
    if (!workspace) return fail(LSQ_EINVAL, "%s: NULL workspace (%lld bytes are needed: lsq_attn_paged_w8_workspace)", what, static_cast<ll>(pl.ws_bytes));
    if (!aligned_to(workspace, 16)) return fail(LSQ_EINVAL, "%s: the workspace must be 16-byte aligned", what);
    if (workspace_bytes < pl.ws_bytes)
        return fail(LSQ_EINVAL, "%s: the workspace has %lld bytes, %lld are needed (lsq_attn_paged_w8_workspace)", what,
                    static_cast<ll>(workspace_bytes), static_cast<ll>(pl.ws_bytes));
    if (overlap(workspace, pl.ws_bytes, q_levels, q_span) || overlap(workspace, pl.ws_bytes, k_pool, k_span) ||
        overlap(workspace, pl.ws_bytes, v_pool, v_span) || overlap(workspace, pl.ws_bytes, y, y_bytes) ||
        overlap(workspace, pl.ws_bytes, table, 1024) || overlap(workspace, pl.ws_bytes, block_table, bt_bytes) ||
        (key_lengths && overlap(workspace, pl.ws_bytes, key_lengths, 4 * geom->B)))
        return fail(LSQ_EINVAL, "%s: the workspace's %lld bytes overlap q, a pool, y, the table, the block table or key_lengths", what,
                    static_cast<ll>(pl.ws_bytes));
    if (overlap(block_table, bt_bytes, k_pool, k_span) || overlap(block_table, bt_bytes, v_pool, v_span))
        return fail(LSQ_EINVAL, "%s: the block table's %lld bytes overlap a pool", what, static_cast<ll>(bt_bytes));
    return split_launch<lsq::attn_paged_scores_kernel, lsq::attn_paged_context_kernel, lsq::attn_paged_reduce_kernel>(
        what, pl, geom, consts, scores_out, probs_out, so, po, co, table, key_lengths, q_levels, k_pool, v_pool, y, workspace, stream,
        lsq::paged_keys(*pages, block_table));
}

int lsq_attn_paged_w8_plan(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, int qkv_aligned, int y_aligned,
                           int64_t splits, int32_t* out8) {
    const char* what = "lsq_attn_paged_w8_plan";
    if (int rc = check_paged_geom(what, geom, pages)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::SplPlan pl = lsq::plan_paged(*geom, *pages, qkv_aligned != 0, y_aligned != 0, splits);
    if (int rc = check_grid(what, pl.grid)) return rc;
    lsq::split_plan_out(pl, lsq::paged_family(pl), out8);
    return LSQ_OK;
}

int lsq_kv_append_paged_w8(const lsq_kv_append_paged_w8_geom* geom, const void* block_table, const void* positions, const void* k_levels,
                           const void* v_levels, void* k_pool, void* v_pool, void* stream) {
    const char* what = "lsq_kv_append_paged_w8";
    if (int rc = check_append_geom(what, geom)) return rc;
    if (!k_levels || !v_levels || !k_pool || !v_pool) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!block_table) return fail(LSQ_EINVAL, "%s: NULL block table", what);
    if (!aligned_to(block_table, 4)) return fail(LSQ_EINVAL, "%s: the block table must be 4-byte aligned", what);
    if (positions && !aligned_to(positions, 4)) return fail(LSQ_EINVAL, "%s: positions must be 4-byte aligned", what);
    const lsq_attn_w8_strides ks{geom->k_sb, geom->k_st, geom->k_sh}, vs{geom->v_sb, geom->v_st, geom->v_sh};
    const lsq_attn_w8_strides kp{geom->kp_sp, geom->kp_sh, geom->kp_ss}, vp{geom->vp_sp, geom->vp_sh, geom->vp_ss};
    const int64_t k_span = span_of(ks, geom->B, geom->T, geom->Hkv, geom->D), v_span = span_of(vs, geom->B, geom->T, geom->Hkv, geom->D);
    const int64_t kp_span = span_of(kp, geom->pages.Np, geom->Hkv, geom->pages.ps, geom->D);
    const int64_t vp_span = span_of(vp, geom->pages.Np, geom->Hkv, geom->pages.ps, geom->D);
    const int64_t bt_bytes = 4 * ((geom->B - 1) * geom->pages.bt_ld + geom->pages.Mp);
    const void* pools[2] = {k_pool, v_pool};
    const int64_t spans[2] = {kp_span, vp_span};
    for (int i = 0; i < 2; ++i)
        if (overlap(pools[i], spans[i], k_levels, k_span) || overlap(pools[i], spans[i], v_levels, v_span) ||
            overlap(pools[i], spans[i], block_table, bt_bytes) || (positions && overlap(pools[i], spans[i], positions, 4 * geom->B)))
            return fail(LSQ_EINVAL, "%s: the %s pool's %lld bytes overlap a source, the block table or positions", what, i ? "v" : "k",
                        static_cast<ll>(spans[i]));
    if (overlap(k_pool, kp_span, v_pool, vp_span)) return fail(LSQ_EINVAL, "%s: the two pools overlap each other", what);
    const lsq::ApPlan pl = lsq::plan_append(*geom, aligned_to(k_levels, 16) && aligned_to(v_levels, 16) && aligned_to(k_pool, 16) && aligned_to(v_pool, 16));
    if (int rc = check_grid(what, pl.grid)) return rc;
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kSplThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int32_t* bt = static_cast<const int32_t*>(block_table);
    const int32_t* pos = static_cast<const int32_t*>(positions);
    const uint8_t* k = static_cast<const uint8_t*>(k_levels);
    const uint8_t* v = static_cast<const uint8_t*>(v_levels);
    if (pl.family == LSQ_ATTN_PAGED_W8_APPEND_PACKETS)
        hipLaunchKernelGGL(lsq::kv_append_paged_kernel<true>, grid, block, 0, st, pl.g, bt, pos, k, v, static_cast<uint8_t*>(k_pool), static_cast<uint8_t*>(v_pool));
    else
        hipLaunchKernelGGL(lsq::kv_append_paged_kernel<false>, grid, block, 0, st, pl.g, bt, pos, k, v, static_cast<uint8_t*>(k_pool), static_cast<uint8_t*>(v_pool));
    return hip_status(hipGetLastError(), what);
}

int lsq_kv_append_paged_w8_plan(const lsq_kv_append_paged_w8_geom* geom, int aligned, int32_t* out8) {
    const char* what = "lsq_kv_append_paged_w8_plan";
    if (int rc = check_append_geom(what, geom)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::ApPlan pl = lsq::plan_append(*geom, aligned != 0);
    if (int rc = check_grid(what, pl.grid)) return rc;
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = lsq::kSplThreads;
    out8[3] = pl.units;
    out8[4] = out8[5] = out8[6] = 0;
    out8[7] = pl.family;
    return LSQ_OK;
}

}  // extern "C"
