// lsq_attn_decode_checks.hpp -- the host-side checks that the C ABIs on a `lsq_attn_decode_w8_geom` say the same way: liblsq_hip_attn_
// decode_w8.so, liblsq_hip_attn_prefill_w8.so, liblsq_hip_attn_decode_split_w8.so, liblsq_hip_attn_paged_w8.so, liblsq_hip_attn_chunk_w8.so
// (include/lsq_hip_attn_decode_w8.h lists the refusals).  Every refusal of a geometry, of the eight constants, of a side and of
// key_lengths has ONE text here; an entry calls the checks in the order of its header.  Host code only, in the anonymous namespace
// of the including translation unit, as lsq_attn_w8_checks.hpp, which this includes.
#pragma once
#include <algorithm>

#include "lsq_attn_w8_checks.hpp"
#include "../../../include/lsq_hip_attn_decode_w8.h"

namespace {

bool strides16(const lsq_attn_w8_strides& s) { return s.s0 % 16 == 0 && s.s1 % 16 == 0 && s.ld % 16 == 0; }

// k and v as pools of Np pages of ps slots each, read through a block table of Mp entries a row (include/lsq_hip_attn_paged_w8.h,
// whose own checks of the three come first)
struct DecodePools {
    int64_t Np, ps, Mp;
};

// the geometry of a decode, prefill or split call; with `pools`, of a paged one: Tk is the table's capacity (so only D has a limit
// of its own left), k and v are called k_pool and v_pool and must not overlap themselves
int check_decode_geom(const char* what, const lsq_attn_decode_w8_geom* g, const DecodePools* pools = nullptr) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (!level_dtype(g->q_dtype) || !level_dtype(g->k_dtype) || !level_dtype(g->v_dtype))
        return fail(LSQ_EINVAL, "%s: q_dtype, k_dtype and v_dtype must be LSQ_ATTN_W8_U8 (0) or LSQ_ATTN_W8_I8 (1), got %lld, %lld and %lld",
                    what, static_cast<ll>(g->q_dtype), static_cast<ll>(g->k_dtype), static_cast<ll>(g->v_dtype));
    if (g->B < 1 || g->H < 1 || g->Hkv < 1 || g->Tq < 1 || g->Tk < 1 || g->D < 1)
        return fail(LSQ_EINVAL, "%s: [B, H, Hkv, Tq, Tk, D] = [%lld, %lld, %lld, %lld, %lld, %lld], every extent must be at least 1", what,
                    static_cast<ll>(g->B), static_cast<ll>(g->H), static_cast<ll>(g->Hkv), static_cast<ll>(g->Tq), static_cast<ll>(g->Tk),
                    static_cast<ll>(g->D));
    if (pools && g->Tk != pools->Mp * pools->ps)
        return fail(LSQ_EINVAL, "%s: Tk = %lld is not the table's capacity Mp ps = %lld x %lld", what, static_cast<ll>(g->Tk),
                    static_cast<ll>(pools->Mp), static_cast<ll>(pools->ps));
    if (g->H % g->Hkv != 0)
        return fail(LSQ_EINVAL, "%s: H = %lld query heads are not a multiple of Hkv = %lld kv heads", what, static_cast<ll>(g->H),
                    static_cast<ll>(g->Hkv));
    if (g->causal && g->causal_offset < 0)
        return fail(LSQ_EINVAL, "%s: causal_offset = %lld must be at least 0", what, static_cast<ll>(g->causal_offset));
    if (pools && g->D > LSQ_ATTN_W8_MAX_K)
        return fail(LSQ_EINVAL, "%s: D = %lld, at most %d are served (the raw sums stay in 32 bits)", what, static_cast<ll>(g->D),
                    LSQ_ATTN_W8_MAX_K);
    if (!pools && (g->D > LSQ_ATTN_W8_MAX_K || g->Tk > LSQ_ATTN_W8_MAX_K))
        return fail(LSQ_EINVAL, "%s: D = %lld and Tk = %lld, at most %d are served (the raw sums stay in 32 bits)", what, static_cast<ll>(g->D),
                    static_cast<ll>(g->Tk), LSQ_ATTN_W8_MAX_K);
    const int64_t lim = int64_t{1} << 20;
    if (g->Tq > lim || g->B > lim || g->H > lim || g->B * g->H > lim)
        return fail(LSQ_EINVAL, "%s: Tq = %lld and B * H = %lld x %lld may each be 2^20 at most", what, static_cast<ll>(g->Tq),
                    static_cast<ll>(g->B), static_cast<ll>(g->H));
    if (int rc = check_strides(what, "q", g->q, g->D)) return rc;
    if (int rc = check_strides(what, pools ? "k_pool" : "k", g->k, g->D)) return rc;
    if (int rc = check_strides(what, pools ? "v_pool" : "v", g->v, g->D)) return rc;
    if (int rc = check_strides(what, "y", g->y, g->D)) return rc;
    if (pools && (self_overlap(g->k, pools->Np, g->Hkv, pools->ps, g->D) || self_overlap(g->v, pools->Np, g->Hkv, pools->ps, g->D)))
        return fail(LSQ_EINVAL, "%s: pages, heads or slots of a pool overlap each other (k strides %lld, %lld, %lld; v strides %lld, %lld, "
                    "%lld for [%lld, %lld, %lld, %lld])", what, static_cast<ll>(g->k.s0), static_cast<ll>(g->k.s1), static_cast<ll>(g->k.ld),
                    static_cast<ll>(g->v.s0), static_cast<ll>(g->v.s1), static_cast<ll>(g->v.ld), static_cast<ll>(pools->Np),
                    static_cast<ll>(g->Hkv), static_cast<ll>(pools->ps), static_cast<ll>(g->D));
    if (self_overlap(g->y, g->B, g->H, g->Tq, g->D))
        return fail(LSQ_EINVAL, "%s: y's rows or batches overlap each other (strides %lld, %lld, %lld for [%lld, %lld, %lld, %lld])", what,
                    static_cast<ll>(g->y.s0), static_cast<ll>(g->y.s1), static_cast<ll>(g->y.ld), static_cast<ll>(g->B),
                    static_cast<ll>(g->H), static_cast<ll>(g->Tq), static_cast<ll>(g->D));
    return LSQ_OK;
}

// the scales and zero points of q, k, v and the probabilities: eight device scalars
int check_decode_consts(const char* what, const lsq_attn_decode_w8_consts* consts) {
    if (!consts) return fail(LSQ_EINVAL, "%s: NULL constants", what);
    const void* cs[8] = {consts->s_q, consts->z_q, consts->s_k, consts->z_k, consts->s_v, consts->z_v, consts->s_p, consts->z_p};
    for (const void* c : cs) {
        if (!c) return fail(LSQ_EINVAL, "%s: NULL scale or zero point", what);
        if (!aligned_to(c, 4)) return fail(LSQ_EINVAL, "%s: the scales and zero points must be element-aligned", what);
    }
    return LSQ_OK;
}

// a side of the op is a quantizer: levels out only
int check_side(const char* what, const char* name, const lsq_attn_w8_out* c, lsq::AttnOut& arg) {
    int64_t y_elem = 1;
    if (int rc = check_out(what, c, arg, y_elem)) return rc;
    if (!c->out_scale) return fail(LSQ_EINVAL, "%s: the %s side needs out_scale and out_shift (levels out only)", what, name);
    return LSQ_OK;
}

// the scores, the probabilities and the context, which carry one mid_dtype
int check_decode_sides(const char* what, const lsq_attn_w8_out* scores_out, const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out,
                       lsq::AttnOut& so, lsq::AttnOut& po, lsq::AttnOut& co) {
    if (int rc = check_side(what, "scores", scores_out, so)) return rc;
    if (int rc = check_side(what, "probabilities", probs_out, po)) return rc;
    if (int rc = check_side(what, "context", ctx_out, co)) return rc;
    if (scores_out->mid_dtype != probs_out->mid_dtype || scores_out->mid_dtype != ctx_out->mid_dtype)
        return fail(LSQ_EINVAL, "%s: the three sides carry one mid_dtype, got codes %lld, %lld and %lld", what,
                    static_cast<ll>(scores_out->mid_dtype), static_cast<ll>(probs_out->mid_dtype), static_cast<ll>(ctx_out->mid_dtype));
    return LSQ_OK;
}

int check_key_lengths(const char* what, const lsq_attn_decode_w8_geom* geom, const void* key_lengths) {
    if (geom->has_lengths && !key_lengths) return fail(LSQ_EINVAL, "%s: key_lengths is NULL but the geometry says has_lengths", what);
    if (!geom->has_lengths && key_lengths) return fail(LSQ_EINVAL, "%s: key_lengths is given but the geometry says has_lengths = 0", what);
    if (key_lengths && !aligned_to(key_lengths, 4)) return fail(LSQ_EINVAL, "%s: key_lengths must be 4-byte aligned", what);
    return LSQ_OK;
}

// 128 where a side's levels are uint8, 0 where they are int8
int side_off(const lsq_attn_w8_out* c) { return std::max(c->quant_max, c->type_max) > 127 ? 128 : 0; }

}  // namespace
