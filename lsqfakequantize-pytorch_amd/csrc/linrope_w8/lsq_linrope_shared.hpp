// lsq_linrope_shared.hpp -- what the two qkv linears with the rotary embedding and the KV-cache append in their epilogue say the same
// way: csrc/linrope_w8/lsq_linrope_w8.hip (8-bit weight levels) and csrc/linrope_w4/lsq_linrope_w4.hip (packed 4- / 2-bit codes).
// The rotation's device functions, the geometry of the heads and destinations, the placement of the rows (where a row of rq, k and
// v goes, decided once per workgroup), the decoding of a work item into its two 16-row strips, and the host's checks of
// include/lsq_hip_linrope_w8.h's geometry.  The two libraries stay separate; each compiles these pieces into its own kernel.
//
// rope_dequant, rope_pair and their constants are TWIN COPIES of those in csrc/rope_w8/lsq_rope_w8.hip, a translation unit: a fix
// there belongs here too.
//
// Include after the library's own tile / check headers (fail, overlap, aligned_to, ll come from csrc/lsq_companion_abi.hpp).
#pragma once
#include "../lsq_w8_out_side.hpp"
#include "../../../include/lsq_hip_linrope_w8.h"

namespace lsq {

constexpr int kLrPlaceBytes = 16 * (4 + 4 + 3 * 8); // p, flags and three offsets of 16 rows
constexpr int kLrQ = 1, kLrK = 2, kLrV = 4;         // the write flags of a row

// ---- TWIN COPIES of csrc/rope_w8/lsq_rope_w8.hip's RopeArg, RopeQ, rope_constants, rope_dequant and rope_pair ----
struct RopeArg {            // kernel argument: the constants
    const float* s_x;
    const int32_t* zx;
    const float* scale;     // the output quantizer
    const float* shift;
    float qmin, qmax, tmin, tmax;
    int mid;                // LSQ_F32 / LSQ_BF16 / LSQ_F16
};

struct RopeQ : W8OutSide {  // the constants, read once per thread
    float s_x, zx, off;     // off: 128.0f for int8 levels, what the flipped byte carries too much; 0.0f for uint8
};

__device__ __forceinline__ RopeQ rope_constants(const RopeArg& a, uint32_t flip) {
    RopeQ q;
    w8o_constants(q, a);
    q.s_x = a.s_x[0];
    q.zx = static_cast<float>(a.zx[0]);
    q.off = flip ? 128.0f : 0.0f;
    return q;
}

// LevelsTensor.dequantize(mid) of byte I of a packet's word `w`, flipped by 0x80 per byte for int8 levels so that it holds
// level + off as an unsigned byte: float(level) = float(byte) - off exactly, then (float(level) - float(zero)) * scale, rounded to mid
template <int I>
__device__ __forceinline__ float rope_dequant(uint32_t w, const RopeQ& q) {
    const float l = __fsub_rn(static_cast<float>((w >> (8 * I)) & 0xffu), q.off);
    return w8o_round_mid(__fmul_rn(__fsub_rn(l, q.zx), q.s_x), q.mid);
}

// the pair of the contract: two rounded fp32 products and one rounded fp32 difference / sum, each rounded to mid; never an fma
__device__ __forceinline__ void rope_pair(float di, float dj, float c, float s, int mid, float& ui, float& uj) {
    const float ic = w8o_round_mid(__fmul_rn(di, c), mid), js = w8o_round_mid(__fmul_rn(dj, s), mid);
    const float jc = w8o_round_mid(__fmul_rn(dj, c), mid), is = w8o_round_mid(__fmul_rn(di, s), mid);
    ui = w8o_round_mid(__fsub_rn(ic, js), mid);
    uj = w8o_round_mid(__fadd_rn(jc, is), mid);
}
// ---- end of the twin copies ----

struct LrGeom {             // kernel argument; the host has checked that every offset fits 63 bits
    int64_t row_s[3];       // q: batch; k, v: batch (dense) or page (paged)
    int64_t tok_s[3];       // q: token; k, v: token (dense) or slot (paged)
    int64_t head_s[3];
    int T, H, Hkv, D, R, P;
    int limit;              // tokens a sequence can hold: Tmax (dense) or Mp ps (paged)
    int paged, Np, ps, bt_ld;
    int items;
    uint32_t flip;          // 0x80 for int8 qkv levels (biased by 128 before rope_dequant), 0 for uint8
};

struct LrDst {              // kernel argument: rq, k, v
    uint8_t* p[3];
};

struct LrPlace {            // the placement in LDS: kLrPlaceBytes from `off` on
    int64_t* off;           // [q, k, v][row]
    int32_t* p;             // [row]
    int32_t* flags;         // [row]
};

__device__ __forceinline__ LrPlace lr_place_at(unsigned char* base) {
    LrPlace pl;
    pl.off = reinterpret_cast<int64_t*>(base);
    pl.p = reinterpret_cast<int32_t*>(pl.off + 3 * 16);
    pl.flags = pl.p + 16;
    return pl;
}

// where row m = tid goes, by threads 0..15: p = positions[b] + t, the three write flags and the byte offsets of the row in rq, k
// and v -- dense from strides, paged from ONE block-table read.  The caller's barrier follows.
__device__ __forceinline__ void lr_place_row(const LrGeom& g, int M, const int32_t* __restrict__ pos, const int32_t* __restrict__ bt,
                                             const LrPlace& pl, int tid) {
    int flags = 0, p = 0;
    int64_t oq = 0, ok = 0, ov = 0;
    if (tid < M) {
        const int b = tid / g.T, t = tid - b * g.T;
        const int64_t pp = (pos ? static_cast<int64_t>(pos[b]) : 0) + t;
        const bool in_tables = pp >= 0 && pp < g.P;
        if (in_tables) {
            flags |= kLrQ;
            p = static_cast<int>(pp);
            oq = b * g.row_s[0] + t * g.tok_s[0];
        }
        if (pp >= 0 && pp < g.limit) {
            int64_t outer = b, tok = pp;
            bool there = true;
            if (g.paged) {
                const int e = bt[static_cast<int64_t>(b) * g.bt_ld + pp / g.ps];
                there = e >= 0 && e < g.Np;             // a wrong entry must not land in another sequence's page
                outer = e;
                tok = pp % g.ps;
            }
            if (there) {
                flags |= kLrV | (in_tables ? kLrK : 0);
                ok = outer * g.row_s[1] + tok * g.tok_s[1];
                ov = outer * g.row_s[2] + tok * g.tok_s[2];
            }
        }
    }
    pl.off[tid] = oq;
    pl.off[16 + tid] = ok;
    pl.off[32 + tid] = ov;
    pl.p[tid] = p;
    pl.flags[tid] = flags;
}

struct LrItem {             // one work item: two 16-row strips of the qkv weight; the same for the whole workgroup
    int kind;               // 0: q, 1: k, 2: v
    int hh;                 // the head among those of its kind
    bool rot;               // ROTATE (else PASS for q and k, COPY for v)
    int fA, fB;             // the strips' first features in the head
    int bit;                // the row flag that lets this item write
    int64_t nA, nB;         // the strips' first rows of the weight
};

__device__ __forceinline__ LrItem lr_item(const LrGeom& g, int item) {
    const int ipd = g.D / 32, ur = g.R / 32;            // items of a head, and those of them that rotate
    const int head = item / ipd, u = item - head * ipd;
    LrItem it;
    it.kind = head < g.H ? 0 : (head < g.H + g.Hkv ? 1 : 2);
    it.hh = head - (it.kind == 0 ? 0 : (it.kind == 1 ? g.H : g.H + g.Hkv));
    it.rot = it.kind < 2 && u < ur;
    it.fA = it.rot ? 16 * u : 32 * u;                   // (R = 32 ur: the strips beyond R start at 32 u too)
    it.fB = it.rot ? it.fA + g.R / 2 : it.fA + 16;
    it.bit = 1 << it.kind;
    it.nA = static_cast<int64_t>(head) * g.D + it.fA;
    it.nB = static_cast<int64_t>(head) * g.D + it.fB;
    return it;
}

// the item counts of a geometry the kernels serve
inline void lr_item_counts(const lsq_linrope_w8_geom& ge, int& rotate, int& pass, int& copy) {
    rotate = static_cast<int>((ge.H + ge.Hkv) * (ge.R / 32));
    pass = static_cast<int>((ge.H + ge.Hkv) * ((ge.D - ge.R) / 32));
    copy = static_cast<int>(ge.Hkv * (ge.D / 32));
}

// what both kernels ask of the geometry besides their own K: rows, the pairing, D, R and the destination strides
inline bool lr_geom_served(const lsq_linrope_w8_geom& ge) {
    const int64_t M = ge.B * ge.T;
    const bool strides = ge.q_sb % 16 == 0 && ge.q_st % 16 == 0 && ge.q_sh % 16 == 0 && ge.k_so % 16 == 0 && ge.k_st % 16 == 0 &&
                         ge.k_sh % 16 == 0 && ge.v_so % 16 == 0 && ge.v_st % 16 == 0 && ge.v_sh % 16 == 0;
    return strides && M >= 1 && M <= LSQ_LINROPE_W8_MAX_ROWS && ge.style == LSQ_ROPE_W8_HALF && ge.D % 32 == 0 && ge.R % 32 == 0 && ge.R >= 32;
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// host side: the checks of the geometry and of the destinations
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int64_t kMaxExtent = INT32_MAX / 4;       // 29 bits, as lsq_hip_rope_w8.h
constexpr int64_t kMaxOffset = int64_t{1} << 58;

// the (outer, token, head) rows of a destination must not overlap each other: rope_self_overlap of csrc/rope_w8/lsq_rope_w8.hip
bool rows_overlap(const int64_t (&strides)[3], const int64_t (&extents)[3], int64_t cols) {
    int64_t st[3] = {strides[0], strides[1], strides[2]}, ex[3] = {extents[0], extents[1], extents[2]};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (st[j] < st[i]) {
                std::swap(st[i], st[j]);
                std::swap(ex[i], ex[j]);
            }
    int64_t span = cols;
    for (int i = 0; i < 3; ++i) {
        if (ex[i] == 1) continue;
        if (st[i] < span) return true;
        span += (ex[i] - 1) * st[i];
    }
    return false;
}

struct Dest {               // one destination: its name, strides and extents (outer, token, head) and its bytes
    const char* name;
    int64_t st[3], ex[3], bytes;
};

// the geometry's checks, host only (the plan makes them too); fills the three destinations
int check_geom(const char* what, const lsq_linrope_w8_geom* g, Dest (&d)[3]) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (g->B < 1 || g->T < 1 || g->H < 1 || g->Hkv < 1 || g->D < 1)
        return fail(LSQ_EINVAL, "%s: B = %lld, T = %lld, H = %lld, Hkv = %lld, D = %lld: every extent must be at least 1", what,
                    static_cast<ll>(g->B), static_cast<ll>(g->T), static_cast<ll>(g->H), static_cast<ll>(g->Hkv), static_cast<ll>(g->D));
    if (g->B > kMaxExtent || g->T > kMaxExtent || g->H > kMaxExtent || g->Hkv > kMaxExtent || g->D > kMaxExtent ||
        (g->H + 2 * g->Hkv) * g->D > kMaxExtent)
        return fail(LSQ_EINVAL, "%s: an extent is beyond 29 bits", what);
    if (g->style != LSQ_ROPE_W8_HALF && g->style != LSQ_ROPE_W8_INTERLEAVED)
        return fail(LSQ_EINVAL, "%s: style must be LSQ_ROPE_W8_HALF (0) or LSQ_ROPE_W8_INTERLEAVED (1), got %lld", what, static_cast<ll>(g->style));
    if (g->P < 1) return fail(LSQ_EINVAL, "%s: the tables hold P = %lld positions, at least 1 is needed", what, static_cast<ll>(g->P));
    if (g->P > kMaxExtent) return fail(LSQ_EINVAL, "%s: P = %lld is beyond 29 bits", what, static_cast<ll>(g->P));
    if (g->R < 2 || g->R % 2 != 0 || g->R > g->D)
        return fail(LSQ_EINVAL, "%s: the rotary dimension R = %lld must be even, at least 2 and at most D = %lld", what, static_cast<ll>(g->R),
                    static_cast<ll>(g->D));
    if (g->paged != 0 && g->paged != 1) return fail(LSQ_EINVAL, "%s: paged must be 0 or 1, got %lld", what, static_cast<ll>(g->paged));
    int64_t outer = g->B, toks = g->Tmax;
    if (g->paged) {
        const lsq_attn_paged_w8_pages& pg = g->pages;
        if (pg.Np < 1 || pg.ps < 1 || pg.Mp < 1)
            return fail(LSQ_EINVAL, "%s: Np = %lld pages of ps = %lld slots and Mp = %lld table entries: every extent must be at least 1", what,
                        static_cast<ll>(pg.Np), static_cast<ll>(pg.ps), static_cast<ll>(pg.Mp));
        if (pg.Np > kMaxExtent || pg.ps > kMaxExtent || pg.Mp > kMaxExtent || pg.Mp > kMaxExtent / pg.ps)
            return fail(LSQ_EINVAL, "%s: Np, or the Mp ps = %lld x %lld tokens of a sequence, are beyond 29 bits", what, static_cast<ll>(pg.Mp),
                        static_cast<ll>(pg.ps));
        if (pg.bt_ld < pg.Mp || pg.bt_ld > kMaxExtent)
            return fail(LSQ_EINVAL, "%s: the block table's rows are bt_ld = %lld apart, at least Mp = %lld (and at most 2^29) is needed", what,
                        static_cast<ll>(pg.bt_ld), static_cast<ll>(pg.Mp));
        outer = pg.Np;
        toks = pg.ps;
    } else if (g->Tmax < 1 || g->Tmax > kMaxExtent) {
        return fail(LSQ_EINVAL, "%s: the caches hold Tmax = %lld tokens, 1 to 2^29 are served", what, static_cast<ll>(g->Tmax));
    }
    d[0] = Dest{"rq", {g->q_sb, g->q_st, g->q_sh}, {g->B, g->T, g->H}, 0};
    d[1] = Dest{"k", {g->k_so, g->k_st, g->k_sh}, {outer, toks, g->Hkv}, 0};
    d[2] = Dest{"v", {g->v_so, g->v_st, g->v_sh}, {outer, toks, g->Hkv}, 0};
    for (Dest& t : d) {
        t.bytes = g->D;
        for (int i = 0; i < 3; ++i) {
            if (t.st[i] < 0 || t.st[i] > kMaxOffset / t.ex[i])
                return fail(LSQ_EINVAL, "%s: the strides (%lld, %lld, %lld) of %s must not be negative and must keep every offset within 2^58",
                            what, static_cast<ll>(t.st[0]), static_cast<ll>(t.st[1]), static_cast<ll>(t.st[2]), t.name);
            t.bytes += (t.ex[i] - 1) * t.st[i];
        }
        if (rows_overlap(t.st, t.ex, g->D))
            return fail(LSQ_EINVAL, "%s: under %s's strides (%lld, %lld, %lld) two rows of D = %lld bytes overlap", what, t.name,
                        static_cast<ll>(t.st[0]), static_cast<ll>(t.st[1]), static_cast<ll>(t.st[2]), static_cast<ll>(g->D));
    }
    return LSQ_OK;
}

// the rotation's sides and tables, said as csrc/rope_w8/ says them; `mid`: the projection's mid_dtype
int check_rotation(const char* what, const lsq_linrope_w8_geom* geom, int mid, const lsq_rope_w8_in* qkv, const lsq_rope_w8_out* rot,
                   const void* cos, const void* sin, const void* positions, const void* block_table, lsq::RopeArg& ra) {
    int64_t y_elem = 1;
    if (!qkv || !qkv->s_x || !qkv->zx) return fail(LSQ_EINVAL, "%s: NULL input side of the rotation, s_x or zx", what);
    if (!rot) return fail(LSQ_EINVAL, "%s: NULL output description of the rotation", what);
    if (!cos || !sin) return fail(LSQ_EINVAL, "%s: NULL cos or sin", what);
    if (!aligned_to(qkv->s_x, 4) || !aligned_to(qkv->zx, 4)) return fail(LSQ_EINVAL, "%s: the rotation's s_x and zx must be element-aligned", what);
    if (!aligned_to(cos, 4) || !aligned_to(sin, 4)) return fail(LSQ_EINVAL, "%s: cos and sin must be element-aligned", what);
    if (int rc = check_out_side(what, *rot, ra, y_elem)) return rc;
    if (!rot->out_scale) return fail(LSQ_EINVAL, "%s: NULL out_scale and out_shift: a floating rq is not served (lsq_hip_rope_w8.h)", what);
    if (rot->mid_dtype != mid) return fail(LSQ_EINVAL, "%s: the projection and the rotation must have one mid_dtype", what);
    ra.s_x = static_cast<const float*>(qkv->s_x);
    ra.zx = static_cast<const int32_t*>(qkv->zx);
    if (positions && !aligned_to(positions, 4)) return fail(LSQ_EINVAL, "%s: positions must be 4-byte aligned", what);
    if (geom->paged && (!block_table || !aligned_to(block_table, 4)))
        return fail(LSQ_EINVAL, "%s: a paged call needs a block table, 4-byte aligned", what);
    return LSQ_OK;
}

// the destinations against everything that is read, and against each other; `w_bytes`: the bytes of the weight at `w`
int check_dest_overlap(const char* what, const lsq_linrope_w8_geom* geom, const Dest (&d)[3], void* const (&dp)[3], const void* x,
                       int64_t x_bytes, const void* w, int64_t w_bytes, const void* cos, const void* sin, const void* positions,
                       const void* block_table) {
    const int64_t t_bytes = geom->P * (geom->R / 2) * 4;
    const int64_t bt_bytes = geom->paged ? ((geom->B - 1) * geom->pages.bt_ld + geom->pages.Mp) * 4 : 0;
    struct In { const char* name; const void* p; int64_t bytes; };
    const In ins[] = {{"x", x, x_bytes}, {"the weight", w, w_bytes}, {"cos", cos, t_bytes}, {"sin", sin, t_bytes},
                      {"positions", positions, 4 * geom->B}, {"the block table", block_table, bt_bytes}};
    for (int i = 0; i < 3; ++i) {
        for (const In& in : ins)
            if (in.p && in.bytes && overlap(dp[i], d[i].bytes, in.p, in.bytes))
                return fail(LSQ_EINVAL, "%s: %s's %lld bytes overlap %s", what, d[i].name, static_cast<ll>(d[i].bytes), in.name);
        for (int j = i + 1; j < 3; ++j)
            if (overlap(dp[i], d[i].bytes, dp[j], d[j].bytes))
                return fail(LSQ_EINVAL, "%s: %s's %lld bytes overlap %s's %lld", what, d[i].name, static_cast<ll>(d[i].bytes), d[j].name,
                            static_cast<ll>(d[j].bytes));
    }
    return LSQ_OK;
}

// the geometry's part of what the kernels serve, in the order the messages are given: the rows, (the caller's K,) then the
// pairing, D, R and the strides; `other`: what serves the rest
int check_rows_served(const char* what, const lsq_linrope_w8_geom& g, const char* other) {
    if (g.B * g.T > LSQ_LINROPE_W8_MAX_ROWS)
        return fail(LSQ_EINVAL, "%s: B T = %lld rows of x, the kernel serves 1 to %d (%s)", what, static_cast<ll>(g.B * g.T),
                    LSQ_LINROPE_W8_MAX_ROWS, other);
    return LSQ_OK;
}

int check_geom_served(const char* what, const lsq_linrope_w8_geom& g, const Dest (&d)[3], const char* other) {
    if (g.style != LSQ_ROPE_W8_HALF) return fail(LSQ_EINVAL, "%s: the interleaved pairing is not served (%s)", what, other);
    if (g.D % 32 != 0 || g.R % 32 != 0)
        return fail(LSQ_EINVAL, "%s: D = %lld and R = %lld, the kernel serves multiples of 32 (%s)", what, static_cast<ll>(g.D),
                    static_cast<ll>(g.R), other);
    for (const Dest& t : d)
        if (t.st[0] % 16 || t.st[1] % 16 || t.st[2] % 16)
            return fail(LSQ_EINVAL, "%s: the strides (%lld, %lld, %lld) of %s must be multiples of 16 bytes (%s)", what, static_cast<ll>(t.st[0]),
                        static_cast<ll>(t.st[1]), static_cast<ll>(t.st[2]), t.name, other);
    return LSQ_OK;
}

// the kernel's geometry from the header's
lsq::LrGeom kernel_geom(const lsq_linrope_w8_geom* geom, const Dest (&d)[3], int items, bool qkv_signed) {
    lsq::LrGeom g{};
    for (int i = 0; i < 3; ++i) {
        g.row_s[i] = d[i].st[0];
        g.tok_s[i] = d[i].st[1];
        g.head_s[i] = d[i].st[2];
    }
    g.T = static_cast<int>(geom->T);
    g.H = static_cast<int>(geom->H);
    g.Hkv = static_cast<int>(geom->Hkv);
    g.D = static_cast<int>(geom->D);
    g.R = static_cast<int>(geom->R);
    g.P = static_cast<int>(geom->P);
    g.limit = static_cast<int>(geom->paged ? geom->pages.Mp * geom->pages.ps : geom->Tmax);
    g.paged = static_cast<int>(geom->paged);
    g.Np = geom->paged ? static_cast<int>(geom->pages.Np) : 0;
    g.ps = geom->paged ? static_cast<int>(geom->pages.ps) : 1;
    g.bt_ld = geom->paged ? static_cast<int>(geom->pages.bt_ld) : 0;
    g.items = items;
    g.flip = qkv_signed ? 0x80u : 0u;
    return g;
}

}  // namespace
