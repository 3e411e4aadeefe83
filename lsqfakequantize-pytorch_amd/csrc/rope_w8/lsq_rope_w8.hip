// lsq_rope_w8.hip -- rotary position embedding and the KV-cache append on 8-bit levels on gfx950 (include/lsq_hip_rope_w8.h, which
// states the contract): the kernels and the C ABI of liblsq_hip_rope_w8.so.  Bandwidth kernels whose cost is their addressing.
//
//  * PACKETS, rotate (D % 16 == 0, bases and strides multiples of 16 bytes, R % 32 == 0 for the half style, R % 16 == 0 for the
//    interleaved one): a token's head is U work units.  Half style: unit j < R / 32 is the PAIR of 16-byte packets at the features
//    16 j and 16 j + R / 2 -- one lane loads both and produces both, no value crosses lanes --; interleaved: unit j < R / 16 is one
//    packet, its pairs lie inside it; a packet beyond R is a unit of its own that only dequantizes.  Item = (token, head group,
//    unit), the unit fastest: adjacent lanes sit on adjacent packets.  A lane tests its token's position once -- a skipped token
//    issues no load and no store --, loads its 16 (8) cos and sin values as 16-byte loads and walks `hpl` heads of the token with
//    them (the tables do not depend on h); all loads of a head are issued before its arithmetic, the outputs go through
//    w8o_store16.
//  * PACKETS, copy: item = (token, head, packet), a 16-byte load and store.
//  * GENERIC (every other legal call): one lane per pair, per feature beyond R, or per byte in COPY.  Correct, not tuned.
//
// rope_dequant is elt_dequant of ../eltwise_w8/lsq_eltwise_w8.hip and rope_self_overlap is self_overlap of
// ../attn_w8/lsq_attn_w8_checks.hpp, copied: this file must not depend on those libraries' sources.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../lsq_w8_out_side.hpp"
#include "../lsq_w8_out_side_host.hpp"
#include "../../../include/lsq_hip_rope_w8.h"

namespace lsq {

typedef __attribute__((ext_vector_type(4))) float rope_f32x4;

constexpr int kRopeMaxHeads = 4;                // heads a lane walks with one set of table values
constexpr int kRopeBlocksPerCU = 2;             // the grid "fills the chip" from here
constexpr int kRopeGeneric = 0, kRopeHalf = 1, kRopeInter = 2, kRopeCopyPackets = 3, kRopeCopyGeneric = 4;

struct RopeGeom {           // kernel argument; the host has checked that every offset fits 63 bits and every item 32
    int64_t x_sb, x_st, x_sh, y_sb, y_st, y_sh;
    int T, H, D, R, P, Tout;
    int U, UR;              // work units per token and head, and those of them that rotate
    int HG, hpl;            // head groups per token, heads per lane
    int scatter, interleaved;
    uint32_t flip;          // 0x80808080 for int8 levels (biased by 128 on load), 0 for uint8
    uint32_t items;
};

struct RopeArg {            // kernel argument: the constants
    const float* s_x;
    const int32_t* zx;
    const float* scale;     // the output quantizer; NULL: a floating y
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

__device__ __forceinline__ void rope_dequant16(float (&d)[16], u32x4 v, const RopeQ& q) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        d[4 * i] = rope_dequant<0>(v[i], q);
        d[4 * i + 1] = rope_dequant<1>(v[i], q);
        d[4 * i + 2] = rope_dequant<2>(v[i], q);
        d[4 * i + 3] = rope_dequant<3>(v[i], q);
    }
}

// the pair of the contract: two rounded fp32 products and one rounded fp32 difference / sum, each rounded to mid; never an fma
__device__ __forceinline__ void rope_pair(float di, float dj, float c, float s, int mid, float& ui, float& uj) {
    const float ic = w8o_round_mid(__fmul_rn(di, c), mid), js = w8o_round_mid(__fmul_rn(dj, s), mid);
    const float jc = w8o_round_mid(__fmul_rn(dj, c), mid), is = w8o_round_mid(__fmul_rn(di, s), mid);
    ui = w8o_round_mid(__fsub_rn(ic, js), mid);
    uj = w8o_round_mid(__fadd_rn(jc, is), mid);
}

// Token `tok` = b T + t: its position p and the output token it goes to; false: the token is not written.  `limit`: P, or Tout in
// COPY.  scatter = 0: t < T <= Tout, checked on the host.
__device__ __forceinline__ bool rope_place(const RopeGeom& g, const int32_t* __restrict__ pos, uint32_t tok, int limit, int& b, int& t,
                                           int& p, int& to) {
    b = static_cast<int>(tok / static_cast<uint32_t>(g.T));
    t = static_cast<int>(tok - static_cast<uint32_t>(b) * static_cast<uint32_t>(g.T));
    const int64_t pp = (pos ? static_cast<int64_t>(pos[b]) : 0) + t;
    if (pp < 0 || pp >= limit || (g.scatter && pp >= g.Tout)) return false;
    p = static_cast<int>(pp);
    to = g.scatter ? p : t;
    return true;
}

// item = (tok HG + hg) U + u
template <bool INTERLEAVED>
__global__ __launch_bounds__(kBlock) void rope_w8_packets_kernel(RopeGeom g, RopeArg a, const float* __restrict__ cos_t,
                                                                  const float* __restrict__ sin_t, const int32_t* __restrict__ pos,
                                                                  const uint8_t* __restrict__ x, void* __restrict__ y) {
    const uint32_t item = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (item >= g.items) return;
    const uint32_t r0 = item / static_cast<uint32_t>(g.U), u = item - r0 * static_cast<uint32_t>(g.U);
    const uint32_t tok = r0 / static_cast<uint32_t>(g.HG), hg = r0 - tok * static_cast<uint32_t>(g.HG);
    int b, t, p, to;
    if (!rope_place(g, pos, tok, g.P, b, t, p, to)) return;         // one predicate per token: no load, no store
    const bool rot = static_cast<int>(u) < g.UR;
    // the unit's first feature, and for the half style its partner's
    const int f0 = rot ? 16 * static_cast<int>(u) : g.R + 16 * (static_cast<int>(u) - g.UR);
    const int f1 = f0 + g.R / 2;
    constexpr int NC = INTERLEAVED ? 8 : 16;
    float c[NC], s[NC];
    if (rot) {
        const int64_t col = static_cast<int64_t>(p) * (g.R / 2) + NC * static_cast<int>(u);     // a multiple of NC: 16-byte aligned
        const rope_f32x4* __restrict__ cp = reinterpret_cast<const rope_f32x4*>(cos_t + col);
        const rope_f32x4* __restrict__ sp = reinterpret_cast<const rope_f32x4*>(sin_t + col);
#pragma unroll
        for (int i = 0; i < NC / 4; ++i) {
            const rope_f32x4 cv = cp[i], sv = sp[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c[4 * i + k] = cv[k];
                s[4 * i + k] = sv[k];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NC; ++i) c[i] = s[i] = 0.0f;
    }
    const RopeQ q = rope_constants(a, g.flip);
    const uint8_t* __restrict__ xt = x + b * g.x_sb + t * g.x_st;
    const int64_t yt = b * g.y_sb + to * g.y_st;
    const int h0 = static_cast<int>(hg) * g.hpl, h1 = min(g.H, h0 + g.hpl);
    const bool two = !INTERLEAVED && rot;
    for (int h = h0; h < h1; ++h) {
        const uint8_t* __restrict__ xh = xt + h * g.x_sh;
        u32x4 v0 = *reinterpret_cast<const u32x4*>(xh + f0), v1 = u32x4{0u, 0u, 0u, 0u};
        if (two) v1 = *reinterpret_cast<const u32x4*>(xh + f1);
        asm volatile("" : "+v"(v0), "+v"(v1));          // both in flight before the arithmetic
        const int64_t yh = yt + h * g.y_sh;
        float d0[16], o0[16];
        rope_dequant16(d0, v0 ^ g.flip, q);
        if (!rot) {
            w8o_store16(y, yh + f0, d0, q);
        } else if (INTERLEAVED) {
#pragma unroll
            for (int i = 0; i < 8; ++i) rope_pair(d0[2 * i], d0[2 * i + 1], c[i], s[i], q.mid, o0[2 * i], o0[2 * i + 1]);
            w8o_store16(y, yh + f0, o0, q);
        } else {
            float d1[16], o1[16];
            rope_dequant16(d1, v1 ^ g.flip, q);
#pragma unroll
            for (int i = 0; i < 16; ++i) rope_pair(d0[i], d1[i], c[i % NC], s[i % NC], q.mid, o0[i], o1[i]);
            w8o_store16(y, yh + f0, o0, q);
            w8o_store16(y, yh + f1, o1, q);
        }
    }
}

// one lane per pair or per feature beyond R: item = (tok H + h) U + e, U = R / 2 + D - R, UR = R / 2
__global__ __launch_bounds__(kBlock) void rope_w8_generic_kernel(RopeGeom g, RopeArg a, const float* __restrict__ cos_t,
                                                                  const float* __restrict__ sin_t, const int32_t* __restrict__ pos,
                                                                  const uint8_t* __restrict__ x, void* __restrict__ y) {
    const uint32_t item = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (item >= g.items) return;
    const uint32_t r0 = item / static_cast<uint32_t>(g.U), e = item - r0 * static_cast<uint32_t>(g.U);
    const uint32_t tok = r0 / static_cast<uint32_t>(g.H), h = r0 - tok * static_cast<uint32_t>(g.H);
    int b, t, p, to;
    if (!rope_place(g, pos, tok, g.P, b, t, p, to)) return;
    const RopeQ q = rope_constants(a, g.flip);
    const uint8_t* __restrict__ xh = x + b * g.x_sb + t * g.x_st + static_cast<int64_t>(h) * g.x_sh;
    const int64_t yh = b * g.y_sb + to * g.y_st + static_cast<int64_t>(h) * g.y_sh;
    const uint32_t flip = g.flip & 0xffu;
    if (static_cast<int>(e) >= g.UR) {
        const int f = g.R + static_cast<int>(e) - g.UR;
        w8o_store1(y, yh + f, rope_dequant<0>(static_cast<uint32_t>(xh[f]) ^ flip, q), q);
        return;
    }
    const int i = g.interleaved ? 2 * static_cast<int>(e) : static_cast<int>(e), j = g.interleaved ? i + 1 : i + g.R / 2;
    const int64_t col = static_cast<int64_t>(p) * (g.R / 2) + static_cast<int>(e);
    const float di = rope_dequant<0>(static_cast<uint32_t>(xh[i]) ^ flip, q), dj = rope_dequant<0>(static_cast<uint32_t>(xh[j]) ^ flip, q);
    float ui, uj;
    rope_pair(di, dj, cos_t[col], sin_t[col], q.mid, ui, uj);
    w8o_store1(y, yh + i, ui, q);
    w8o_store1(y, yh + j, uj, q);
}

// COPY, packets: item = (tok H + h) U + u, U = D / 16
__global__ __launch_bounds__(kBlock) void rope_w8_copy_packets_kernel(RopeGeom g, const int32_t* __restrict__ pos, const uint8_t* __restrict__ x,
                                                                       uint8_t* __restrict__ y) {
    const uint32_t item = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (item >= g.items) return;
    const uint32_t r0 = item / static_cast<uint32_t>(g.U), u = item - r0 * static_cast<uint32_t>(g.U);
    const uint32_t tok = r0 / static_cast<uint32_t>(g.H), h = r0 - tok * static_cast<uint32_t>(g.H);
    int b, t, p, to;
    if (!rope_place(g, pos, tok, g.Tout, b, t, p, to)) return;
    const u32x4 v = *reinterpret_cast<const u32x4*>(x + b * g.x_sb + t * g.x_st + static_cast<int64_t>(h) * g.x_sh + 16 * u);
    *reinterpret_cast<u32x4*>(y + b * g.y_sb + to * g.y_st + static_cast<int64_t>(h) * g.y_sh + 16 * u) = v;
}

// COPY, one lane per byte: item = (tok H + h) D + f
__global__ __launch_bounds__(kBlock) void rope_w8_copy_generic_kernel(RopeGeom g, const int32_t* __restrict__ pos, const uint8_t* __restrict__ x,
                                                                       uint8_t* __restrict__ y) {
    const uint32_t item = blockIdx.x * static_cast<uint32_t>(kBlock) + threadIdx.x;
    if (item >= g.items) return;
    const uint32_t r0 = item / static_cast<uint32_t>(g.U), f = item - r0 * static_cast<uint32_t>(g.U);
    const uint32_t tok = r0 / static_cast<uint32_t>(g.H), h = r0 - tok * static_cast<uint32_t>(g.H);
    int b, t, p, to;
    if (!rope_place(g, pos, tok, g.Tout, b, t, p, to)) return;
    y[b * g.y_sb + to * g.y_st + static_cast<int64_t>(h) * g.y_sh + f] = x[b * g.x_sb + t * g.x_st + static_cast<int64_t>(h) * g.x_sh + f];
}

// ------------------------------------------------------------------------------------------------
// host side: the plan
// ------------------------------------------------------------------------------------------------
struct RopePlan {
    int family, kernel, block;
    int64_t grid, items;
    RopeGeom g;
};

// `y_elem`: 0 where a base is not 16-byte aligned, else the bytes of one element of y
inline RopePlan plan_rope(const lsq_rope_w8_geom& ge, int64_t y_elem) {
    RopePlan pl = {};
    pl.block = kBlock;
    const bool copy = ge.mode == LSQ_ROPE_W8_COPY, inter = ge.style == LSQ_ROPE_W8_INTERLEAVED;
    const int64_t R = copy ? 0 : ge.R;
    RopeGeom& g = pl.g;
    g = RopeGeom{ge.x_sb, ge.x_st, ge.x_sh, ge.y_sb, ge.y_st, ge.y_sh, static_cast<int>(ge.T), static_cast<int>(ge.H), static_cast<int>(ge.D),
                 static_cast<int>(R), static_cast<int>(copy ? ge.Tout : ge.P), static_cast<int>(ge.Tout), 0, 0, static_cast<int>(ge.H), 1,
                 static_cast<int>(ge.scatter), inter ? 1 : 0, ge.x_dtype == LSQ_ROPE_W8_I8 ? 0x80808080u : 0u, 0u};
    const int64_t tokens = ge.B * ge.T;
    bool packets = y_elem > 0 && ge.D % 16 == 0 && ge.x_sb % 16 == 0 && ge.x_st % 16 == 0 && ge.x_sh % 16 == 0 &&
                   ge.y_sb * y_elem % 16 == 0 && ge.y_st * y_elem % 16 == 0 && ge.y_sh * y_elem % 16 == 0;
    if (!copy) packets = packets && R % (inter ? 16 : 32) == 0;
    if (!packets) {
        pl.family = LSQ_ROPE_W8_GENERIC;
        pl.kernel = copy ? kRopeCopyGeneric : kRopeGeneric;
        g.UR = static_cast<int>(R / 2);
        g.U = static_cast<int>(copy ? ge.D : R / 2 + ge.D - R);
        pl.items = tokens * ge.H * g.U;
    } else if (copy) {
        pl.family = LSQ_ROPE_W8_PACKETS;
        pl.kernel = kRopeCopyPackets;
        g.U = static_cast<int>(ge.D / 16);
        pl.items = tokens * ge.H * g.U;
    } else {
        pl.family = LSQ_ROPE_W8_PACKETS;
        pl.kernel = inter ? kRopeInter : kRopeHalf;
        g.UR = static_cast<int>(inter ? R / 16 : R / 32);
        g.U = g.UR + static_cast<int>((ge.D - R) / 16);
        const int64_t fill = static_cast<int64_t>(device_info().cu_count) * kRopeBlocksPerCU;
        int hpl = static_cast<int>(std::min<int64_t>(ge.H, kRopeMaxHeads));
        while (hpl > 1 && ceil_div(tokens * ceil_div(ge.H, hpl) * g.U, kBlock) < fill) hpl /= 2;
        g.hpl = hpl;
        g.HG = static_cast<int>(ceil_div(ge.H, hpl));
        pl.items = tokens * g.HG * g.U;
    }
    pl.grid = ceil_div(pl.items, kBlock);
    g.items = static_cast<uint32_t>(std::min<int64_t>(pl.items, UINT32_MAX));
    return pl;
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_rope_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int64_t kMaxGrid = (int64_t{1} << 24) - 1;
constexpr int64_t kMaxElems = int64_t{1} << 40;
constexpr int64_t kMaxOffset = int64_t{1} << 58;

int check_grid(const char* what, int64_t grid) {
    // 256 threads a workgroup: the whole launch stays below 2^32 threads, and an item index fits 32 bits
    if (grid > kMaxGrid) return fail(LSQ_EINVAL, "%s: %lld workgroups are beyond 2^24 - 1", what, static_cast<ll>(grid));
    return LSQ_OK;
}

// y's (b, token, h) rows must not overlap each other: the strides sorted, each must clear the span of those below it
bool rope_self_overlap(const int64_t (&strides)[3], const int64_t (&extents)[3], int64_t cols) {
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

int64_t x_span(const lsq_rope_w8_geom& g) { return (g.B - 1) * g.x_sb + (g.T - 1) * g.x_st + (g.H - 1) * g.x_sh + g.D; }
int64_t y_span(const lsq_rope_w8_geom& g) { return (g.B - 1) * g.y_sb + (g.Tout - 1) * g.y_st + (g.H - 1) * g.y_sh + g.D; }

int check_rope_geom(const char* what, const lsq_rope_w8_geom* g) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (g->x_dtype != LSQ_ROPE_W8_U8 && g->x_dtype != LSQ_ROPE_W8_I8)
        return fail(LSQ_EINVAL, "%s: x_dtype must be LSQ_ROPE_W8_U8 (0) or LSQ_ROPE_W8_I8 (1), got %lld", what, static_cast<ll>(g->x_dtype));
    if (g->mode != LSQ_ROPE_W8_ROTATE && g->mode != LSQ_ROPE_W8_COPY)
        return fail(LSQ_EINVAL, "%s: mode must be LSQ_ROPE_W8_ROTATE (0) or LSQ_ROPE_W8_COPY (1), got %lld", what, static_cast<ll>(g->mode));
    if (g->scatter != 0 && g->scatter != 1) return fail(LSQ_EINVAL, "%s: scatter must be 0 or 1, got %lld", what, static_cast<ll>(g->scatter));
    const bool copy = g->mode == LSQ_ROPE_W8_COPY;
    if (g->B < 1 || g->T < 1 || g->H < 1 || g->D < 1 || g->Tout < 1)
        return fail(LSQ_EINVAL, "%s: x is [B, T, H, D] = [%lld, %lld, %lld, %lld] and Tout = %lld, every extent must be at least 1", what,
                    static_cast<ll>(g->B), static_cast<ll>(g->T), static_cast<ll>(g->H), static_cast<ll>(g->D), static_cast<ll>(g->Tout));
    const int64_t lim = INT32_MAX / 4;
    if (g->B > lim || g->T > lim || g->H > lim || g->D > lim || g->Tout > lim) return fail(LSQ_EINVAL, "%s: an extent is beyond 29 bits", what);
    if (!copy) {
        if (g->style != LSQ_ROPE_W8_HALF && g->style != LSQ_ROPE_W8_INTERLEAVED)
            return fail(LSQ_EINVAL, "%s: style must be LSQ_ROPE_W8_HALF (0) or LSQ_ROPE_W8_INTERLEAVED (1), got %lld", what, static_cast<ll>(g->style));
        if (g->P < 1) return fail(LSQ_EINVAL, "%s: the tables hold P = %lld positions, at least 1 is needed", what, static_cast<ll>(g->P));
        if (g->P > lim) return fail(LSQ_EINVAL, "%s: P = %lld is beyond 29 bits", what, static_cast<ll>(g->P));
        if (g->R < 2 || g->R % 2 != 0 || g->R > g->D)
            return fail(LSQ_EINVAL, "%s: the rotary dimension R = %lld must be even, at least 2 and at most D = %lld", what, static_cast<ll>(g->R),
                        static_cast<ll>(g->D));
    }
    if (!g->scatter && g->Tout < g->T)
        return fail(LSQ_EINVAL, "%s: without scatter token t goes to output token t: Tout = %lld must be at least T = %lld", what,
                    static_cast<ll>(g->Tout), static_cast<ll>(g->T));
    if (g->B * std::max(g->T, g->Tout) > kMaxElems / (g->H * g->D)) return fail(LSQ_EINVAL, "%s: the shapes are beyond 2^40 elements", what);
    const int64_t st[6] = {g->x_sb, g->x_st, g->x_sh, g->y_sb, g->y_st, g->y_sh}, ex[6] = {g->B, g->T, g->H, g->B, g->Tout, g->H};
    for (int i = 0; i < 6; ++i)
        if (st[i] < 0 || st[i] > kMaxOffset / ex[i])
            return fail(LSQ_EINVAL, "%s: the strides (%lld, %lld, %lld) of x and (%lld, %lld, %lld) of y must not be negative and must keep "
                        "every offset within 2^58", what, static_cast<ll>(st[0]), static_cast<ll>(st[1]), static_cast<ll>(st[2]),
                        static_cast<ll>(st[3]), static_cast<ll>(st[4]), static_cast<ll>(st[5]));
    const int64_t ys[3] = {g->y_sb, g->y_st, g->y_sh}, ye[3] = {g->B, g->Tout, g->H};
    if (rope_self_overlap(ys, ye, g->D))
        return fail(LSQ_EINVAL, "%s: under y's strides (%lld, %lld, %lld) two rows of D = %lld elements overlap", what, static_cast<ll>(g->y_sb),
                    static_cast<ll>(g->y_st), static_cast<ll>(g->y_sh), static_cast<ll>(g->D));
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_rope_w8_abi_version(void) { return LSQ_ROPE_W8_ABI_VERSION; }

const char* lsq_rope_w8_last_error(void) { return g_last_error; }

int lsq_rope_w8(const lsq_rope_w8_geom* geom, const lsq_rope_w8_in* in, const lsq_rope_w8_out* out, const void* cos, const void* sin,
                const void* positions, const void* x_levels, void* y, void* stream) {
    const char* what = "lsq_rope_w8";
    lsq::RopeArg arg{};
    int64_t y_elem = 1;
    if (int rc = check_rope_geom(what, geom)) return rc;
    const bool copy = geom->mode == LSQ_ROPE_W8_COPY;
    if (copy) {
        if (in || out || cos || sin)
            return fail(LSQ_EINVAL, "%s: LSQ_ROPE_W8_COPY moves bytes: the input side, the output side, cos and sin must be NULL", what);
    } else {
        if (!in || !in->s_x || !in->zx) return fail(LSQ_EINVAL, "%s: NULL input side, s_x or zx", what);
        if (!out) return fail(LSQ_EINVAL, "%s: NULL output description", what);
        if (!cos || !sin) return fail(LSQ_EINVAL, "%s: NULL cos or sin", what);
        if (!aligned_to(in->s_x, 4) || !aligned_to(in->zx, 4)) return fail(LSQ_EINVAL, "%s: s_x and zx must be element-aligned", what);
        if (!aligned_to(cos, 4) || !aligned_to(sin, 4)) return fail(LSQ_EINVAL, "%s: cos and sin must be element-aligned", what);
        if (int rc = check_out_side(what, *out, arg, y_elem)) return rc;
        arg.s_x = static_cast<const float*>(in->s_x);
        arg.zx = static_cast<const int32_t*>(in->zx);
    }
    if (!x_levels || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (positions && !aligned_to(positions, 4)) return fail(LSQ_EINVAL, "%s: positions must be 4-byte aligned", what);
    if (!aligned_to(y, static_cast<uintptr_t>(y_elem))) return fail(LSQ_EINVAL, "%s: a floating y must be element-aligned", what);
    const int64_t x_bytes = x_span(*geom), y_bytes = y_span(*geom) * y_elem;
    if (overlap(y, y_bytes, x_levels, x_bytes))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap x's %lld: the op in place is not served", what, static_cast<ll>(y_bytes),
                    static_cast<ll>(x_bytes));
    if (!copy) {
        const int64_t t_bytes = geom->P * (geom->R / 2) * 4;
        if (overlap(y, y_bytes, cos, t_bytes) || overlap(y, y_bytes, sin, t_bytes))
            return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap the %lld bytes of cos or sin", what, static_cast<ll>(y_bytes), static_cast<ll>(t_bytes));
    }
    if (positions && overlap(y, y_bytes, positions, 4 * geom->B))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap the %lld entries of positions", what, static_cast<ll>(y_bytes), static_cast<ll>(geom->B));
    const bool aligned = aligned_to(x_levels, 16) && aligned_to(y, 16) && (copy || (aligned_to(cos, 16) && aligned_to(sin, 16)));
    const lsq::RopePlan pl = lsq::plan_rope(*geom, aligned ? y_elem : 0);
    if (int rc = check_grid(what, pl.grid)) return rc;
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kBlock);
    const uint8_t* x = static_cast<const uint8_t*>(x_levels);
    const float* ct = static_cast<const float*>(cos);
    const float* st = static_cast<const float*>(sin);
    const int32_t* ps = static_cast<const int32_t*>(positions);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (pl.kernel) {
        case lsq::kRopeHalf: hipLaunchKernelGGL(lsq::rope_w8_packets_kernel<false>, grid, block, 0, s, pl.g, arg, ct, st, ps, x, y); break;
        case lsq::kRopeInter: hipLaunchKernelGGL(lsq::rope_w8_packets_kernel<true>, grid, block, 0, s, pl.g, arg, ct, st, ps, x, y); break;
        case lsq::kRopeCopyPackets:
            hipLaunchKernelGGL(lsq::rope_w8_copy_packets_kernel, grid, block, 0, s, pl.g, ps, x, static_cast<uint8_t*>(y));
            break;
        case lsq::kRopeCopyGeneric:
            hipLaunchKernelGGL(lsq::rope_w8_copy_generic_kernel, grid, block, 0, s, pl.g, ps, x, static_cast<uint8_t*>(y));
            break;
        default: hipLaunchKernelGGL(lsq::rope_w8_generic_kernel, grid, block, 0, s, pl.g, arg, ct, st, ps, x, y); break;
    }
    return hip_status(hipGetLastError(), what);
}

int lsq_rope_w8_plan(const lsq_rope_w8_geom* geom, int aligned, int32_t* out8) {
    const char* what = "lsq_rope_w8_plan";
    if (int rc = check_rope_geom(what, geom)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    if (aligned != 0 && aligned != 1 && aligned != 2 && aligned != 4)
        return fail(LSQ_EINVAL, "%s: aligned must be 0 or the bytes of one element of y (1, 2 or 4), got %d", what, aligned);
    if (geom->mode == LSQ_ROPE_W8_COPY && aligned > 1) return fail(LSQ_EINVAL, "%s: LSQ_ROPE_W8_COPY moves bytes: aligned must be 0 or 1", what);
    const lsq::RopePlan pl = lsq::plan_rope(*geom, aligned);
    if (int rc = check_grid(what, pl.grid)) return rc;
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.block;
    out8[3] = pl.g.hpl;
    out8[4] = pl.g.U;
    out8[5] = pl.g.UR;
    out8[6] = 0;
    out8[7] = pl.kernel;
    return LSQ_OK;
}

}  // extern "C"
