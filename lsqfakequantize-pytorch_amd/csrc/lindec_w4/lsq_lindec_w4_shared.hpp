// lsq_lindec_w4_shared.hpp -- what the decode-shape kernels on packed 4- / 2-bit codes with an 8-bit output say the same way:
// csrc/lindec_w4/lsq_lindec_w4.hip (one weight strip, levels out), csrc/linmid_w4/lsq_linmid_w4.hip (the same for 17 to 64 rows) and
// csrc/linglu_w4/lsq_linglu_w4.hip (a gate and an up strip, the gated product's levels out).  The cut of K (which fixes the order
// of the fp32 sum: include/lsq_hip_lindec_w4.h), the kernel
// arguments, the permuted LDS layout of x with the staging of a chunk, the walk of a wave over its load steps, the hand-over of a
// group's constants and the byte after v.  The two libraries stay separate; each compiles these pieces into its own kernels.
#pragma once
#include "../resadd_w8/lsq_resadd_w8_tiles.hpp"
#include "../requant_w8/lsq_requant_w8_checks.hpp"
#include "../../../include/lsq_hip_resadd_w8.h"

namespace lsq {

constexpr int kW4TileBytes = kQTile * kQTile;       // one [16][16] byte tile
constexpr int64_t kW4MaxK = int64_t{1} << 30, kW4MaxN = int64_t{1} << 30;     // tiles, chunks and packets count in 32 bits
constexpr int kW4FastZero = 256;                    // |qzero| up to here: I fits 32 bits for every G that is served

struct W4Geom {             // kernel argument: the cut of K (host: w4_cut), csrc/qlinear_a8/'s
    int64_t N, K, n_packets, n_groups;
    int G;
    int ppg;                // 16-byte code packets per group
    int span_p;             // packets per span: lcm(ppg, 4)
    int steps_per_span;     // span_p / 4
    int groups_per_span;    // span_p / ppg
    int chunk_spans;        // spans per chunk of x
    int chunk_k;            // elements of K per chunk
    int chunk_groups;       // groups per chunk
    int n_chunks;           // chunks of K
    int row_stride;         // bytes between rows of x in LDS
    int gstride;            // groups per row of the LDS table of sum a - G z
};

struct W4Weight {           // kernel argument
    const uint8_t* codes;
    const float* qscale;
    const int32_t* qzero;
    const void* bias;
    int bias_dtype;
};

// where element j of a block of 16 consecutive k lies in LDS: 4 bits (8 codes per dword): the even codes, then the odd ones;
// 2 bits (16 codes per dword): codes 0, 4, 8, 12, then 1, 5, 9, 13, ...
template <int BITS>
__device__ __forceinline__ constexpr int w4_lds_pos(int j) {
    return BITS == 4 ? (j & 8) + (j & 1) * 4 + ((j & 7) >> 1) : (j & 3) * 4 + (j >> 2);
}

// 16 byte operands in memory order -> in LDS order
template <int BITS>
__device__ __forceinline__ u32x4 w4_deinterleave(u32x4 v) {
    const uint32_t s[4] = {v.x, v.y, v.z, v.w};
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int pos = w4_lds_pos<BITS>(j);
        w[pos >> 2] |= ((s[j >> 2] >> ((j & 3) * 8)) & 0xffu) << ((pos & 3) * 8);
    }
    return u32x4{w[0], w[1], w[2], w[3]};
}

// w8q_byte's steps after v (csrc/requant_w8/lsq_requant_w8_tiles.hpp): the rounding to mid_dtype, the select, the level
__device__ __forceinline__ uint8_t w4q_byte(float v, const W8OutQ& oq) {
    float u = w8r_round(v, oq.mid);
    if (oq.relu) u = (u < 0.0f) ? 0.0f : u;         // a select: a NaN stays a NaN and goes to quant_min below
    return static_cast<uint8_t>(static_cast<int>(level<float>(u, oq.qp, oq.r)) & 0xff);
}

// w8r_byte's steps after v (csrc/resadd_w8/lsq_resadd_w8_tiles.hpp): u, the optional p, d, t, the select, the level.  Every step is
// rounded once: the product d and the sum p + d are NOT one fused multiply-add.
__device__ __forceinline__ uint8_t w4r_byte(float v, const W8OutQ& oq, const W8PreQ& pq, const W8ResQ& rq, uint8_t lr) {
    const float u = w8r_round(v, oq.mid);
    float p = u;
    if (pq.on) p = w8r_round(dequant<float>(level<float>(u, pq.qp, pq.r), pq.qp), oq.mid);
    const float lf = rq.is_signed ? static_cast<float>(static_cast<int8_t>(lr)) : static_cast<float>(lr);
    const float d = w8r_round(__fmul_rn(__fsub_rn(lf, rq.z), rq.s), oq.mid);
    float t = w8r_round(__fadd_rn(p, d), oq.mid);
    if (oq.relu) t = (t < 0.0f) ? 0.0f : t;
    return static_cast<uint8_t>(static_cast<int>(level<float>(t, oq.qp, oq.r)) & 0xff);
}

struct W4Cursor {           // a wave's walk over its load steps of one chunk; everything in it is the same for the whole wave
    int p;                  // the step's first packet, counted from the chunk's first
    int l;                  // the step's index in its span
    int pig;                // packets of the current group behind the cursor
    int g;                  // the current group's index in the chunk
};

struct W4Step {             // one load step in flight: 4 packets of each of the 16 rows
    u32x4 raw;
    float qs;               // lane (n, q): the constants of row n's group that ends at place q of the step, if one does (a place:
    int32_t qz;             // one MFMA, NS of them per step) -- one pair per lane; w4_from_place hands it to the row's four lanes
    int p;                  // the step's first packet in the chunk; -1: past the wave's last step of the chunk
};

// lane (n, q) reads v of lane (n, place): the LDS crossbar, no memory.  Called by whole waves only.
template <typename T>
__device__ __forceinline__ T w4_from_place(T v, int lane, int place) {
    return __shfl(v, (lane & 15) + 16 * place, 64);
}

// One chunk of x into LDS, by the whole workgroup (the caller's barrier precedes: nobody reads the previous chunk any more): the
// `np` packets' worth of level bytes of the M rows from k = kc0 on, ^ flip, each block of 16 bytes in w4_lds_pos's order, rows
// geo.row_stride apart in `xs`; then sum a - G z per (row, group) into aeff[m * geo.gstride + g].  Ends with a barrier.
template <int BITS>
__device__ __forceinline__ void w4_stage_chunk(const W8Act& act, const W8Const& ac, int M, const W4Geom& geo, int64_t kc0, int np,
                                               unsigned char* xs, int32_t* aeff, int tid) {
    constexpr int BE = 128 / BITS;                  // elements per 16-byte packet
    const int bpr = np * (BE / 16);                 // blocks of 16 k per row
    for (int it = tid; it < M * bpr; it += kQBlock) {
        const int m = it / bpr, b = it - m * bpr;
        const u32x4 v = *reinterpret_cast<const u32x4*>(act.a + static_cast<int64_t>(m) * geo.K + kc0 + b * 16) ^ ac.flip;
        *reinterpret_cast<u32x4*>(xs + m * geo.row_stride + b * 16) = w4_deinterleave<BITS>(v);
    }
    __syncthreads();
    const int ng = np * BE / geo.G;                 // groups of this chunk; exact
    for (int it = tid; it < M * ng; it += kQBlock) {
        const int m = it / ng, g = it - m * ng;
        const unsigned char* src = xs + m * geo.row_stride + g * geo.G;
        int sum = 0;
        for (int b = 0; b < geo.G; b += 16) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(src + b);
            sum += w8_sum_bytes(v.x) + w8_sum_bytes(v.y) + w8_sum_bytes(v.z) + w8_sum_bytes(v.w);
        }
        aeff[m * geo.gstride + g] = sum - geo.G * ac.z;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// host side: the cut of K
// ------------------------------------------------------------------------------------------------
// csrc/qlinear_a8/'s plan_a8 (matrix-core form): the order of the sum is fixed by it.  False: the format, the shape or the
// alignment is not served (`g` is untouched).  `pair`: two adjacent packets of one group per MFMA (4 bits, an even ppg).
inline bool w4_cut(int64_t M, int64_t N, int64_t K, int64_t G, int bits, bool aligned, int max_rows, W4Geom& g, bool& pair) {
    const int64_t BE = 128 / bits;
    int64_t span_p = 0;
    if (G % BE == 0) {
        const int64_t ppg = G / BE;
        span_p = ppg % 4 == 0 ? ppg : (ppg % 2 == 0 ? ppg * 2 : ppg * 4);      // lcm(ppg, 4)
    }
    if (!(aligned && M >= 1 && M <= max_rows && K > 0 && K <= kW4MaxK && N <= kW4MaxN && span_p > 0 && span_p * BE <= kQChunk))
        return false;
    g.N = N;
    g.K = K;
    g.n_groups = K / G;
    g.n_packets = K / BE;
    g.G = static_cast<int>(G);
    g.ppg = static_cast<int>(G / BE);
    g.span_p = static_cast<int>(span_p);
    g.steps_per_span = g.span_p / 4;
    g.groups_per_span = g.span_p / g.ppg;
    g.chunk_spans = static_cast<int>(kQChunk / (span_p * BE));
    g.chunk_k = static_cast<int>(g.chunk_spans * span_p * BE);
    g.chunk_groups = g.chunk_spans * g.groups_per_span;
    g.n_chunks = static_cast<int>((K + g.chunk_k - 1) / g.chunk_k);
    const int64_t held = std::max<int64_t>(BE, std::min<int64_t>(g.chunk_k, K));           // elements of one row in LDS
    g.row_stride = static_cast<int>(held) + kQRowPad;
    g.gstride = static_cast<int>(std::max<int64_t>(1, held / G));
    pair = bits == 4 && g.ppg % 2 == 0;
    return true;
}

}  // namespace lsq

namespace {

// the format's checks, said as lsq_qdecode.hpp's check_shape says them; M is not bounded here (the plans answer for any M)
int check_format(const char* what, int64_t M, int64_t N, int64_t K, int64_t G, int bits) {
    if (bits != 4 && bits != 2) return fail(LSQ_EINVAL, "%s: bits must be 4 or 2, got %d", what, bits);
    if (G <= 0) return fail(LSQ_EINVAL, "%s: group_size must be positive, got %lld", what, static_cast<ll>(G));
    if (int rc = check_linear_shape(what, M, N, K)) return rc;
    if (K % G != 0) return fail(LSQ_EINVAL, "%s: K = %lld is not a multiple of group_size %lld", what, static_cast<ll>(K), static_cast<ll>(G));
    if (G % (8 / bits) != 0)
        return fail(LSQ_EINVAL, "%s: group_size %lld is not a multiple of %d, the elements of one byte of %d-bit codes", what,
                    static_cast<ll>(G), 8 / bits, bits);
    return LSQ_OK;
}


// the residual's and the pre-quantizer's checks, said as csrc/resadd_w8/lsq_resadd_w8.hip and csrc/lindec_w8/lsq_lindec_w8.hip say
// them (translation units, not headers: a fix there belongs here too); `MN`: the bytes of y and of the residual
inline int check_res(const char* what, const lsq_resadd_w8_res* r, const void* y, int64_t MN, lsq::W8ResArg& arg) {
    if (r->level_dtype != LSQ_REQUANT_W8_U8 && r->level_dtype != LSQ_REQUANT_W8_I8)
        return fail(LSQ_EINVAL, "%s: the residual's level_dtype must be LSQ_REQUANT_W8_U8 (0) or LSQ_REQUANT_W8_I8 (1), got %lld", what,
                    static_cast<ll>(r->level_dtype));
    if (!r->levels || !r->scale || !r->zero_point) return fail(LSQ_EINVAL, "%s: NULL residual levels, scale or zero_point", what);
    if (!aligned_to(r->scale, 4) || !aligned_to(r->zero_point, 4))
        return fail(LSQ_EINVAL, "%s: the residual's scale and zero_point must be element-aligned", what);
    const uintptr_t a = reinterpret_cast<uintptr_t>(r->levels), b = reinterpret_cast<uintptr_t>(y), n = static_cast<uintptr_t>(MN);
    if (a < b + n && b < a + n)
        return fail(LSQ_EINVAL, "%s: the residual's %lld bytes overlap y's: an in-place add is not served", what, static_cast<ll>(MN));
    arg = lsq::W8ResArg{static_cast<const uint8_t*>(r->levels), static_cast<const float*>(r->scale),
                        static_cast<const int32_t*>(r->zero_point), r->level_dtype == LSQ_REQUANT_W8_I8 ? 1 : 0, 0};
    return LSQ_OK;
}

inline int check_pre(const char* what, const lsq_resadd_w8_pre* p, lsq::W8PreArg& arg) {
    arg = lsq::W8PreArg{nullptr, nullptr, 0.0f, 0.0f, 0.0f, 0.0f};
    if (!p) return LSQ_OK;
    if (!p->scale || !p->shift) return fail(LSQ_EINVAL, "%s: NULL scale or shift of the pre-quantizer", what);
    if (!aligned_to(p->scale, 4) || !aligned_to(p->shift, 4))
        return fail(LSQ_EINVAL, "%s: the pre-quantizer's scale and shift must be element-aligned", what);
    if (int rc = check_byte_range(what, "the pre-quantizer's ", p->quant_min, p->quant_max, p->type_min, p->type_max)) return rc;
    arg = lsq::W8PreArg{static_cast<const float*>(p->scale), static_cast<const float*>(p->shift), static_cast<float>(p->quant_min),
                        static_cast<float>(p->quant_max), static_cast<float>(p->type_min), static_cast<float>(p->type_max)};
    return LSQ_OK;
}

}  // namespace
