// lsq_qgemm_a8.hip -- 8-bit activation levels times packed 4- / 2-bit group-wise weight codes for ANY number of rows of x on
// gfx950 (include/lsq_hip_qgemm_a8.h, which states the contract; the op is include/lsq_hip_qlinear_a8.h's, the weight format
// include/lsq_hip_pack.h's): the kernels and the C ABI of liblsq_hip_qgemm_a8.so.
//
// The result is, row for row, the bits of the decode kernel (qlinear_a8/lsq_qlinear_a8.hip).  What is kept of it: the byte
// operand a = lx - off and z = zx - off, I = sum a c - z sum c - q (sum a - G z) in integers, sum c from a second MFMA with an
// all-ones A operand, the mask / shift unpack of the codes into the B operand of v_mfma_i32_16x16x64_i8, the de-interleaved
// order of x in LDS (a8_lds_pos), the 16-byte non-temporal code load and the 4 x 4 transpose over the lanes
// (qlinear/lsq_qdecode.hpp).  What is new:
//  * TILES.  A workgroup owns 16 * SUBS rows of x by 16 * WAVES columns; wave w owns columns 16 w .. 16 w + 15 of the tile and
//    all its rows.  WAVES is 4, or 1 while 64-column tiles would not give every compute unit a tile; SUBS is 8, or 4 / 2 when
//    all of M is at most 64 / 32 rows (plan_g8).  blockIdx.x = column tile * row tiles + row tile.
//  * K WALK, CHAIN BY CHAIN.  The decode kernel gives span s of a chunk to wave s % 16 and sums the 16 waves' fp32
//    accumulators in wave order.  Here every wave walks all of K itself, in that order: chain w = 0..15 in turn, and for a
//    chain the chunks ascending, the spans w, w + 16, ... of the chunk ascending, the load steps (4 packets) of the span
//    ascending (G8Walk).  acc holds the running chain, sum the chains folded so far: two fp32 accumulator sets per sub-tile.
//    The codes of a column are read in runs of one span at a stride of 16 spans; nothing about the walk depends on M.
//  * ONE STEP.  The workgroup stages the step's 4 packets of x of each of its rows in LDS as the bytes a[m, k] (rows beyond M
//    are zero), and with them sum a per (row, packet); lane (n, q) has loaded packet p0 + q of its column one step ahead.
//    Per packet (or pair of packets at 4 bits) ONE B fragment is unpacked, one MFMA gives sum c, and the fragment runs
//    against the A fragment of each of the SUBS sub-tiles.  When a group ends I is formed and acc = acc + qscale * float(I):
//    a rounded multiply, then a rounded add, as the decode kernel's code has them.
//  * The fused form's levels are formed ONCE, by a pre-pass (levels_kernel) into the caller's workspace.
#include "../qlinear/lsq_qdecode.hpp"
#include "../../../include/lsq_hip_qgemm_a8.h"

#include <climits>

namespace lsq {

constexpr int kG8Chains = kQWaves;                  // fp32 chains per output: the decode kernel's waves
constexpr int kG8Sub = 8;                           // most 16-row sub-tiles per workgroup
constexpr int kG8Wide = 4;                          // waves (16 columns each) of the wide tile
constexpr int kG8FastZero = 256;                    // |qzero| up to here: I fits 32 bits for every G served

struct G8Act {              // kernel argument: where the byte operand and its constants come from
    const uint8_t* a;       // levels form: the levels; fused form: the workspace, a = level(x) - off already
    const float* scale;     // levels form: s_x; fused form: the quantizer's scale
    const float* shift;     // fused form
    const int32_t* zx;      // levels form
    float qmin, qmax, tmin, tmax;   // fused form
    int off;                // 128: levels in 0..255; 0: levels in -128..127
    int fused;
    int aligned;            // `a` is 16-byte aligned
};

struct G8Const {
    int z;                  // zx - off
    float s_x;
    uint32_t flip;          // byte ^ 0x80 read as int8 is byte - 128
};

__device__ __forceinline__ G8Const g8_constants(const G8Act& a) {
    G8Const c;
    if (a.fused) {
        const Range<float> r = Range<float>{a.qmin, a.qmax, a.tmin, a.tmax};
        const QParams<float> q = make_qparams<float>(sanitize_scale_per_tensor<float>(a.scale[0]), a.shift[0], r);
        c.z = static_cast<int>(q.zp) - a.off;
        c.s_x = q.s;
        c.flip = 0u;
    } else {
        c.z = a.zx[0] - a.off;
        c.s_x = a.scale[0];
        c.flip = a.off ? 0x80808080u : 0u;
    }
    return c;
}

struct G8Geom {             // kernel argument: the cut of K, which is plan_a8's
    int64_t M, N, K, n_groups, n_packets, row_tiles, n_chunks, chunk_p;
    int G;
    int ppg;                // 16-byte code packets per group
    int ppg_shift;          // log2(ppg) or -1
    DivU64 ppg_div;
    int span_p;             // packets per span: lcm(ppg, 4)
    int steps_per_span;     // span_p / 4
    int chunk_spans;        // spans per chunk
};

// where element j of a block of 16 consecutive k lies in LDS (the decode kernel's a8_lds_pos)
template <int BITS>
__device__ __forceinline__ constexpr int g8_lds_pos(int j) {
    return BITS == 4 ? (j & 8) + (j & 1) * 4 + ((j & 7) >> 1) : (j & 3) * 4 + (j >> 2);
}

__device__ __forceinline__ int g8_sum_bytes(uint32_t w) {
    return static_cast<int>(static_cast<int8_t>(w)) + static_cast<int>(static_cast<int8_t>(w >> 8)) +
           static_cast<int>(static_cast<int8_t>(w >> 16)) + (static_cast<int>(w) >> 24);
}

// a position of the walk over K: chain w, chunk c, span `span` of the chunk, load step l of the span
struct G8Walk {
    int w, span, l;
    int64_t c;
};

// the first load step at or after `k` in walk order whose first packet exists; false when the walk is over.  The same for
// every thread of the grid.
__device__ __forceinline__ bool g8_settle(G8Walk& k, const G8Geom& geo, int64_t& p0) {
    for (;;) {
        if (k.w >= kG8Chains) return false;
        if (k.c >= geo.n_chunks) {
            ++k.w;
            k.c = 0;
            k.span = k.w;
            k.l = 0;
            continue;
        }
        if (k.span < geo.chunk_spans) {
            p0 = k.c * geo.chunk_p + static_cast<int64_t>(k.span) * geo.span_p + k.l * 4;
            if (p0 < geo.n_packets) return true;
        }
        ++k.c;                                      // the later spans of this chunk lie further still
        k.span = k.w;
        k.l = 0;
    }
}

__device__ __forceinline__ void g8_advance(G8Walk& k, const G8Geom& geo) {
    if (++k.l == geo.steps_per_span) {
        k.l = 0;
        k.span += kG8Chains;
    }
}

struct G8Step {             // one load step in flight: 4 packets of each of the wave's 16 columns
    u32x4 raw;
    float qs[4];
    int32_t qz[4];
    int64_t p0;
    int w;
};

__device__ __forceinline__ float g8_bias_at(const void* bias, int bias_dtype, int64_t n) {
    if (!bias) return 0.0f;
    switch (bias_dtype) {
        case LSQ_BF16: return io_bf16::load1(bias, n);
        case LSQ_F16: return io_f16::load1(bias, n);
        default: return static_cast<const float*>(bias)[n];
    }
}

template <int BITS, bool PAIR, int WAVES, int SUBS>
__global__ __launch_bounds__(WAVES * 64, 2) void qgemm_a8_kernel(G8Act act, const uint8_t* __restrict__ codes, G8Geom geo,
                                                             const float* __restrict__ qscale, const int32_t* __restrict__ qzero,
                                                             const void* __restrict__ bias, int bias_dtype, void* __restrict__ y,
                                                             int y_dtype) {
    constexpr int BE = 128 / BITS;                  // elements per 16-byte code packet = bytes of x per packet
    constexpr int kStride = 4 * BE + kQRowPad;      // bytes between rows of x in LDS
    constexpr int kRows = SUBS * 16;
    constexpr int kThreads = WAVES * 64;
    constexpr int PER = PAIR ? 2 : 1;               // packets per MFMA
    static_assert(!PAIR || BITS == 4, "two packets per MFMA only at 4 bits: a 2-bit packet is 64 elements already");
    extern __shared__ __attribute__((aligned(16))) unsigned char xs[];
    int32_t* asum = reinterpret_cast<int32_t*>(xs + kRows * kStride);          // [4 packets][kRows]: sum a

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const G8Const ac = g8_constants(act);
    const int64_t K = geo.K, N = geo.N, n_packets = geo.n_packets;
    const int64_t tile = static_cast<int64_t>(blockIdx.x);
    const int64_t col_tile = tile / geo.row_tiles, row_tile = tile - col_tile * geo.row_tiles;
    const int64_t m0 = row_tile * kRows;
    const int rows = static_cast<int>(std::min<int64_t>(kRows, geo.M - m0));   // >= 1
    const int64_t n0 = (col_tile * WAVES + wave) * 16;
    const int64_t row = std::min<int64_t>(n0 + nl, N - 1);                     // a clamped row computes a value nobody stores
    const uint8_t* __restrict__ wrow = codes + row * (n_packets * 16);
    const float* __restrict__ qs_row = qscale + row * geo.n_groups;
    const int32_t* __restrict__ qz_row = qzero + row * geo.n_groups;
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const int gz = geo.G * ac.z;

    f32x4 acc[SUBS], sum[SUBS];
    i32x4 P[SUBS], A[SUBS];
#pragma unroll
    for (int rt = 0; rt < SUBS; ++rt) {
        acc[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        sum[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        P[rt] = i32x4{0, 0, 0, 0};
        A[rt] = i32x4{0, 0, 0, 0};
    }
    i32x4 C = {0, 0, 0, 0};
    int pig = 0;                                    // packets of the current group already summed
    int cur_w = 0;                                  // the chain acc belongs to

    auto load_step = [&](G8Step& s, const G8Walk& at, int64_t p0) {
        s.p0 = p0;
        s.w = at.w;
        s.raw = u32x4{0u, 0u, 0u, 0u};
        if (p0 + q < n_packets) s.raw = load_code_packet(wrow, p0 + q);
#pragma unroll
        for (int t = 0; t < 4; ++t) load_packet_scale(qs_row, qz_row, p0 + t, n_packets, geo.ppg_shift, geo.ppg_div, s.qs[t], s.qz[t]);
    };
    // chain cur_w is complete: sum = sum + acc, the decode kernel's sum over its waves in wave order
    auto fold_chain = [&]() {
#pragma unroll
        for (int rt = 0; rt < SUBS; ++rt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sum[rt][i] = __fadd_rn(sum[rt][i], acc[rt][i]);
            acc[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        ++cur_w;
    };

    G8Walk ld = {0, 0, 0, 0};
    int64_t p_next = 0;
    bool more = g8_settle(ld, geo, p_next);
    G8Step nxt;
    if (more) load_step(nxt, ld, p_next);

    while (more) {                                  // the same for the whole grid
        const G8Step cur = nxt;
        // x of this step: 4 packets of BE bytes per row, de-interleaved, and their byte sums
        __syncthreads();                            // the previous step's reads of LDS are done
        for (int it = tid; it < kRows * 4; it += kThreads) {
            const int m = it >> 2, t = it & 3;
            const bool live = m < rows && cur.p0 + t < n_packets;
            const uint8_t* src = act.a + (m0 + m) * K + (cur.p0 + t) * BE;
            u32x4 v[BE / 16];
#pragma unroll
            for (int b = 0; b < BE / 16; ++b) {
                v[b] = u32x4{0u, 0u, 0u, 0u};
                if (live) {
                    if (act.aligned) {
                        v[b] = *reinterpret_cast<const u32x4*>(src + b * 16);
                    } else {
                        uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                        for (int j = 0; j < 16; ++j) d[j >> 2] |= static_cast<uint32_t>(src[b * 16 + j]) << ((j & 3) * 8);
                        v[b] = u32x4{d[0], d[1], d[2], d[3]};
                    }
                    v[b] = v[b] ^ ac.flip;
                }
            }
            int s = 0;
#pragma unroll
            for (int b = 0; b < BE / 16; ++b) {
                const uint32_t in[4] = {v[b].x, v[b].y, v[b].z, v[b].w};
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int pos = g8_lds_pos<BITS>(j);
                    w[pos >> 2] |= ((in[j >> 2] >> ((j & 3) * 8)) & 0xffu) << ((pos & 3) * 8);
                }
                *reinterpret_cast<u32x4*>(xs + m * kStride + t * BE + b * 16) = u32x4{w[0], w[1], w[2], w[3]};
                s += g8_sum_bytes(in[0]) + g8_sum_bytes(in[1]) + g8_sum_bytes(in[2]) + g8_sum_bytes(in[3]);
            }
            asum[t * kRows + m] = s;
        }
        __syncthreads();

        // the next step's codes and scales, in flight during this step's MFMAs
        g8_advance(ld, geo);
        more = g8_settle(ld, geo, p_next);
        if (more) load_step(nxt, ld, p_next);

        while (cur_w < cur.w) fold_chain();         // the chains before this step's, the empty ones too

        uint32_t r[4] = {cur.raw.x, cur.raw.y, cur.raw.z, cur.raw.w};
        transpose_over_rows(r);
#pragma unroll
        for (int t = 0; t < 4; t += PER) {
            if (cur.p0 + t < n_packets) {           // the same for the whole workgroup
                const unsigned char* xa = xs + nl * kStride + t * BE;
                i32x4 b;
                if constexpr (BITS == 2) {
                    const uint32_t v = r[t];
                    b = i32x4{static_cast<int>(v & 0x03030303u), static_cast<int>((v >> 2) & 0x03030303u),
                              static_cast<int>((v >> 4) & 0x03030303u), static_cast<int>((v >> 6) & 0x03030303u)};
                } else {
                    const uint32_t v = r[t], v2 = PAIR ? r[t + PER - 1] : 0u;
                    b = i32x4{static_cast<int>(v & 0x0F0F0F0Fu), static_cast<int>((v >> 4) & 0x0F0F0F0Fu),
                              static_cast<int>(v2 & 0x0F0F0F0Fu), static_cast<int>((v2 >> 4) & 0x0F0F0F0Fu)};
                }
                C = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b, C, 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < SUBS; ++rt) {
                    const unsigned char* xr = xa + rt * 16 * kStride;
                    i32x4 a = {0, 0, 0, 0};
                    if constexpr (BITS == 2) {
                        a = *reinterpret_cast<const i32x4*>(xr + q * 16);
                    } else {
                        const u32x2 lo = *reinterpret_cast<const u32x2*>(xr + q * 8);
                        a.x = static_cast<int>(lo.x);
                        a.y = static_cast<int>(lo.y);
                        if constexpr (PAIR) {
                            const u32x2 hi = *reinterpret_cast<const u32x2*>(xr + BE + q * 8);
                            a.z = static_cast<int>(hi.x);
                            a.w = static_cast<int>(hi.y);
                        }
                    }
                    P[rt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, P[rt], 0, 0, 0);
                    // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
                    A[rt] = A[rt] + *reinterpret_cast<const i32x4*>(asum + t * kRows + rt * 16 + q * 4);
                    if constexpr (PAIR) A[rt] = A[rt] + *reinterpret_cast<const i32x4*>(asum + (t + 1) * kRows + rt * 16 + q * 4);
                }
                pig += PER;
                if (pig == geo.ppg) {               // the group is complete: the same for the whole workgroup
                    const int32_t qz = cur.qz[t + PER - 1];
                    const float qs = cur.qs[t + PER - 1];
                    const bool far = qz < -kG8FastZero || qz > kG8FastZero;
                    const bool any_far = __ballot(far) != 0;
#pragma unroll
                    for (int rt = 0; rt < SUBS; ++rt) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int ae = A[rt][i] - gz;
                            float f;
                            if (!any_far) {
                                f = static_cast<float>(P[rt][i] - ac.z * C[i] - qz * ae);
                            } else {
                                f = static_cast<float>(static_cast<int64_t>(P[rt][i]) - static_cast<int64_t>(ac.z) * C[i] -
                                                       static_cast<int64_t>(qz) * ae);
                            }
                            acc[rt][i] = __fadd_rn(acc[rt][i], __fmul_rn(qs, f));
                        }
                        P[rt] = i32x4{0, 0, 0, 0};
                        A[rt] = i32x4{0, 0, 0, 0};
                    }
                    C = i32x4{0, 0, 0, 0};
                    pig = 0;
                }
            }
            __builtin_amdgcn_sched_barrier(0);      // one packet's LDS reads at a time
        }
    }
    while (cur_w < kG8Chains) fold_chain();

    const int64_t n = n0 + nl;
    if (n < N) {
        const float b = g8_bias_at(bias, bias_dtype, n);
#pragma unroll
        for (int rt = 0; rt < SUBS; ++rt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = rt * 16 + q * 4 + i;
                if (m < rows) {
                    const float v = __fadd_rn(__fmul_rn(sum[rt][i], ac.s_x), b);
                    const int64_t at = (m0 + m) * N + n;
                    if (y_dtype == LSQ_BF16) store_out<io_bf16, false>(y, at, v);
                    else if (y_dtype == LSQ_F16) store_out<io_f16, false>(y, at, v);
                    else store_out<io_f32, false>(y, at, v);
                }
            }
        }
    }
}

// the fused form's pre-pass: ws[i] = level(x[i]) - off as a byte, 16 elements per thread and turn
template <typename IO>
__global__ __launch_bounds__(kBlock) void qgemm_a8_levels_kernel(const void* __restrict__ x, int64_t n16, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, float qmin, float qmax, float tmin,
                                                                 float tmax, int off, uint8_t* __restrict__ ws) {
    const Range<float> r = Range<float>{qmin, qmax, tmin, tmax};
    const QParams<float> qp = make_qparams<float>(sanitize_scale_per_tensor<float>(scale[0]), shift[0], r);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n16; i += stride) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int a = static_cast<int>(level<float>(IO::load1(x, i * 16 + j), qp, r)) - off;
            w[j >> 2] |= static_cast<uint32_t>(a & 0xff) << ((j & 3) * 8);
        }
        *reinterpret_cast<u32x4*>(ws + i * 16) = u32x4{w[0], w[1], w[2], w[3]};
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launchers
// ------------------------------------------------------------------------------------------------
struct G8Plan {
    const char* unserved;           // NULL: served on the matrix cores; else why not
    bool pair;
    int waves, subs, lds, ks;
    int64_t col_tiles, grid;
    G8Geom geo;
};

constexpr int g8_lds_bytes(int bits, int subs) { return subs * 16 * (4 * (128 / bits) + kQRowPad) + 4 * subs * 16 * 4; }

inline G8Plan plan_g8(int64_t M, int64_t N, int64_t K, int64_t G, int bits) {
    G8Plan pl = {};
    const int64_t BE = 128 / bits;
    if (G % BE != 0) {
        pl.unserved = "group_size is not a multiple of the 128 / bits elements of one 16-byte code packet";
        return pl;
    }
    const int64_t ppg = G / BE;
    const int64_t span_p = ppg % 4 == 0 ? ppg : (ppg % 2 == 0 ? ppg * 2 : ppg * 4);     // lcm(ppg, 4)
    if (span_p * BE > kQChunk) {
        pl.unserved = "a span of lcm(group_size, 4 code packets) elements is beyond 4096";
        return pl;
    }
    const int64_t cus = device_info().cu_count;
    G8Geom& g = pl.geo;
    g.M = M;
    g.N = N;
    g.K = K;
    g.n_groups = K / G;
    g.n_packets = K / BE;
    g.G = static_cast<int>(G);
    g.ppg = static_cast<int>(ppg);
    g.ppg_shift = log2_exact(g.ppg);
    g.ppg_div = make_div(g.ppg);
    g.span_p = static_cast<int>(span_p);
    g.steps_per_span = g.span_p / 4;
    g.chunk_spans = static_cast<int>(kQChunk / (span_p * BE));
    g.chunk_p = static_cast<int64_t>(g.chunk_spans) * span_p;
    g.n_chunks = (g.n_packets + g.chunk_p - 1) / g.chunk_p;
    pl.pair = bits == 4 && g.ppg % 2 == 0;
    pl.subs = M <= 32 ? 2 : (M <= 64 ? 4 : kG8Sub);
    g.row_tiles = (M + pl.subs * 16 - 1) / (pl.subs * 16);
    const int64_t wide = (N + 16 * kG8Wide - 1) / (16 * kG8Wide);
    // 64-column tiles once they give every compute unit a tile; below that 16-column tiles, four times as many
    pl.waves = (wide <= INT64_MAX / g.row_tiles && g.row_tiles * wide < cus) ? 1 : kG8Wide;
    pl.col_tiles = (N + 16 * pl.waves - 1) / (16 * pl.waves);
    pl.grid = pl.col_tiles <= INT64_MAX / g.row_tiles ? g.row_tiles * pl.col_tiles : INT64_MAX;
    pl.ks = static_cast<int>(4 * BE);
    pl.lds = g8_lds_bytes(bits, pl.subs);
    return pl;
}

struct G8Weights {
    const void* codes;
    const void* qscale;
    const void* qzero;
    const void* bias;
    int bias_dtype;
};

template <int BITS, bool PAIR, int WAVES, int SUBS>
static hipError_t g8_launch(const G8Plan& pl, const G8Act& act, const G8Weights& w, void* y, int y_dtype, hipStream_t stream) {
    static_assert(g8_lds_bytes(BITS, SUBS) <= 64 * 1024, "the tile fits the LDS a kernel gets unasked");
    hipLaunchKernelGGL((qgemm_a8_kernel<BITS, PAIR, WAVES, SUBS>), dim3(static_cast<unsigned>(pl.grid)), dim3(WAVES * 64), pl.lds, stream,
                       act, static_cast<const uint8_t*>(w.codes), pl.geo, static_cast<const float*>(w.qscale),
                       static_cast<const int32_t*>(w.qzero), w.bias, w.bias_dtype, y, y_dtype);
    return hipGetLastError();
}

template <int BITS, bool PAIR, int WAVES>
static hipError_t g8_subs(const G8Plan& pl, const G8Act& act, const G8Weights& w, void* y, int y_dtype, hipStream_t stream) {
    if (pl.subs == 2) return g8_launch<BITS, PAIR, WAVES, 2>(pl, act, w, y, y_dtype, stream);
    if (pl.subs == 4) return g8_launch<BITS, PAIR, WAVES, 4>(pl, act, w, y, y_dtype, stream);
    return g8_launch<BITS, PAIR, WAVES, kG8Sub>(pl, act, w, y, y_dtype, stream);
}

template <int BITS, bool PAIR>
static hipError_t g8_waves(const G8Plan& pl, const G8Act& act, const G8Weights& w, void* y, int y_dtype, hipStream_t stream) {
    return pl.waves == 1 ? g8_subs<BITS, PAIR, 1>(pl, act, w, y, y_dtype, stream)
                         : g8_subs<BITS, PAIR, kG8Wide>(pl, act, w, y, y_dtype, stream);
}

static hipError_t g8_gemm(const G8Plan& pl, int bits, const G8Act& act, const G8Weights& w, void* y, int y_dtype, hipStream_t stream) {
    if (bits == 2) return g8_waves<2, false>(pl, act, w, y, y_dtype, stream);
    return pl.pair ? g8_waves<4, true>(pl, act, w, y, y_dtype, stream) : g8_waves<4, false>(pl, act, w, y, y_dtype, stream);
}

template <typename IO>
static hipError_t g8_levels(const void* x, int64_t n16, const G8Act& act, void* ws, hipStream_t stream) {
    const int64_t cus = device_info().cu_count;
    const int grid = static_cast<int>(std::min(std::max<int64_t>(1, (n16 + kBlock - 1) / kBlock), cus * 8));
    hipLaunchKernelGGL((qgemm_a8_levels_kernel<IO>), dim3(grid), dim3(kBlock), 0, stream, x, n16, act.scale, act.shift, act.qmin,
                       act.qmax, act.tmin, act.tmax, act.off, static_cast<uint8_t*>(ws));
    return hipGetLastError();
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_qgemm_a8.h: validation, dtype dispatch, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// the shape of a call: lsq_qdecode.hpp's check_shape with the GEMM's row rule
int check_g8_shape(int dtype, int64_t M, int64_t N, int64_t K, int64_t G, int bits, const char* what) {
    if (dtype == LSQ_F64) return fail(LSQ_EINVAL, "%s: float64 is not supported (the kernel computes in integers and float32)", what);
    if (dtype != LSQ_F32 && dtype != LSQ_BF16 && dtype != LSQ_F16) return fail(LSQ_EINVAL, "%s: unknown dtype code %d", what, dtype);
    if (bits != 4 && bits != 2) return fail(LSQ_EINVAL, "%s: bits must be 4 or 2, got %d", what, bits);
    const long long m = M, n = N, k = K, g = G;
    if (G <= 0) return fail(LSQ_EINVAL, "%s: group_size must be positive, got %lld", what, g);
    if (N < 0 || K < 0) return fail(LSQ_EINVAL, "%s: negative weight shape [%lld, %lld]", what, n, k);
    if (K % G != 0) return fail(LSQ_EINVAL, "%s: K = %lld is not a multiple of group_size %lld", what, k, g);
    if (G % (8 / bits) != 0)
        return fail(LSQ_EINVAL, "%s: group_size %lld is not a multiple of %d, the elements of one byte of %d-bit codes", what, g,
                    8 / bits, bits);
    if (M < 1) return fail(LSQ_EINVAL, "%s: M = %lld rows of x, at least 1 is needed", what, m);
    if (M > INT64_MAX / std::max<int64_t>(1, std::max(N, K)) / 4 || N > INT64_MAX / std::max<int64_t>(1, K))
        return fail(LSQ_EINVAL, "%s: M = %lld rows of x on a [%lld, %lld] weight are beyond 64-bit offsets", what, m, n, k);
    return LSQ_OK;
}

int check_g8_weights(const char* what, int y_dtype, const void* codes, const void* qscale, const void* qzero, const void* bias,
                     int bias_dtype, const void* y) {
    if (!codes || !qscale || !qzero || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (bias && bias_dtype != LSQ_F32 && bias_dtype != y_dtype)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of y's type, got dtype code %d", what, bias_dtype);
    if (!aligned_to(y, elem_bytes(y_dtype))) return fail(LSQ_EINVAL, "%s: x and y must be element-aligned", what);
    if (!aligned_to(qscale, 4) || !aligned_to(qzero, 4) || (bias && !aligned_to(bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: qscale, qzero and bias must be element-aligned", what);
    return LSQ_OK;
}

// the plan of a served call, or the refusal
int served_plan(const char* what, lsq::G8Plan& pl, int64_t M, int64_t N, int64_t K, int64_t G, int bits, const void* codes) {
    pl = lsq::plan_g8(M, N, K, G, bits);
    if (pl.unserved)
        return fail(LSQ_EINVAL, "%s: not served: %s (call the decode kernel %d rows at a time)", what, pl.unserved, LSQ_QLINEAR_A8_MAX_ROWS);
    if (!aligned_to(codes, 16))
        return fail(LSQ_EINVAL, "%s: not served: codes are not 16-byte aligned (call the decode kernel %d rows at a time)", what,
                    LSQ_QLINEAR_A8_MAX_ROWS);
    if (pl.grid > INT32_MAX)
        return fail(LSQ_EINVAL, "%s: %lld row tiles by %lld column tiles are beyond a 31-bit grid", what,
                    static_cast<long long>(pl.geo.row_tiles), static_cast<long long>(pl.col_tiles));
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_qgemm_a8_abi_version(void) { return LSQ_QGEMM_A8_ABI_VERSION; }

const char* lsq_qgemm_a8_last_error(void) { return g_last_error; }

int lsq_qgemm_a8_forward_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, const void* codes,
                                int64_t N, int64_t K, int64_t group_size, int bits, const void* qscale, const void* qzero,
                                const void* bias, int bias_dtype, void* y, int y_dtype, void* stream) {
    const char* what = "lsq_qgemm_a8_forward_levels";
    if (int rc = check_g8_shape(y_dtype, M, N, K, group_size, bits, what)) return rc;
    if (level_dtype != LSQ_A8_U8 && level_dtype != LSQ_A8_I8)
        return fail(LSQ_EINVAL, "%s: level_dtype must be LSQ_A8_U8 (0) or LSQ_A8_I8 (1), got %d", what, level_dtype);
    if (!x_levels || !s_x || !zx) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (int rc = check_g8_weights(what, y_dtype, codes, qscale, qzero, bias, bias_dtype, y)) return rc;
    if (!aligned_to(s_x, 4) || !aligned_to(zx, 4)) return fail(LSQ_EINVAL, "%s: s_x and zx must be element-aligned", what);
    if (N == 0) return LSQ_OK;
    lsq::G8Plan pl;
    if (int rc = served_plan(what, pl, M, N, K, group_size, bits, codes)) return rc;
    lsq::G8Act act{};
    act.a = static_cast<const uint8_t*>(x_levels);
    act.scale = static_cast<const float*>(s_x);
    act.zx = static_cast<const int32_t*>(zx);
    act.off = level_dtype == LSQ_A8_U8 ? 128 : 0;
    act.fused = 0;
    act.aligned = aligned_to(x_levels, 16) ? 1 : 0;
    const lsq::G8Weights w{codes, qscale, qzero, bias, bias_dtype};
    return hip_status(lsq::g8_gemm(pl, bits, act, w, y, y_dtype, static_cast<hipStream_t>(stream)), what);
}

int lsq_qgemm_a8_forward(int dtype, const void* x, int64_t M, const void* scale, const void* shift, int64_t quant_min,
                         int64_t quant_max, int64_t type_min, int64_t type_max, const void* codes, int64_t N, int64_t K,
                         int64_t group_size, int bits, const void* qscale, const void* qzero, const void* bias, int bias_dtype,
                         void* y, void* levels_ws, void* stream) {
    const char* what = "lsq_qgemm_a8_forward";
    if (int rc = check_g8_shape(dtype, M, N, K, group_size, bits, what)) return rc;
    const long long lo = std::min(quant_min, type_min), hi = std::max(quant_max, type_max);
    if (quant_min > quant_max || type_min > type_max || !((lo >= 0 && hi <= 255) || (lo >= -128 && hi <= 127)))
        return fail(LSQ_EINVAL, "%s: [quant_min, quant_max] = [%lld, %lld] and [type_min, type_max] = [%lld, %lld] must lie within "
                    "0..255 or within -128..127", what, static_cast<long long>(quant_min), static_cast<long long>(quant_max),
                    static_cast<long long>(type_min), static_cast<long long>(type_max));
    if (!x || !scale || !shift) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (int rc = check_g8_weights(what, dtype, codes, qscale, qzero, bias, bias_dtype, y)) return rc;
    if (!aligned_to(x, elem_bytes(dtype))) return fail(LSQ_EINVAL, "%s: x and y must be element-aligned", what);
    if (!aligned_to(scale, 4) || !aligned_to(shift, 4))
        return fail(LSQ_EINVAL, "%s: scale and shift must be element-aligned", what);
    if (N == 0) return LSQ_OK;
    lsq::G8Plan pl;
    if (int rc = served_plan(what, pl, M, N, K, group_size, bits, codes)) return rc;
    if (!levels_ws || !aligned_to(levels_ws, 16))
        return fail(LSQ_EINVAL, "%s: levels_ws must be a 16-byte aligned device buffer of M * K bytes", what);
    lsq::G8Act act{};
    act.a = static_cast<const uint8_t*>(levels_ws);
    act.scale = static_cast<const float*>(scale);
    act.shift = static_cast<const float*>(shift);
    act.qmin = static_cast<float>(quant_min);
    act.qmax = static_cast<float>(quant_max);
    act.tmin = static_cast<float>(type_min);
    act.tmax = static_cast<float>(type_max);
    act.off = hi > 127 ? 128 : 0;
    act.fused = 1;
    act.aligned = 1;
    const lsq::G8Weights w{codes, qscale, qzero, bias, bias_dtype};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n16 = M * K / 16;                 // exact: K is a multiple of one code packet's 32 or 64 elements
    hipError_t e = hipSuccess;
    switch (dtype) {
        case LSQ_BF16: e = lsq::g8_levels<lsq::io_bf16>(x, n16, act, levels_ws, s); break;
        case LSQ_F16: e = lsq::g8_levels<lsq::io_f16>(x, n16, act, levels_ws, s); break;
        default: e = lsq::g8_levels<lsq::io_f32>(x, n16, act, levels_ws, s); break;
    }
    if (e != hipSuccess) return hip_status(e, what);
    return hip_status(lsq::g8_gemm(pl, bits, act, w, y, dtype, s), what);
}

int lsq_qgemm_a8_plan(int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int32_t* out8) {
    const char* what = "lsq_qgemm_a8_plan";
    if (int rc = check_g8_shape(LSQ_F32, M, N, K, group_size, bits, what)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    const lsq::G8Plan pl = lsq::plan_g8(M, N, K, group_size, bits);
    if (pl.unserved) return LSQ_OK;
    if (pl.grid > INT32_MAX)
        return fail(LSQ_EINVAL, "%s: %lld row tiles by %lld column tiles are beyond a 31-bit grid", what,
                    static_cast<long long>(pl.geo.row_tiles), static_cast<long long>(pl.col_tiles));
    out8[0] = 1;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.waves * 64;
    out8[3] = pl.subs * 16;
    out8[4] = 16 * pl.waves;
    out8[5] = pl.lds;
    out8[6] = pl.ks;
    out8[7] = pl.subs;
    return LSQ_OK;
}

}  // extern "C"
