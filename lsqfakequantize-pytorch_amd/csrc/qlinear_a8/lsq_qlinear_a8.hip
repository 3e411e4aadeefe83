// lsq_qlinear_a8.hip -- 8-bit activation levels times packed 4- / 2-bit group-wise weight codes for up to 16 rows of x on
// gfx950 (include/lsq_hip_qlinear_a8.h, which states the arithmetic contract; the weight format is include/lsq_hip_pack.h's):
// the kernels and the C ABI of liblsq_hip_qlinear_a8.so.
//
//     I[m, n, g] = sum_{k in g} (lx[m, k] - zx) * (code[n, k] - qzero[n, g]),   y[m, n] = s_x * sum_g qscale[n, g] * float(I)
//
// Both kernels work on the BYTE OPERAND a[m, k] = lx[m, k] - off with off = 128 for a 0..255 range and 0 for a -128..127
// range, which is an int8 for every legal level, and on z = zx - off.  With c = code, q = qzero and G elements per group
//     I = sum a c  -  z sum c  -  q (sum a - G z)
// in integers: nothing cancels, and no property of the quantizer decides anything -- zx is read in the kernel.  The levels
// come from memory (XLevels) or are formed from a floating x with lsq_math.hpp's make_qparams / level() while x is read
// (XFloat): everything after that is the same code, so the two entry forms agree bit for bit.
//
// lsq_qdecode.hpp has the design both decode linears share -- tile ownership, K split by wave, the transpose, the order of
// the sum -- and its pieces; particular to 8-bit levels:
//  * MATRIX-CORE form (G a multiple of the BE = 128 / bits elements of one 16-byte code packet, lcm(G, 4 packets) <= 4096
//    elements, codes 16-byte aligned).  K is cut into SPANS of lcm(G, 4 BE) elements -- whole groups and whole load steps --
//    and span s of a chunk belongs to wave s % 16, so a group's integer sum stays in one wave.  Two load steps are in flight,
//    the first two issued before x is staged; after the transpose one MFMA reads one packet (or two adjacent ones of one
//    group).  The B operand of v_mfma_i32_16x16x64_i8 is the codes as the unsigned nibbles (crumbs) they are: a mask and a
//    shift per dword.  An integer sum has no order, so x is laid out in LDS in that de-interleaved order and the A operand
//    is one ds_read of 8 or 16 bytes.  A second MFMA with an all-ones A operand gives sum c.  x is staged once per workgroup
//    and chunk (at most 4096 k) as the bytes a[m, k]; sum a - G z per (row, group) is formed from the staged bytes.  When a
//    group ends, I is formed (32-bit when every |qzero| of the wave's columns is at most 256, else 64-bit), converted with
//    one rounding and multiplied by qscale.  After the sum over the waves the result is multiplied by s_x, the bias is
//    added in fp32, and it is rounded once.
//  * GENERIC form (every other legal format): the lanes of a segment of the wave share one group, multiply-add in 64-bit
//    integers and sum with a butterfly; the segments' fp32 sums meet in a second butterfly.
#include "../qlinear/lsq_qdecode.hpp"

namespace lsq {

constexpr int kAMaxLds = kQRedBytes + LSQ_QLINEAR_A8_MAX_ROWS * (kQChunk + kQRowPad) + LSQ_QLINEAR_A8_MAX_ROWS * (kQChunk / 32) * 4;
constexpr int kAFastZero = 256;                     // |qzero| up to here: I fits 32 bits for every G of the matrix-core form

// ------------------------------------------------------------------------------------------------
// the activation: where a[m, k] comes from
// ------------------------------------------------------------------------------------------------
struct A8Act {              // kernel argument
    const void* x;          // levels (bytes) or floating x
    const float* scale;     // levels form: s_x; fused form: the quantizer's scale
    const float* shift;     // fused form
    const int32_t* zx;      // levels form
    float qmin, qmax, tmin, tmax;   // fused form
    int off;                // 128: levels in 0..255; 0: levels in -128..127
};

struct A8Const {            // what a thread derives from A8Act once
    QParams<float> q;
    Range<float> r;
    int off, z;             // z = zx - off
    float s_x;
};

struct XLevels {
    __device__ static __forceinline__ A8Const constants(const A8Act& a) {
        A8Const c;
        c.q = QParams<float>{1.0f, 1.0f, 0.0f};
        c.r = Range<float>{0.0f, 0.0f, 0.0f, 0.0f};
        c.off = a.off;
        c.z = a.zx[0] - a.off;
        c.s_x = a.scale[0];
        return c;
    }
    // byte ^ 0x80 read as int8 is byte - 128
    __device__ static __forceinline__ int get1(const A8Act& a, const A8Const& c, int64_t i) {
        return static_cast<int>(static_cast<int8_t>(static_cast<const uint8_t*>(a.x)[i] ^ static_cast<uint8_t>(c.off)));
    }
};

template <typename IO>
struct XFloat {
    __device__ static __forceinline__ A8Const constants(const A8Act& a) {
        A8Const c;
        c.r = Range<float>{a.qmin, a.qmax, a.tmin, a.tmax};
        c.q = make_qparams<float>(sanitize_scale_per_tensor<float>(a.scale[0]), a.shift[0], c.r);
        c.off = a.off;
        c.z = static_cast<int>(c.q.zp) - a.off;
        c.s_x = c.q.s;
        return c;
    }
    __device__ static __forceinline__ int get1(const A8Act& a, const A8Const& c, int64_t i) {
        return static_cast<int>(level<float>(IO::load1(a.x, i), c.q, c.r)) - c.off;
    }
};

// ------------------------------------------------------------------------------------------------
// matrix-core form
// ------------------------------------------------------------------------------------------------
struct A8Geom {             // kernel argument: the cut of K (host: plan_a8)
    int64_t N, K, n_groups, n_packets;
    int G;
    int ppg;                // 16-byte code packets per group
    int ppg_shift;          // log2(ppg) or -1
    DivU64 ppg_div;
    int span_p;             // packets per span: lcm(ppg, 4)
    int steps_per_span;     // span_p / 4
    int groups_per_span;    // span_p / ppg
    int chunk_spans;        // spans per chunk of x
    int chunk_k;            // elements of K per chunk
    int row_stride;         // bytes between rows of x in LDS
    int gstride;            // groups per row of the LDS table of sum a - G z
};

// where element j of a block of 16 consecutive k lies in LDS: the order in which the masks and shifts below hand the codes
// of a dword to the MFMA.  4 bits (8 codes per dword): the even codes, then the odd ones; 2 bits (16 codes per dword): codes
// 0, 4, 8, 12, then 1, 5, 9, 13, ...
template <int BITS>
__device__ __forceinline__ constexpr int a8_lds_pos(int j) {
    return BITS == 4 ? (j & 8) + (j & 1) * 4 + ((j & 7) >> 1) : (j & 3) * 4 + (j >> 2);
}

struct A8Cursor {           // a wave's walk over its load steps of one chunk
    int span, l;
};

struct A8Step {             // one load step in flight: 4 packets of each of the 16 rows
    u32x4 raw;
    float qs[4];
    int32_t qz[4];
    int64_t p0;
    bool valid;
};

__device__ __forceinline__ int a8_sum_bytes(uint32_t w) {
    return static_cast<int>(static_cast<int8_t>(w)) + static_cast<int>(static_cast<int8_t>(w >> 8)) +
           static_cast<int>(static_cast<int8_t>(w >> 16)) + (static_cast<int>(w) >> 24);
}

template <typename XS, typename OUT, int BITS, bool PAIR>
__global__ __launch_bounds__(kQBlock) void qlinear_a8_mfma_kernel(A8Act act, int M, const uint8_t* __restrict__ codes, A8Geom geo,
                                                                 const float* __restrict__ qscale, const int32_t* __restrict__ qzero,
                                                                 const void* __restrict__ bias, int bias_f32, void* __restrict__ y) {
    constexpr int D = 32 / BITS;                    // elements per dword
    constexpr int BE = 4 * D;                       // elements per 16-byte packet
    static_assert(!PAIR || BITS == 4, "two packets per MFMA only at 4 bits: a 2-bit packet is 64 elements already");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);
    unsigned char* xs = smem + kQRedBytes;
    int32_t* aeff = reinterpret_cast<int32_t*>(xs + M * geo.row_stride);       // [M][gstride]: sum a - G z

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const A8Const ac = XS::constants(act);
    const int64_t K = geo.K, N = geo.N, n_packets = geo.n_packets;
    const int64_t row_bytes = n_packets * 16;
    const int64_t n_chunks = (K + geo.chunk_k - 1) / geo.chunk_k;
    const int64_t chunk_p = static_cast<int64_t>(geo.chunk_spans) * geo.span_p;
    const int64_t tiles = (N + kQTile - 1) / kQTile;
    const int64_t first_tile = static_cast<int64_t>(blockIdx.x);
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};

    for (int64_t tile = first_tile; tile < tiles; tile += static_cast<int64_t>(gridDim.x)) {
        const int64_t row = std::min<int64_t>(tile * kQTile + nl, N - 1);          // a clamped row computes a value nobody stores
        const uint8_t* __restrict__ wrow = codes + row * row_bytes;
        const float* __restrict__ qs_row = qscale + row * geo.n_groups;
        const int32_t* __restrict__ qz_row = qzero + row * geo.n_groups;

        // the load step the cursor points at, and the cursor one step further
        auto load_step = [&](A8Step& s, A8Cursor& cur, int64_t chunk_p0) {
            s.p0 = chunk_p0 + static_cast<int64_t>(cur.span) * geo.span_p + cur.l * 4;
            s.valid = cur.span < geo.chunk_spans && s.p0 < n_packets;
            s.raw = u32x4{0u, 0u, 0u, 0u};
            if (s.valid) {
                if (s.p0 + q < n_packets) s.raw = load_code_packet(wrow, s.p0 + q);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    load_packet_scale(qs_row, qz_row, s.p0 + t, n_packets, geo.ppg_shift, geo.ppg_div, s.qs[t], s.qz[t]);
            }
            if (++cur.l == geo.steps_per_span) {
                cur.l = 0;
                cur.span += kQWaves;
            }
        };

        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int64_t c = 0; c < n_chunks; ++c) {
            const int64_t kc0 = c * geo.chunk_k;
            const int64_t chunk_p0 = c * chunk_p;
            A8Cursor ld = {wave, 0};
            A8Step s0, s1;
            load_step(s0, ld, chunk_p0);
            load_step(s1, ld, chunk_p0);
            if (n_chunks > 1 || tile == first_tile) {       // x stays in LDS across tiles when one chunk holds it
                __syncthreads();
                const int kc_len = static_cast<int>(std::min<int64_t>(geo.chunk_k, K - kc0));
                const int bpr = kc_len / 16;                // blocks of 16 k per row; exact, BE % 16 == 0
                for (int it = tid; it < M * bpr; it += kQBlock) {
                    const int m = it / bpr, b = it - m * bpr;
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int a = XS::get1(act, ac, static_cast<int64_t>(m) * K + kc0 + b * 16 + j);
                        const int pos = a8_lds_pos<BITS>(j);
                        w[pos >> 2] |= static_cast<uint32_t>(a & 0xff) << ((pos & 3) * 8);
                    }
                    *reinterpret_cast<u32x4*>(xs + m * geo.row_stride + b * 16) = u32x4{w[0], w[1], w[2], w[3]};
                }
                __syncthreads();
                const int ng = kc_len / geo.G;              // groups of this chunk; exact
                for (int it = tid; it < M * ng; it += kQBlock) {
                    const int m = it / ng, g = it - m * ng;
                    const unsigned char* src = xs + m * geo.row_stride + g * geo.G;
                    int sum = 0;
                    for (int b = 0; b < geo.G; b += 16) {
                        const u32x4 v = *reinterpret_cast<const u32x4*>(src + b);
                        sum += a8_sum_bytes(v.x) + a8_sum_bytes(v.y) + a8_sum_bytes(v.z) + a8_sum_bytes(v.w);
                    }
                    aeff[m * geo.gstride + g] = sum - geo.G * ac.z;
                }
                __syncthreads();
            }

            // the wave's steps of this chunk: spans wave, wave + 16, ...; a span starts a group and ends one
            i32x4 P = {0, 0, 0, 0}, C = {0, 0, 0, 0};
            int pig = 0;                                    // packets of the current group already summed
            int g_local = 0;                                // the current group's index in the chunk
            A8Cursor cp = {wave, 0};
            auto compute_step = [&](const A8Step& s) {
                if (cp.l == 0) {
                    g_local = cp.span * geo.groups_per_span;
                    pig = 0;
                }
                uint32_t r[4] = {s.raw.x, s.raw.y, s.raw.z, s.raw.w};
                transpose_over_rows(r);
                constexpr int PER = PAIR ? 2 : 1;           // packets per MFMA
#pragma unroll
                for (int t = 0; t < 4; t += PER) {
                    if (s.p0 + t >= n_packets) continue;    // the same for the whole wave
                    const int koff = static_cast<int>((s.p0 + t) * BE - kc0);      // this packet's first element in the chunk
                    const unsigned char* xa = xs + nl * geo.row_stride + koff;
                    i32x4 a = {0, 0, 0, 0}, b;
                    if constexpr (BITS == 2) {
                        if (nl < M) a = *reinterpret_cast<const i32x4*>(xa + q * 16);
                        const uint32_t v = r[t];
                        b = i32x4{static_cast<int>(v & 0x03030303u), static_cast<int>((v >> 2) & 0x03030303u),
                                  static_cast<int>((v >> 4) & 0x03030303u), static_cast<int>((v >> 6) & 0x03030303u)};
                    } else {
                        if (nl < M) {
                            const u32x2 lo = *reinterpret_cast<const u32x2*>(xa + q * 8);
                            a.x = static_cast<int>(lo.x);
                            a.y = static_cast<int>(lo.y);
                            if constexpr (PAIR) {
                                const u32x2 hi = *reinterpret_cast<const u32x2*>(xa + BE + q * 8);
                                a.z = static_cast<int>(hi.x);
                                a.w = static_cast<int>(hi.y);
                            }
                        }
                        const uint32_t v = r[t], v2 = PAIR ? r[t + PER - 1] : 0u;
                        b = i32x4{static_cast<int>(v & 0x0F0F0F0Fu), static_cast<int>((v >> 4) & 0x0F0F0F0Fu),
                                  static_cast<int>(v2 & 0x0F0F0F0Fu), static_cast<int>((v2 >> 4) & 0x0F0F0F0Fu)};
                    }
                    P = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, P, 0, 0, 0);
                    C = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b, C, 0, 0, 0);
                    pig += PER;
                    if (pig == geo.ppg) {                   // the group is complete: the same for the whole wave
                        const int32_t qz = s.qz[t + PER - 1];
                        const float qs = s.qs[t + PER - 1];
                        const bool far = qz < -kAFastZero || qz > kAFastZero;
                        const bool any_far = __ballot(far) != 0;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int m = q * 4 + i;        // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
                            const int ae = m < M ? aeff[m * geo.gstride + g_local] : 0;
                            float f;
                            if (!any_far) {
                                f = static_cast<float>(P[i] - ac.z * C[i] - qz * ae);
                            } else {
                                f = static_cast<float>(static_cast<int64_t>(P[i]) - static_cast<int64_t>(ac.z) * C[i] -
                                                       static_cast<int64_t>(qz) * ae);
                            }
                            acc[i] = acc[i] + qs * f;
                        }
                        P = i32x4{0, 0, 0, 0};
                        C = i32x4{0, 0, 0, 0};
                        pig = 0;
                        ++g_local;
                    }
                }
                if (++cp.l == geo.steps_per_span) {
                    cp.l = 0;
                    cp.span += kQWaves;
                }
            };
            while (s0.valid) {                              // the same for the whole wave
                compute_step(s0);
                load_step(s0, ld, chunk_p0);
                if (!s1.valid) break;
                compute_step(s1);
                load_step(s1, ld, chunk_p0);
            }
        }
        // the waves' tiles, summed in wave order
        *reinterpret_cast<f32x4*>(red + (wave * 64 + lane) * 4) = acc;
        __syncthreads();
        if (tid < 256) {
            const int l = tid & 63, reg = tid >> 6;
            float sum = 0.0f;
#pragma unroll
            for (int w = 0; w < kQWaves; ++w) sum = sum + red[(w * 64 + l) * 4 + reg];
            const int64_t n = tile * kQTile + (l & 15);
            const int m = (l >> 4) * 4 + reg;
            if (m < M && n < N) store_out<OUT, false>(y, static_cast<int64_t>(m) * N + n, sum * ac.s_x + bias_at<OUT>(bias, bias_f32, n));
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// generic form
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t a8_shfl_xor_i64(int64_t v, int mask) {
    int lo = static_cast<int>(static_cast<uint64_t>(v) & 0xffffffffu), hi = static_cast<int>(static_cast<uint64_t>(v) >> 32);
    lo = __shfl_xor(lo, mask, 64);
    hi = __shfl_xor(hi, mask, 64);
    return static_cast<int64_t>((static_cast<uint64_t>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo));
}

// bytes_per_group: code bytes of one group; seg_shift: log2 of the lanes that share a group (the smallest power of two that
// holds bytes_per_group, at most 64)
template <typename XS, typename OUT, int BITS>
__global__ __launch_bounds__(kBlock) void qlinear_a8_generic_kernel(A8Act act, int M, const uint8_t* __restrict__ codes, int64_t N,
                                                                   int64_t K, int64_t n_groups, int64_t bytes_per_group, int seg_shift,
                                                                   const float* __restrict__ qscale, const int32_t* __restrict__ qzero,
                                                                   const void* __restrict__ bias, int bias_f32, void* __restrict__ y) {
    constexpr int PB = 8 / BITS;
    constexpr int R = kQGenericRowsAtOnce;
    constexpr uint32_t kMask = (1u << BITS) - 1u;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int seg_lanes = 1 << seg_shift, seg = lane >> seg_shift, sl = lane & (seg_lanes - 1);
    const int64_t groups_at_once = 64 >> seg_shift;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    const int64_t row_bytes = K / PB;
    const A8Const ac = XS::constants(act);
    for (int64_t n = wave; n < N; n += waves) {
        const uint8_t* __restrict__ wrow = codes + n * row_bytes;
        for (int m0 = 0; m0 < M; m0 += R) {
            float acc[R];
#pragma unroll
            for (int i = 0; i < R; ++i) acc[i] = 0.0f;
            for (int64_t g0 = 0; g0 < n_groups; g0 += groups_at_once) {
                const int64_t g = g0 + seg;
                const bool active = g < n_groups;
                const float qs = active ? qscale[n * n_groups + g] : 0.0f;
                const int64_t qz = active ? qzero[n * n_groups + g] : 0;
                int64_t I[R];
#pragma unroll
                for (int i = 0; i < R; ++i) I[i] = 0;
                if (active) {
                    for (int64_t b = sl; b < bytes_per_group; b += seg_lanes) {
                        const int64_t byte_at = g * bytes_per_group + b;
                        const uint32_t byte = wrow[byte_at];
#pragma unroll
                        for (int j = 0; j < PB; ++j) {
                            const int64_t cz = static_cast<int64_t>((byte >> (j * BITS)) & kMask) - qz;
                            const int64_t k = byte_at * PB + j;
#pragma unroll
                            for (int i = 0; i < R; ++i)
                                if (m0 + i < M)
                                    I[i] += static_cast<int64_t>(XS::get1(act, ac, static_cast<int64_t>(m0 + i) * K + k) - ac.z) * cz;
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    for (int s = seg_lanes >> 1; s >= 1; s >>= 1) I[i] += a8_shfl_xor_i64(I[i], s);      // integers: any order
                    acc[i] = acc[i] + qs * static_cast<float>(I[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                for (int s = seg_lanes; s <= 32; s <<= 1) acc[i] = acc[i] + __shfl_xor(acc[i], s, 64);     // the segments' sums
                if (lane == 0 && m0 + i < M)
                    store_out<OUT, false>(y, static_cast<int64_t>(m0 + i) * N + n, acc[i] * ac.s_x + bias_at<OUT>(bias, bias_f32, n));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launchers
// ------------------------------------------------------------------------------------------------
struct A8Plan {
    bool mfma, pair;
    int grid, block, lds, waves, cols;
    A8Geom geo;
    int64_t bytes_per_group;
    int seg_shift;
};

inline A8Plan plan_a8(int64_t M, int64_t N, int64_t K, int64_t G, int bits, bool aligned) {
    A8Plan pl{};
    const int64_t cus = device_info().cu_count;
    const int64_t BE = 128 / bits;
    int64_t span_p = 0;
    if (G % BE == 0) {
        const int64_t ppg = G / BE;
        span_p = ppg % 4 == 0 ? ppg : (ppg % 2 == 0 ? ppg * 2 : ppg * 4);      // lcm(ppg, 4)
    }
    pl.mfma = aligned && span_p > 0 && span_p * BE <= kQChunk;
    if (pl.mfma) {
        A8Geom& g = pl.geo;
        g.N = N;
        g.K = K;
        g.n_groups = K / G;
        g.n_packets = K / BE;
        g.G = static_cast<int>(G);
        g.ppg = static_cast<int>(G / BE);
        g.ppg_shift = log2_exact(g.ppg);
        g.ppg_div = make_div(g.ppg);
        g.span_p = static_cast<int>(span_p);
        g.steps_per_span = g.span_p / 4;
        g.groups_per_span = g.span_p / g.ppg;
        g.chunk_spans = static_cast<int>(kQChunk / (span_p * BE));
        g.chunk_k = static_cast<int>(g.chunk_spans * span_p * BE);
        const int64_t held = std::max<int64_t>(BE, std::min<int64_t>(g.chunk_k, K));       // elements of one row in LDS
        g.row_stride = static_cast<int>(held) + kQRowPad;
        g.gstride = static_cast<int>(std::max<int64_t>(1, held / G));
        pl.pair = bits == 4 && g.ppg % 2 == 0;
        pl.block = kQBlock;
        pl.lds = kQRedBytes + static_cast<int>(M) * g.row_stride + static_cast<int>(M) * g.gstride * 4;
        pl.waves = kQWaves;
        pl.cols = kQTile;
        pl.grid = mfma_grid(N, cus);
    } else {
        pl.block = kBlock;
        pl.lds = 0;
        pl.waves = 1;
        pl.cols = 1;
        pl.bytes_per_group = G / (8 / bits);
        pl.seg_shift = 0;
        while (pl.seg_shift < 6 && (int64_t{1} << pl.seg_shift) < pl.bytes_per_group) ++pl.seg_shift;
        pl.grid = generic_grid(N, cus);
    }
    return pl;
}

struct A8Weights {
    const void* codes;
    const void* qscale;
    const void* qzero;
    const void* bias;
    int bias_f32;
};

template <typename XS, typename OUT, int BITS, bool PAIR>
static hipError_t a8_launch_mfma(const A8Plan& pl, const A8Act& act, int64_t M, const A8Weights& w, void* y, hipStream_t stream) {
    static LdsOnce once;
    if (const hipError_t e = allow_lds(once, reinterpret_cast<const void*>(&qlinear_a8_mfma_kernel<XS, OUT, BITS, PAIR>), kAMaxLds))
        return e;
    hipLaunchKernelGGL((qlinear_a8_mfma_kernel<XS, OUT, BITS, PAIR>), dim3(pl.grid), dim3(pl.block), pl.lds, stream, act,
                       static_cast<int>(M), static_cast<const uint8_t*>(w.codes), pl.geo, static_cast<const float*>(w.qscale),
                       static_cast<const int32_t*>(w.qzero), w.bias, w.bias_f32, y);
    return hipGetLastError();
}

template <typename XS, typename OUT>
static hipError_t a8_launch(const A8Plan& pl, const A8Act& act, int64_t M, const A8Weights& w, int64_t N, int64_t K, int64_t G,
                            int bits, void* y, hipStream_t stream) {
    if (pl.mfma) {
        if (bits == 2) return a8_launch_mfma<XS, OUT, 2, false>(pl, act, M, w, y, stream);
        return pl.pair ? a8_launch_mfma<XS, OUT, 4, true>(pl, act, M, w, y, stream)
                       : a8_launch_mfma<XS, OUT, 4, false>(pl, act, M, w, y, stream);
    }
    if (bits == 4) {
        hipLaunchKernelGGL((qlinear_a8_generic_kernel<XS, OUT, 4>), dim3(pl.grid), dim3(pl.block), 0, stream, act, static_cast<int>(M),
                           static_cast<const uint8_t*>(w.codes), N, K, K / G, pl.bytes_per_group, pl.seg_shift,
                           static_cast<const float*>(w.qscale), static_cast<const int32_t*>(w.qzero), w.bias, w.bias_f32, y);
    } else {
        hipLaunchKernelGGL((qlinear_a8_generic_kernel<XS, OUT, 2>), dim3(pl.grid), dim3(pl.block), 0, stream, act, static_cast<int>(M),
                           static_cast<const uint8_t*>(w.codes), N, K, K / G, pl.bytes_per_group, pl.seg_shift,
                           static_cast<const float*>(w.qscale), static_cast<const int32_t*>(w.qzero), w.bias, w.bias_f32, y);
    }
    return hipGetLastError();
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_qlinear_a8.h: validation, dtype dispatch, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

int check_shape(int dtype, int64_t M, int64_t N, int64_t K, int64_t G, int bits, const char* what) {
    return check_shape(dtype, M, N, K, G, bits, what, "the kernel computes in integers and float32",
                       "dequantize the levels and call the prefill route beyond that");
}

int check_weights(const char* what, int y_dtype, const void* codes, const void* qscale, const void* qzero, const void* bias,
                  int bias_dtype, const void* y) {
    if (!codes || !qscale || !qzero || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (bias && bias_dtype != LSQ_F32 && bias_dtype != y_dtype)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of y's type, got dtype code %d", what, bias_dtype);
    if (!aligned_to(y, elem_bytes(y_dtype))) return fail(LSQ_EINVAL, "%s: x and y must be element-aligned", what);
    if (!aligned_to(qscale, 4) || !aligned_to(qzero, 4) || (bias && !aligned_to(bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: qscale, qzero and bias must be element-aligned", what);
    return LSQ_OK;
}

template <typename XS>
hipError_t launch_for_output(int y_dtype, const lsq::A8Plan& pl, const lsq::A8Act& act, int64_t M, const lsq::A8Weights& w, int64_t N,
                             int64_t K, int64_t G, int bits, void* y, hipStream_t s) {
    switch (y_dtype) {
        case LSQ_BF16: return lsq::a8_launch<XS, lsq::io_bf16>(pl, act, M, w, N, K, G, bits, y, s);
        case LSQ_F16: return lsq::a8_launch<XS, lsq::io_f16>(pl, act, M, w, N, K, G, bits, y, s);
        default: return lsq::a8_launch<XS, lsq::io_f32>(pl, act, M, w, N, K, G, bits, y, s);
    }
}

}  // namespace

extern "C" {

int lsq_qlinear_a8_abi_version(void) { return LSQ_QLINEAR_A8_ABI_VERSION; }

const char* lsq_qlinear_a8_last_error(void) { return g_last_error; }

int lsq_qlinear_a8_forward_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, const void* codes,
                                  int64_t N, int64_t K, int64_t group_size, int bits, const void* qscale, const void* qzero,
                                  const void* bias, int bias_dtype, void* y, int y_dtype, void* stream) {
    const char* what = "lsq_qlinear_a8_forward_levels";
    if (int rc = check_shape(y_dtype, M, N, K, group_size, bits, what)) return rc;
    if (level_dtype != LSQ_A8_U8 && level_dtype != LSQ_A8_I8)
        return fail(LSQ_EINVAL, "%s: level_dtype must be LSQ_A8_U8 (0) or LSQ_A8_I8 (1), got %d", what, level_dtype);
    if (!x_levels || !s_x || !zx) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (int rc = check_weights(what, y_dtype, codes, qscale, qzero, bias, bias_dtype, y)) return rc;
    if (!aligned_to(s_x, 4) || !aligned_to(zx, 4)) return fail(LSQ_EINVAL, "%s: s_x and zx must be element-aligned", what);
    if (N == 0) return LSQ_OK;
    const lsq::A8Plan pl = lsq::plan_a8(M, N, K, group_size, bits, aligned_to(codes, 16));
    lsq::A8Act act{};
    act.x = x_levels;
    act.scale = static_cast<const float*>(s_x);
    act.zx = static_cast<const int32_t*>(zx);
    act.off = level_dtype == LSQ_A8_U8 ? 128 : 0;
    const lsq::A8Weights w{codes, qscale, qzero, bias, bias_dtype == LSQ_F32 ? 1 : 0};
    return hip_status(launch_for_output<lsq::XLevels>(y_dtype, pl, act, M, w, N, K, group_size, bits, y, static_cast<hipStream_t>(stream)),
                      what);
}

int lsq_qlinear_a8_forward(int dtype, const void* x, int64_t M, const void* scale, const void* shift, int64_t quant_min,
                           int64_t quant_max, int64_t type_min, int64_t type_max, const void* codes, int64_t N, int64_t K,
                           int64_t group_size, int bits, const void* qscale, const void* qzero, const void* bias, int bias_dtype,
                           void* y, void* stream) {
    const char* what = "lsq_qlinear_a8_forward";
    if (int rc = check_shape(dtype, M, N, K, group_size, bits, what)) return rc;
    const long long lo = std::min(quant_min, type_min), hi = std::max(quant_max, type_max);
    if (quant_min > quant_max || type_min > type_max || !((lo >= 0 && hi <= 255) || (lo >= -128 && hi <= 127)))
        return fail(LSQ_EINVAL, "%s: [quant_min, quant_max] = [%lld, %lld] and [type_min, type_max] = [%lld, %lld] must lie within "
                    "0..255 or within -128..127", what, static_cast<long long>(quant_min), static_cast<long long>(quant_max),
                    static_cast<long long>(type_min), static_cast<long long>(type_max));
    if (!x || !scale || !shift) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (int rc = check_weights(what, dtype, codes, qscale, qzero, bias, bias_dtype, y)) return rc;
    if (!aligned_to(x, elem_bytes(dtype))) return fail(LSQ_EINVAL, "%s: x and y must be element-aligned", what);
    if (!aligned_to(scale, 4) || !aligned_to(shift, 4))
        return fail(LSQ_EINVAL, "%s: scale and shift must be element-aligned", what);
    if (N == 0) return LSQ_OK;
    const lsq::A8Plan pl = lsq::plan_a8(M, N, K, group_size, bits, aligned_to(codes, 16));
    lsq::A8Act act{};
    act.x = x;
    act.scale = static_cast<const float*>(scale);
    act.shift = static_cast<const float*>(shift);
    act.qmin = static_cast<float>(quant_min);
    act.qmax = static_cast<float>(quant_max);
    act.tmin = static_cast<float>(type_min);
    act.tmax = static_cast<float>(type_max);
    act.off = hi > 127 ? 128 : 0;
    const lsq::A8Weights w{codes, qscale, qzero, bias, bias_dtype == LSQ_F32 ? 1 : 0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    switch (dtype) {
        case LSQ_BF16: e = lsq::a8_launch<lsq::XFloat<lsq::io_bf16>, lsq::io_bf16>(pl, act, M, w, N, K, group_size, bits, y, s); break;
        case LSQ_F16: e = lsq::a8_launch<lsq::XFloat<lsq::io_f16>, lsq::io_f16>(pl, act, M, w, N, K, group_size, bits, y, s); break;
        default: e = lsq::a8_launch<lsq::XFloat<lsq::io_f32>, lsq::io_f32>(pl, act, M, w, N, K, group_size, bits, y, s); break;
    }
    return hip_status(e, what);
}

int lsq_qlinear_a8_plan(int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int32_t* out8) {
    const char* what = "lsq_qlinear_a8_plan";
    if (int rc = check_shape(LSQ_F32, M, N, K, group_size, bits, what)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::A8Plan pl = lsq::plan_a8(M, N, K, group_size, bits, true);
    lsq::write_plan8(out8, pl.mfma, pl.grid, pl.block, pl.lds, pl.mfma ? pl.geo.chunk_k : 0, pl.waves, pl.cols);
    return LSQ_OK;
}

}  // extern "C"
