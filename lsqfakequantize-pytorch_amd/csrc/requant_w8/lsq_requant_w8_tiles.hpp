// lsq_requant_w8_tiles.hpp -- the W8A8 TILES kernel with an 8-bit output: csrc/qconv_w8/lsq_w8_tiles_loop.hpp's body with an
// epilogue that requantizes in registers, gathers the tile's bytes in LDS and stores 16-byte packets along n.
#pragma once
#include "../qconv_w8/lsq_qconv_w8_tiles.hpp"

namespace lsq {

struct W8OutArg {           // kernel argument: the output quantizer
    const float* scale;     // one value each, read in the kernel
    const float* shift;
    float qmin, qmax, tmin, tmax;
    int relu;
    int mid;                // LSQ_F32 / LSQ_BF16 / LSQ_F16: the rounding between the fp32 steps and the quantizer
    int packets;            // tiles: N % 16 == 0 and y 16-byte aligned
};

struct W8OutQ {
    QParams<float> qp;
    Range<float> r;
    int relu, mid;
};

__device__ __forceinline__ W8OutQ w8q_constants(const W8OutArg& o) {
    W8OutQ q;
    q.r = Range<float>{o.qmin, o.qmax, o.tmin, o.tmax};
    q.qp = make_qparams<float>(sanitize_scale_per_tensor<float>(o.scale[0]), o.shift[0], q.r);
    q.relu = o.relu;
    q.mid = o.mid;
    return q;
}

// the fp32 steps of the contract on the exact integer (w8_store's), the rounding to mid_dtype, the select, the level
__device__ __forceinline__ uint8_t w8q_byte(int64_t I, const W8Weight& wt, float s_x, int64_t n, const W8OutQ& oq) {
    float v = __fmul_rn(__fmul_rn(wt.scale[n], static_cast<float>(I)), s_x);
    if (wt.bias) v = __fadd_rn(v, w8_bias_at(wt.bias, wt.bias_dtype, n));
    float u = v;
    if (oq.mid == LSQ_BF16) u = static_cast<float>(io_bf16::to_elem(v));
    else if (oq.mid == LSQ_F16) u = static_cast<float>(io_f16::to_elem(v));
    if (oq.relu) u = (u < 0.0f) ? 0.0f : u;         // a select: a NaN stays a NaN and goes to quant_min below
    return static_cast<uint8_t>(static_cast<int>(level<float>(u, oq.qp, oq.r)) & 0xff);
}

// the linear's A operand: row m of a dense [M, K] byte matrix, K % 16 == 0 and `a` 16-byte aligned
struct W8LinSrc {
    const uint8_t* a;
    uint32_t flip;
    int64_t K;
    struct Row { int64_t base; };
    struct Col { int64_t k; };
    __device__ __forceinline__ Row row(int64_t m) const { return Row{m * K}; }
    __device__ __forceinline__ Col col(int64_t k) const { return Col{k}; }
    __device__ __forceinline__ void advance(Col& p) const { p.k += 16; }
    __device__ __forceinline__ u32x4 packet(const Row& r, const Col& p) const {
        return *reinterpret_cast<const u32x4*>(a + r.base + p.k) ^ flip;
    }
};

// the tile's bytes in LDS, [kRows][kCols]: wide tiles over the staging area, split K behind the four int32 tiles that lie
// over it.  A lane of the epilogue holds four rows of ONE column: stored from there the bytes would be 1-byte stores strided
// by N.
template <int SUBS, bool SPLITK>
__device__ __forceinline__ unsigned char* w8q_tile_bytes() {
    typedef W8TileShape<SUBS, SPLITK> T;
    constexpr int kOffset = SPLITK ? kW8TileWaves * SUBS * 64 * 16 : 0;
    static_assert(kOffset + T::kRows * T::kCols <= T::kRows * kW8TileStride, "the byte tile fits the staging area");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    return smem + kOffset;
}

// the stores of the byte tile, along n, after the barrier behind the epilogue.  Bytes of columns n >= N and of rows m >= rows
// are never read.
template <int SUBS, bool SPLITK>
__device__ __forceinline__ void w8q_store_tile(const W8TileAt at, int64_t N, int packets, uint8_t* __restrict__ y) {
    typedef W8TileShape<SUBS, SPLITK> T;
    const unsigned char* outb = w8q_tile_bytes<SUBS, SPLITK>();
    const int tid = static_cast<int>(threadIdx.x);
    if (packets) {                                  // N % 16 == 0: a packet that starts inside N lies inside N
        constexpr int kPackets = T::kCols / 16;     // per row
        for (int it = tid; it < T::kRows * kPackets; it += T::kThreads) {
            const int m = it / kPackets, p = it - m * kPackets;
            const int64_t n = at.nt0 + p * 16;
            if (m < at.rows && n < N)
                *reinterpret_cast<u32x4*>(y + (at.m0 + m) * N + n) = *reinterpret_cast<const u32x4*>(outb + m * T::kCols + p * 16);
        }
    } else {
        for (int it = tid; it < T::kRows * T::kCols; it += T::kThreads) {
            const int m = it / T::kCols, c = it - m * T::kCols;
            const int64_t n = at.nt0 + c;
            if (m < at.rows && n < N) y[(at.m0 + m) * N + n] = outb[it];
        }
    }
}

template <int SUBS, bool SPLITK, typename Src>
__device__ __forceinline__ void w8q_tiles_body(const Src src, const W8Const ac, const W8Weight& wt, const W8Geom& geo,
                                               const W8OutArg& out, uint8_t* __restrict__ y) {
    constexpr int kCols = W8TileShape<SUBS, SPLITK>::kCols;
    unsigned char* outb = w8q_tile_bytes<SUBS, SPLITK>();
    const W8TileAt at = w8_tile_at<SUBS, SPLITK>(geo);
    w8_tiles_run<SUBS, SPLITK>(src, ac, wt, geo, [] {}, [] {}, [&] {
        const W8OutQ oq = w8q_constants(out);
        return [=, &wt](int64_t I, int m, int c, int64_t n) { outb[m * kCols + c] = w8q_byte(I, wt, ac.s_x, n, oq); };
    });
    __syncthreads();
    w8q_store_tile<SUBS, SPLITK>(at, geo.N, out.packets, y);
}

// ------------------------------------------------------------------------------------------------
// WRITTEN OUT, for requant_w8_linear_tiles_kernel only: w8q_tiles_body as one function, K loop included.  On w8_tiles_run the
// split-K SUBS = 8 linear kernel measured 1.7-2.0 % slower on [4096, 4096] at M = 128 (its K loop the same instructions in
// other registers); written out, the six linear kernels are instruction for instruction what they were ("One
// tile loop").  A fix to w8_tiles_run's loop or to w8q_store_tile belongs here too.
// ------------------------------------------------------------------------------------------------
// the tile's bytes in LDS: wide tiles over the staging area, split K behind the four int32 tiles that lie over it
template <int SUBS, bool SPLITK>
constexpr int w8q_lin_out_offset() { return SPLITK ? kW8TileWaves * SUBS * 64 * 16 : 0; }

template <int SUBS, bool SPLITK, typename Src>
__device__ __forceinline__ void w8q_lin_tiles_body(const Src src, const W8Const ac, const W8Weight& wt, const W8Geom& geo,
                                               const W8OutArg& out, uint8_t* __restrict__ y) {
    constexpr int kRows = SUBS * 16;
    constexpr int kThreads = kW8TileWaves * 64;
    constexpr int NT = SPLITK ? 1 : 4;              // MFMA k-steps of 64 per wave and step
    constexpr int kItems = (kRows * 4 + kThreads - 1) / kThreads;      // (row, 64 bytes) staging items per thread
    constexpr int kCols = SPLITK ? kW8Tile : kW8Tile * kW8TileWaves;   // output columns of the tile
    static_assert(kThreads % 4 == 0, "a thread's items share their quarter of the step");
    static_assert(w8q_lin_out_offset<SUBS, SPLITK>() + kRows * kCols <= kRows * kW8TileStride, "the byte tile fits the staging area");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* xs = smem;                                                   // [kRows][kW8TileStride]
    int32_t* rowsum = reinterpret_cast<int32_t*>(smem + kRows * kW8TileStride);  // [kRows][4]
    int32_t* redC = rowsum + kRows * 4;                                         // [wave][column]
    int32_t* redP = reinterpret_cast<int32_t*>(smem);                           // split K: [wave][sub-tile][lane][register], over xs
    unsigned char* outb = smem + w8q_lin_out_offset<SUBS, SPLITK>();                // [kRows][kCols], over xs

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const uint32_t flipw = wt.off ? 0x80808080u : 0u;
    const int64_t K = geo.K, N = geo.N, n_p = K / 16;
    const int64_t tile = static_cast<int64_t>(blockIdx.x);
    const int64_t col_tile = tile / geo.row_tiles, row_tile = tile - col_tile * geo.row_tiles;
    const int64_t m0 = row_tile * kRows;
    const int rows = static_cast<int>(std::min<int64_t>(kRows, geo.M - m0));   // >= 1
    const int64_t n0 = SPLITK ? col_tile * kW8Tile : (col_tile * kW8TileWaves + wave) * kW8Tile;
    const int64_t row = std::min<int64_t>(n0 + nl, N - 1);                     // a clamped row computes a value nobody stores
    const uint8_t* __restrict__ wrow = wt.w + row * K;
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const int ts = tid & 3;

    i32x4 P[SUBS];
#pragma unroll
    for (int rt = 0; rt < SUBS; ++rt) P[rt] = i32x4{0, 0, 0, 0};
    i32x4 C = {0, 0, 0, 0};
    int rs[kItems];                                 // sum a of this thread's staging items over all steps
    typename Src::Row srow[kItems];                 // ... and where their rows come from
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        rs[j] = 0;
        srow[j] = src.row(m0 + ((tid + j * kThreads) >> 2));
    }

    auto load_b = [&](u32x4 (&b)[NT], int64_t k0) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int t = SPLITK ? wave : j;
            const int64_t p = k0 / 16 + 4 * t + q;
            b[j] = u32x4{0u, 0u, 0u, 0u};
            if (p < n_p) b[j] = load_code_packet(wrow, p) ^ flipw;
        }
    };

    u32x4 nxt[NT];
    load_b(nxt, 0);
    for (int64_t k0 = 0; k0 < K; k0 += kW8Step) {   // the same for the whole grid
        u32x4 cur[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) cur[j] = nxt[j];
        __syncthreads();                            // the previous step's reads of LDS are done
        typename Src::Col scol = src.col(k0 + ts * 64);
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) {
            const int64_t k = k0 + ts * 64 + bb * 16;
#pragma unroll
            for (int j = 0; j < kItems; ++j) {
                const int it = tid + j * kThreads;
                if (it < kRows * 4) {
                    const int m = it >> 2;
                    u32x4 v = {0u, 0u, 0u, 0u};
                    if (m < rows && k < K) v = src.packet(srow[j], scol);
                    *reinterpret_cast<u32x4*>(xs + m * kW8TileStride + ts * 64 + bb * 16) = v;
                    rs[j] += w8_sum_bytes(v.x) + w8_sum_bytes(v.y) + w8_sum_bytes(v.z) + w8_sum_bytes(v.w);
                }
            }
            src.advance(scol);
        }
        __syncthreads();
        if (k0 + kW8Step < K) load_b(nxt, k0 + kW8Step);    // in flight during this step's MFMAs
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int t = SPLITK ? wave : j;
            const i32x4 bt = w8_as_i32(cur[j]);
            C = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bt, C, 0, 0, 0);
            const unsigned char* xa = xs + nl * kW8TileStride + t * 64 + q * 16;
#pragma unroll
            for (int rt = 0; rt < SUBS; ++rt) {
                const i32x4 a = *reinterpret_cast<const i32x4*>(xa + rt * 16 * kW8TileStride);
                P[rt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bt, P[rt], 0, 0, 0);
            }
        }
    }

    __syncthreads();                                // the last step's reads of LDS are done: the staging area is free
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const int it = tid + j * kThreads;
        if (it < kRows * 4) rowsum[it] = rs[j];
    }
    if constexpr (SPLITK) {
#pragma unroll
        for (int rt = 0; rt < SUBS; ++rt) *reinterpret_cast<i32x4*>(redP + ((wave * SUBS + rt) * 64 + lane) * 4) = P[rt];
        if (q == 0) redC[wave * 16 + nl] = C[0];
    }
    __syncthreads();

    // ---- the epilogue: one byte per output, in registers, into the byte tile [kRows][kCols] in LDS ----
    // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register.  A lane holds four rows of ONE column: stored from
    // here the bytes would be 1-byte stores strided by N.
    const W8OutQ oq = w8q_constants(out);
    if constexpr (SPLITK) {
        const int l = tid & 63, reg = tid >> 6;
        const int col = l & 15;
        const int64_t n = n0 + col;
        if (n < N) {
            int64_t sc = 0;
#pragma unroll
            for (int w = 0; w < kW8TileWaves; ++w) sc += redC[w * 16 + col];
            const int z_w = wt.zero[n] - wt.off;
#pragma unroll
            for (int rt = 0; rt < SUBS; ++rt) {
                const int m = rt * 16 + (l >> 4) * 4 + reg;
                if (m < rows) {
                    int64_t sp = 0;
#pragma unroll
                    for (int w = 0; w < kW8TileWaves; ++w) sp += redP[((w * SUBS + rt) * 64 + l) * 4 + reg];
                    const int64_t ss = static_cast<int64_t>(rowsum[m * 4]) + rowsum[m * 4 + 1] + rowsum[m * 4 + 2] + rowsum[m * 4 + 3];
                    outb[m * kCols + col] = w8q_byte(w8_exact(sp, sc, ss, K, ac.z, z_w), wt, ac.s_x, n, oq);
                }
            }
        }
    } else {
        const int64_t n = n0 + nl;
        if (n < N) {
            const int z_w = wt.zero[n] - wt.off;
#pragma unroll
            for (int rt = 0; rt < SUBS; ++rt) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = rt * 16 + q * 4 + i;
                    if (m < rows) {
                        const int64_t ss = static_cast<int64_t>(rowsum[m * 4]) + rowsum[m * 4 + 1] + rowsum[m * 4 + 2] + rowsum[m * 4 + 3];
                        outb[m * kCols + wave * kW8Tile + nl] = w8q_byte(w8_exact(P[rt][i], C[i], ss, K, ac.z, z_w), wt, ac.s_x, n, oq);
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- the stores, along n.  Bytes of columns n >= N and of rows m >= rows were never written and are never read. ----
    const int64_t nt0 = col_tile * kCols;           // the tile's first column
    if (out.packets) {                              // N % 16 == 0: a packet that starts inside N lies inside N
        constexpr int kPackets = kCols / 16;        // per row
        for (int it = tid; it < kRows * kPackets; it += kThreads) {
            const int m = it / kPackets, p = it - m * kPackets;
            const int64_t n = nt0 + p * 16;
            if (m < rows && n < N)
                *reinterpret_cast<u32x4*>(y + (m0 + m) * N + n) = *reinterpret_cast<const u32x4*>(outb + m * kCols + p * 16);
        }
    } else {
        for (int it = tid; it < kRows * kCols; it += kThreads) {
            const int m = it / kCols, c = it - m * kCols;
            const int64_t n = nt0 + c;
            if (m < rows && n < N) y[(m0 + m) * N + n] = outb[it];
        }
    }
}


}  // namespace lsq
