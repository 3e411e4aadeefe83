// lsq_resadd_w8_tiles.hpp -- the W8A8 TILES kernel that closes a residual block: csrc/requant_w8/lsq_requant_w8_tiles.hpp's
// w8q_tiles_body (the K loop of csrc/qconv_w8/lsq_qconv_w8_tiles.hpp's w8_tiles_body, step for step) with a residual LEVEL per
// output in the epilogue.  The residual tile is loaded as 16-byte packets along n during the LAST K step (behind its MFMAs),
// written into the LDS region of the output byte tile after the loop's last barrier, and read from there by the lane that
// forms the output byte, which then overwrites it.  The body is written out here rather than shared through an epilogue hook
// of w8q_tiles_body: liblsq_hip_requant_w8.so stays byte for byte what it is ("Code sharing").  A fix to the
// loop belongs in all four copies.
#pragma once
#include "../requant_w8/lsq_requant_w8_tiles.hpp"

namespace lsq {

struct W8ResArg {           // kernel argument: the residual levels, dense [M, N] bytes in y's layout
    const uint8_t* l;
    const float* scale;     // one value each, read in the kernel as they are
    const int32_t* zero;
    int is_signed;          // int8 levels
    int packets;            // tiles: N % 16 == 0 and `l` 16-byte aligned
};

struct W8PreArg {           // kernel argument: the layer's own output fake-quantizer
    const float* scale;     // NULL: none
    const float* shift;
    float qmin, qmax, tmin, tmax;
};

struct W8ResQ {
    float s, z;
    int is_signed;
};

struct W8PreQ {
    QParams<float> qp;
    Range<float> r;
    int on;
};

__device__ __forceinline__ W8ResQ w8r_res_constants(const W8ResArg& a) {
    return W8ResQ{a.scale[0], static_cast<float>(a.zero[0]), a.is_signed};
}

__device__ __forceinline__ W8PreQ w8r_pre_constants(const W8PreArg& a) {
    W8PreQ p;
    p.on = a.scale != nullptr;
    p.r = Range<float>{a.qmin, a.qmax, a.tmin, a.tmax};
    p.qp = QParams<float>{1.0f, 1.0f, 0.0f};
    if (p.on) p.qp = make_qparams<float>(sanitize_scale_per_tensor<float>(a.scale[0]), a.shift[0], p.r);
    return p;
}

__device__ __forceinline__ float w8r_round(float v, int mid) {
    if (mid == LSQ_BF16) return static_cast<float>(io_bf16::to_elem(v));
    if (mid == LSQ_F16) return static_cast<float>(io_f16::to_elem(v));
    return v;
}

// w8q_byte with the contract's p, d and t between the rounding to mid_dtype and the select.  Every step is rounded once: the
// product d and the sum p + d are NOT one fused multiply-add (for mid_dtype float32 the rounding between them is the identity).
__device__ __forceinline__ uint8_t w8r_byte(int64_t I, const W8Weight& wt, float s_x, int64_t n, const W8OutQ& oq, const W8PreQ& pq,
                                            const W8ResQ& rq, uint8_t lr) {
    float v = __fmul_rn(__fmul_rn(wt.scale[n], static_cast<float>(I)), s_x);
    if (wt.bias) v = __fadd_rn(v, w8_bias_at(wt.bias, wt.bias_dtype, n));
    const float u = w8r_round(v, oq.mid);
    float p = u;
    if (pq.on) p = w8r_round(dequant<float>(level<float>(u, pq.qp, pq.r), pq.qp), oq.mid);
    const float lf = rq.is_signed ? static_cast<float>(static_cast<int8_t>(lr)) : static_cast<float>(lr);
    const float d = w8r_round(__fmul_rn(__fsub_rn(lf, rq.z), rq.s), oq.mid);
    float t = w8r_round(__fadd_rn(p, d), oq.mid);
    if (oq.relu) t = (t < 0.0f) ? 0.0f : t;         // a select: a NaN stays a NaN and goes to quant_min below
    return static_cast<uint8_t>(static_cast<int>(level<float>(t, oq.qp, oq.r)) & 0xff);
}

template <int SUBS, bool SPLITK, typename Src>
__device__ __forceinline__ void w8r_tiles_body(const Src src, const W8Const ac, const W8Weight& wt, const W8Geom& geo,
                                               const W8OutArg& out, const W8ResArg& res, const W8PreArg& pre,
                                               uint8_t* __restrict__ y) {
    constexpr int kRows = SUBS * 16;
    constexpr int kThreads = kW8TileWaves * 64;
    constexpr int NT = SPLITK ? 1 : 4;              // MFMA k-steps of 64 per wave and step
    constexpr int kItems = (kRows * 4 + kThreads - 1) / kThreads;      // (row, 64 bytes) staging items per thread
    constexpr int kCols = SPLITK ? kW8Tile : kW8Tile * kW8TileWaves;   // output columns of the tile
    constexpr int kPackets = kCols / 16;            // 16-byte packets of a row of the byte tile
    constexpr int kResItems = (kRows * kPackets + kThreads - 1) / kThreads;    // residual packets per thread: at most 2
    static_assert(kThreads % 4 == 0, "a thread's items share their quarter of the step");
    static_assert(kResItems <= 2, "the residual tile costs a thread at most eight registers");
    static_assert(w8q_out_offset<SUBS, SPLITK>() + kRows * kCols <= kRows * kW8TileStride, "the byte tile fits the staging area");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* xs = smem;                                                   // [kRows][kW8TileStride]
    int32_t* rowsum = reinterpret_cast<int32_t*>(smem + kRows * kW8TileStride);  // [kRows][4]
    int32_t* redC = rowsum + kRows * 4;                                         // [wave][column]
    int32_t* redP = reinterpret_cast<int32_t*>(smem);                           // split K: [wave][sub-tile][lane][register], over xs
    unsigned char* outb = smem + w8q_out_offset<SUBS, SPLITK>();                // [kRows][kCols], over xs: residual in, y out

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const uint32_t flipw = wt.off ? 0x80808080u : 0u;
    const int64_t K = geo.K, N = geo.N, n_p = K / 16;
    const int64_t tile = static_cast<int64_t>(blockIdx.x);
    const int64_t col_tile = tile / geo.row_tiles, row_tile = tile - col_tile * geo.row_tiles;
    const int64_t m0 = row_tile * kRows;
    const int rows = static_cast<int>(std::min<int64_t>(kRows, geo.M - m0));   // >= 1
    const int64_t n0 = SPLITK ? col_tile * kW8Tile : (col_tile * kW8TileWaves + wave) * kW8Tile;
    const int64_t nt0 = col_tile * kCols;           // the tile's first column
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
    u32x4 rp[kResItems];                            // this thread's packets of the residual tile
#pragma unroll
    for (int j = 0; j < kResItems; ++j) rp[j] = u32x4{0u, 0u, 0u, 0u};

    auto load_b = [&](u32x4 (&b)[NT], int64_t k0) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int t = SPLITK ? wave : j;
            const int64_t p = k0 / 16 + 4 * t + q;
            b[j] = u32x4{0u, 0u, 0u, 0u};
            if (p < n_p) b[j] = load_code_packet(wrow, p) ^ flipw;
        }
    };
    // N % 16 == 0: a packet that starts inside N lies inside N (the guard of the packet store)
    auto load_res = [&]() {
#pragma unroll
        for (int j = 0; j < kResItems; ++j) {
            const int it = tid + j * kThreads;
            const int m = it / kPackets, p = it - m * kPackets;
            const int64_t n = nt0 + p * 16;
            if (it < kRows * kPackets && m < rows && n < N) rp[j] = *reinterpret_cast<const u32x4*>(res.l + (m0 + m) * N + n);
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
        else if (res.packets) load_res();                   // the last step: the residual tile in the place of the next b
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
    // the residual tile into the byte tile (no byte of it overlaps rowsum, redC or redP).  Bytes of columns n >= N and of rows
    // m >= rows are not written here, not read in the epilogue and not stored.
    if (res.packets) {
#pragma unroll
        for (int j = 0; j < kResItems; ++j) {
            const int it = tid + j * kThreads;
            if (it < kRows * kPackets) *reinterpret_cast<u32x4*>(outb + it * 16) = rp[j];
        }
    } else {                                        // byte by byte along n: consecutive lanes on consecutive bytes
        for (int it = tid; it < kRows * kCols; it += kThreads) {
            const int m = it / kCols, c = it - m * kCols;
            const int64_t n = nt0 + c;
            if (m < rows && n < N) outb[it] = res.l[(m0 + m) * N + n];
        }
    }
    __syncthreads();

    // ---- the epilogue: one byte per output, in registers, over its residual byte in the byte tile [kRows][kCols] in LDS ----
    // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register.  A lane holds four rows of ONE column: it reads the
    // residual byte at (m, column) and writes the output byte to the same place -- no other lane touches that byte.
    const W8OutQ oq = w8q_constants(out);
    const W8PreQ pq = w8r_pre_constants(pre);
    const W8ResQ rq = w8r_res_constants(res);
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
                    unsigned char* at = outb + m * kCols + col;
                    *at = w8r_byte(w8_exact(sp, sc, ss, K, ac.z, z_w), wt, ac.s_x, n, oq, pq, rq, *at);
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
                        unsigned char* at = outb + m * kCols + wave * kW8Tile + nl;
                        *at = w8r_byte(w8_exact(P[rt][i], C[i], ss, K, ac.z, z_w), wt, ac.s_x, n, oq, pq, rq, *at);
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- the stores, along n.  Bytes of columns n >= N and of rows m >= rows are never read. ----
    if (out.packets) {                              // N % 16 == 0: a packet that starts inside N lies inside N
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
