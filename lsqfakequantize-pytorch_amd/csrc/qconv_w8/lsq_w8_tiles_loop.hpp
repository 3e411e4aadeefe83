// lsq_w8_tiles_loop.hpp -- the W8A8 TILES kernel's body, once, for the three libraries whose tile kernels read their A
// operand through a packet SOURCE: csrc/qconv_w8/ (float output), csrc/requant_w8/ (8-bit output) and csrc/resadd_w8/ (8-bit
// output with a residual).  Two more copies of this K loop remain: qlinear_w8_tiles_kernel in
// csrc/qlinear_w8/lsq_qlinear_w8.hip, which stages through w8_load16 and whose kernels change by 10 to 34 VGPRs when they
// share a function template ("Code sharing"), and w8q_lin_tiles_body in
// csrc/requant_w8/lsq_requant_w8_tiles.hpp, where one linear kernel measured 2 % slower on this body ("One
// tile loop"): a fix to the loop belongs in all three.
//
// The body works on an [M, K] matrix of byte operands a = lx - off against the weight's [N, K] bytes.  It does not read the
// matrix itself: `Src` says where packet (row m, bytes k .. k + 15) comes from.
//     struct Src {
//         struct Row;  Row row(int64_t m) const;                  // once per staging row, before the K loop
//         struct Col;  Col col(int64_t k) const;                  // once per step: the thread's first packet, k % 64 == 0
//         void advance(Col&) const;                               // the packet 16 bytes further
//         u32x4 packet(const Row&, const Col&) const;             // the 16 byte operands; called for m < M and k < K only
//     };
// What the three kernels do differently is in three callables:
//     last_step()                  in the last K step, in the place of the load of the next weight packets
//     before_epilogue()            after the loop, when the staging area is free and before the barrier that publishes the row
//                                  sums and the split-K partials: what else the epilogue reads from LDS is written here
//     epilogue()                   after that barrier: forms the epilogue's constants (here and not earlier: they would stay live
//                                  across the loop) and returns emit(I, m, c, n), which is called with the exact integer I of
//                                  row m and column c of the tile, which is output column n
#pragma once
#include "../qlinear_w8/lsq_w8_shared.hpp"

namespace lsq {

template <int SUBS, bool SPLITK>
struct W8TileShape {
    static constexpr int kRows = SUBS * 16;
    static constexpr int kThreads = kW8TileWaves * 64;
    static constexpr int kCols = SPLITK ? kW8Tile : kW8Tile * kW8TileWaves;    // output columns of the tile
};

struct W8TileAt {           // where this workgroup's tile lies (scalars only)
    int64_t m0, nt0;        // its first row and column
    int rows;               // its rows inside M: >= 1
};

template <int SUBS, bool SPLITK>
__device__ __forceinline__ W8TileAt w8_tile_at(const W8Geom& geo) {
    typedef W8TileShape<SUBS, SPLITK> T;
    const int64_t tile = static_cast<int64_t>(blockIdx.x);
    const int64_t col_tile = tile / geo.row_tiles, row_tile = tile - col_tile * geo.row_tiles;
    const int64_t m0 = row_tile * T::kRows;
    return W8TileAt{m0, col_tile * T::kCols, static_cast<int>(std::min<int64_t>(T::kRows, geo.M - m0))};
}

// ------------------------------------------------------------------------------------------------
// matrix-core form, TILES: a workgroup of 4 waves owns 16 * SUBS rows and walks K in steps of 256, staging the rows' 256
// bytes per step; the staging threads keep sum_k a of their rows in registers.  Wide: 64 columns, wave v owns columns
// 16 v .. 16 v + 15 and all of the step.  SPLITK: 16 columns, wave v takes k 64 v .. 64 v + 63 of every step, and the four
// int32 tiles are summed through LDS.  The next step's weight packets are in flight during this step's MFMAs.
// A thread stages the same 64-byte quarter (tid & 3) of every step for each of its rows.
// ------------------------------------------------------------------------------------------------
template <int SUBS, bool SPLITK, typename Src, typename LastStep, typename BeforeEpilogue, typename Epilogue>
__device__ __forceinline__ void w8_tiles_run(const Src src, const W8Const ac, const W8Weight& wt, const W8Geom& geo, LastStep last_step,
                                             BeforeEpilogue before_epilogue, Epilogue epilogue) {
    constexpr int kRows = W8TileShape<SUBS, SPLITK>::kRows, kThreads = W8TileShape<SUBS, SPLITK>::kThreads;
    constexpr int NT = SPLITK ? 1 : 4;             // MFMA k-steps of 64 per wave and step
    constexpr int kItems = (kRows * 4 + kThreads - 1) / kThreads;      // (row, 64 bytes) staging items per thread
    static_assert(kThreads % 4 == 0, "a thread's items share their quarter of the step");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* xs = smem;                                                   // [kRows][kW8TileStride]
    int32_t* rowsum = reinterpret_cast<int32_t*>(smem + kRows * kW8TileStride);  // [kRows][4]
    int32_t* redC = rowsum + kRows * 4;                                         // [wave][column]
    int32_t* redP = reinterpret_cast<int32_t*>(smem);                           // split K: [wave][sub-tile][lane][register], over xs

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const uint32_t flipw = wt.off ? 0x80808080u : 0u;
    const int64_t K = geo.K, N = geo.N, n_p = K / 16;
    const W8TileAt at = w8_tile_at<SUBS, SPLITK>(geo);                         // the callables' wrappers ask the same function
    const int64_t m0 = at.m0;
    const int rows = at.rows;
    const int64_t n0 = SPLITK ? at.nt0 : at.nt0 + wave * kW8Tile;
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
        else last_step();
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
    before_epilogue();
    __syncthreads();
    const auto emit = epilogue();

    // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register.  A lane holds four rows of ONE column.
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
                    emit(w8_exact(sp, sc, ss, K, ac.z, z_w), m, col, n);
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
                        emit(w8_exact(P[rt][i], C[i], ss, K, ac.z, z_w), m, wave * kW8Tile + nl, n);
                    }
                }
            }
        }
    }
}

}  // namespace lsq
