// lsq_qlinear_w8.hip -- 8-bit activation levels times 8-bit weight levels with one (scale, zero point) per output row on
// gfx950 (include/lsq_hip_qlinear_w8.h, which states the arithmetic contract): the kernels and the C ABI of
// liblsq_hip_qlinear_w8.so.
//
//     I[m, n] = sum_k (lx[m, k] - zx) * (lw[n, k] - zw[n]),   y[m, n] = ((s_w[n] * float(I)) * s_x) + bias[n]
//
// Every kernel works on the BYTE OPERANDS a = lx - off_x and w = lw - off_w (off = 128 for a 0..255 range, else 0: byte ^ 0x80
// read as int8 is byte - 128), int8 for every legal level, and on z_a = zx - off_x, z_w = zw[n] - off_w:
//     I = sum a w  -  z_a sum_k w  -  z_w sum_k a  +  K z_a z_w
// in 64-bit integers, once per output.  The sum runs over all of K, and an integer sum has no order: the kernels split K
// over waves and steps as they like and the bits do not change.
//
//  * MATRIX-CORE form (K % 16 == 0, K <= 65536 so that the raw sums fit 32 bits, lw 16-byte aligned).  One
//    v_mfma_i32_16x16x64_i8 multiplies 16 rows of x by 16 rows of w over 64 k: lane (i = lane & 15, q = lane >> 4) holds bytes
//    16 q .. 16 q + 15 of those 64 of row i, for A and for B alike, and D has column = lane & 15, row = 4 * (lane >> 4) +
//    register.  The B operand is 16 bytes of lw as they lie in memory (one non-temporal global_load_dwordx4, an xor for a
//    uint8 weight): no unpack.  The A operand is one ds_read_b128 of x, staged in LDS as the byte operand.  A second MFMA
//    with an all-ones A operand gives sum_k w per column.  A K that is no multiple of 64 ends in a step whose missing
//    16-byte packets are zero on both sides.
//      DECODE (M <= 16): a workgroup of 16 waves owns 16 output columns and walks the tiles in a persistent grid.  x is
//      staged in chunks of at most 4096 k (and stays in LDS across tiles when one chunk holds all of K); wave v takes the
//      256 k of the chunk that start at 256 v: four packets per lane in flight, issued before x is staged.  A third MFMA
//      with an all-ones B operand gives sum_k a per row.  The waves' int32 tiles are summed through LDS, one thread per output.
//      TILES (M > 16): a workgroup of 4 waves owns 16 * SUBS rows (SUBS = 2 / 4 / 8 for M <= 32 / <= 64 / more) and walks K
//      in steps of 256, staging the rows' 256 bytes per step; the staging threads keep sum_k a of their rows in registers.
//      Wide: 64 columns, wave v owns columns 16 v .. 16 v + 15 and all of the step.  Split K, while the wide tiles would
//      not give every compute unit one: 16 columns, wave v takes k 64 v .. 64 v + 63 of every step, and the four int32
//      tiles are summed through LDS.  The next step's weight packets are in flight during this step's MFMAs.
//  * GENERIC form (every other legal call): one wave per output column, four rows of x at a time, 64-bit integer
//    multiply-adds over the lanes' k and a butterfly.  Correct for every legal input; not tuned.
//  * The fused entry form runs a pre-pass (levels_kernel) that writes the byte operand a = level(x) - off into the caller's
//    workspace with lsq_math.hpp's make_qparams / level(); everything after it is the levels form's code.
#include "lsq_w8_shared.hpp"
#include "../../../include/lsq_hip_qlinear_w8.h"

namespace lsq {

constexpr int kW8Waves = 16;                        // decode: waves that split K
constexpr int kW8Block = kW8Waves * 64;
constexpr int kW8Chunk = 4096;                      // decode: most elements of K per LDS chunk of x
constexpr int kW8RedBytes = kW8Waves * 256 * 4 + 2 * kW8Waves * 16 * 4;   // decode: sum a w, sum a, sum w of every wave

// ------------------------------------------------------------------------------------------------
// matrix-core form, DECODE: up to 16 rows of x
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kW8Block) void qlinear_w8_decode_kernel(W8Act act, int M, W8Weight wt, int64_t N, int64_t K, int row_stride,
                                                                    void* __restrict__ y, int y_dtype) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t* redP = reinterpret_cast<int32_t*>(smem);       // [wave][lane][register]
    int32_t* redS = redP + kW8Waves * 256;                  // [wave][row]
    int32_t* redC = redS + kW8Waves * 16;                   // [wave][column]
    unsigned char* xs = smem + kW8RedBytes;

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const W8Const ac = w8_constants(act);
    const uint32_t flipw = wt.off ? 0x80808080u : 0u;
    const int64_t n_p = K / 16;                             // 16-byte packets per row
    const int64_t tiles = (N + kW8Tile - 1) / kW8Tile;
    const int64_t n_chunks = (K + kW8Chunk - 1) / kW8Chunk;
    const int64_t first_tile = static_cast<int64_t>(blockIdx.x);
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};

    for (int64_t tile = first_tile; tile < tiles; tile += static_cast<int64_t>(gridDim.x)) {
        const int64_t row = std::min<int64_t>(tile * kW8Tile + nl, N - 1);         // a clamped row computes a value nobody stores
        const uint8_t* __restrict__ wrow = wt.w + row * K;
        i32x4 P = {0, 0, 0, 0}, S = {0, 0, 0, 0}, C = {0, 0, 0, 0};
        for (int64_t c = 0; c < n_chunks; ++c) {
            const int64_t kc0 = c * kW8Chunk;
            const int64_t k0 = kc0 + wave * kW8Step;        // this wave's 256 k of the chunk
            u32x4 b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int64_t p = k0 / 16 + 4 * t + q;
                b[t] = u32x4{0u, 0u, 0u, 0u};
                if (p < n_p) b[t] = load_code_packet(wrow, p) ^ flipw;
            }
            if (n_chunks > 1 || tile == first_tile) {       // x stays in LDS across tiles when one chunk holds it
                __syncthreads();
                const int kc_len = static_cast<int>(std::min<int64_t>(kW8Chunk, K - kc0));
                const int nb = kc_len / 16;                 // blocks of 16 k per row; exact
                const int nbp = (nb + 15) & ~15;            // ... up to whole steps, zero beyond the row
                for (int it = tid; it < M * nbp; it += kW8Block) {
                    const int m = it / nbp, bb = it - m * nbp;
                    u32x4 v = {0u, 0u, 0u, 0u};
                    if (bb < nb) v = w8_load16(act, ac.flip, static_cast<int64_t>(m) * K + kc0 + bb * 16);
                    *reinterpret_cast<u32x4*>(xs + m * row_stride + bb * 16) = v;
                }
                __syncthreads();
            }
            if (k0 < K) {                                   // the same for the whole wave
                const unsigned char* xa = xs + nl * row_stride + wave * kW8Step + q * 16;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    i32x4 a = {0, 0, 0, 0};
                    if (nl < M) a = *reinterpret_cast<const i32x4*>(xa + t * 64);
                    const i32x4 bt = w8_as_i32(b[t]);
                    P = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bt, P, 0, 0, 0);
                    S = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, ones, S, 0, 0, 0);
                    C = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bt, C, 0, 0, 0);
                }
            }
        }
        // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register.  S is the same in every column, C in every row.
        *reinterpret_cast<i32x4*>(redP + (wave * 64 + lane) * 4) = P;
        if (nl == 0) *reinterpret_cast<i32x4*>(redS + wave * 16 + q * 4) = S;
        if (q == 0) redC[wave * 16 + nl] = C[0];
        __syncthreads();
        if (tid < 256) {
            const int l = tid & 63, reg = tid >> 6;
            const int col = l & 15, m = (l >> 4) * 4 + reg;
            int64_t sp = 0, ss = 0, sc = 0;
#pragma unroll
            for (int w = 0; w < kW8Waves; ++w) {
                sp += redP[(w * 64 + l) * 4 + reg];
                ss += redS[w * 16 + m];
                sc += redC[w * 16 + col];
            }
            const int64_t n = tile * kW8Tile + col;
            if (m < M && n < N)
                w8_store(w8_exact(sp, sc, ss, K, ac.z, wt.zero[n] - wt.off), wt, ac.s_x, n, y, y_dtype, static_cast<int64_t>(m) * N + n);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// matrix-core form, TILES: any number of rows
// (This K loop is written out here, in csrc/qconv_w8/lsq_w8_tiles_loop.hpp's w8_tiles_run, which nearly every other W8A8 tile kernel
//  runs, and in one more place named there: shared as a function it changes these kernels by 10 to 34 VGPRs.  A fix
//  here belongs there too.)
// ------------------------------------------------------------------------------------------------
template <int SUBS, bool SPLITK>
__global__ __launch_bounds__(kW8TileWaves * 64, 2) void qlinear_w8_tiles_kernel(W8Act act, W8Weight wt, W8Geom geo, void* __restrict__ y,
                                                                               int y_dtype) {
    constexpr int kRows = SUBS * 16;
    constexpr int kThreads = kW8TileWaves * 64;
    constexpr int NT = SPLITK ? 1 : 4;              // MFMA k-steps of 64 per wave and step
    constexpr int kItems = (kRows * 4 + kThreads - 1) / kThreads;      // (row, 64 bytes) staging items per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* xs = smem;                                                   // [kRows][kW8TileStride]
    int32_t* rowsum = reinterpret_cast<int32_t*>(smem + kRows * kW8TileStride);  // [kRows][4]
    int32_t* redC = rowsum + kRows * 4;                                         // [wave][column]
    int32_t* redP = reinterpret_cast<int32_t*>(smem);                           // split K: [wave][sub-tile][lane][register], over xs

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const W8Const ac = w8_constants(act);
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

    i32x4 P[SUBS];
#pragma unroll
    for (int rt = 0; rt < SUBS; ++rt) P[rt] = i32x4{0, 0, 0, 0};
    i32x4 C = {0, 0, 0, 0};
    int rs[kItems];                                 // sum a of this thread's staging items over all steps
#pragma unroll
    for (int j = 0; j < kItems; ++j) rs[j] = 0;

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
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int it = tid + j * kThreads;
            if (it < kRows * 4) {
                const int m = it >> 2, t = it & 3;
                int s = 0;
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) {
                    const int64_t k = k0 + t * 64 + bb * 16;
                    u32x4 v = {0u, 0u, 0u, 0u};
                    if (m < rows && k < K) v = w8_load16(act, ac.flip, (m0 + m) * K + k);
                    *reinterpret_cast<u32x4*>(xs + m * kW8TileStride + t * 64 + bb * 16) = v;
                    s += w8_sum_bytes(v.x) + w8_sum_bytes(v.y) + w8_sum_bytes(v.z) + w8_sum_bytes(v.w);
                }
                rs[j] += s;
            }
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

    __syncthreads();                                // the last step's reads of LDS are done
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

    // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
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
                    w8_store(w8_exact(sp, sc, ss, K, ac.z, z_w), wt, ac.s_x, n, y, y_dtype, (m0 + m) * N + n);
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
                        w8_store(w8_exact(P[rt][i], C[i], ss, K, ac.z, z_w), wt, ac.s_x, n, y, y_dtype, (m0 + m) * N + n);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// generic form
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void qlinear_w8_generic_kernel(W8Act act, int64_t M, W8Weight wt, int64_t N, int64_t K,
                                                                   void* __restrict__ y, int y_dtype) {
    constexpr int R = kQGenericRowsAtOnce;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    const W8Const ac = w8_constants(act);
    const uint8_t flipx = static_cast<uint8_t>(ac.flip & 0xffu), flipw = static_cast<uint8_t>(wt.off);
    for (int64_t n = wave; n < N; n += waves) {
        const uint8_t* __restrict__ wrow = wt.w + n * K;
        const int z_w = wt.zero[n] - wt.off;
        for (int64_t m0 = 0; m0 < M; m0 += R) {
            int64_t I[R];
#pragma unroll
            for (int i = 0; i < R; ++i) I[i] = 0;
            for (int64_t k = lane; k < K; k += 64) {
                const int64_t wz = static_cast<int>(static_cast<int8_t>(wrow[k] ^ flipw)) - z_w;
#pragma unroll
                for (int i = 0; i < R; ++i)
                    if (m0 + i < M) I[i] += (static_cast<int>(static_cast<int8_t>(act.a[(m0 + i) * K + k] ^ flipx)) - ac.z) * wz;
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                for (int s = 32; s >= 1; s >>= 1) I[i] += w8_shfl_xor_i64(I[i], s);        // integers: any order
                if (lane == 0 && m0 + i < M) w8_store(I[i], wt, ac.s_x, n, y, y_dtype, (m0 + i) * N + n);
            }
        }
    }
}

// the fused form's pre-pass: ws[i] = level(x[i]) - off as a byte, 16 elements per thread and turn, then the tail
template <typename IO>
__global__ __launch_bounds__(kBlock) void qlinear_w8_levels_kernel(const void* __restrict__ x, int64_t n, const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, float qmin, float qmax, float tmin,
                                                                  float tmax, int off, uint8_t* __restrict__ ws) {
    const Range<float> r = Range<float>{qmin, qmax, tmin, tmax};
    const QParams<float> qp = make_qparams<float>(sanitize_scale_per_tensor<float>(scale[0]), shift[0], r);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock, n16 = n / 16;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    for (int64_t i = first; i < n16; i += stride) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int a = static_cast<int>(level<float>(IO::load1(x, i * 16 + j), qp, r)) - off;
            w[j >> 2] |= static_cast<uint32_t>(a & 0xff) << ((j & 3) * 8);
        }
        *reinterpret_cast<u32x4*>(ws + i * 16) = u32x4{w[0], w[1], w[2], w[3]};
    }
    for (int64_t i = n16 * 16 + first; i < n; i += stride)
        ws[i] = static_cast<uint8_t>((static_cast<int>(level<float>(IO::load1(x, i), qp, r)) - off) & 0xff);
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launchers
// ------------------------------------------------------------------------------------------------
struct W8Plan {
    int form, shape, block, lds, rows, cols, ksplit, subs, row_stride;
    int64_t grid, row_tiles, col_tiles;
};

constexpr int kW8MaxDecodeLds = kW8RedBytes + 16 * (kW8Chunk + kW8RowPad);

inline W8Plan plan_w8(int64_t M, int64_t N, int64_t K, bool aligned) {
    W8Plan pl = {};
    const int64_t cus = device_info().cu_count;
    if (!(aligned && K > 0 && K % 16 == 0 && K <= kW8MaxK)) {
        pl.form = 0;
        pl.shape = LSQ_W8_SHAPE_GENERIC;
        pl.block = kBlock;
        pl.rows = kQGenericRowsAtOnce;
        pl.cols = kBlock / 64;
        pl.ksplit = 1;
        pl.grid = generic_grid(N, cus);
        return pl;
    }
    pl.form = 1;
    if (M <= 16) {
        pl.shape = LSQ_W8_SHAPE_DECODE;
        pl.block = kW8Block;
        pl.rows = 16;
        pl.cols = kW8Tile;
        pl.ksplit = kW8Waves;
        pl.row_stride = static_cast<int>(std::min<int64_t>((K + kW8Step - 1) / kW8Step * kW8Step, kW8Chunk)) + kW8RowPad;
        pl.lds = kW8RedBytes + static_cast<int>(M) * pl.row_stride;
        pl.grid = std::min<int64_t>(std::max<int64_t>(1, (N + kW8Tile - 1) / kW8Tile), cus);
        return pl;
    }
    pl.subs = M <= 32 ? 2 : (M <= 64 ? 4 : kW8MaxSubs);
    pl.rows = pl.subs * 16;
    pl.row_tiles = (M + pl.rows - 1) / pl.rows;
    const int64_t wide = (N + 16 * kW8TileWaves - 1) / (16 * kW8TileWaves);
    // 64-column tiles once they give every compute unit a tile; below that 16-column tiles, four times as many, K split over the waves
    const bool split = wide <= INT64_MAX / pl.row_tiles && pl.row_tiles * wide < cus;
    pl.shape = split ? LSQ_W8_SHAPE_TILES_SPLIT_K : LSQ_W8_SHAPE_TILES;
    pl.cols = split ? kW8Tile : 16 * kW8TileWaves;
    pl.ksplit = split ? kW8TileWaves : 1;
    pl.col_tiles = (N + pl.cols - 1) / pl.cols;
    pl.grid = pl.col_tiles <= INT64_MAX / pl.row_tiles ? pl.row_tiles * pl.col_tiles : INT64_MAX;
    pl.block = kW8TileWaves * 64;
    pl.lds = w8_tiles_lds(pl.subs);
    return pl;
}

template <int SUBS, bool SPLITK>
static hipError_t w8_launch_tiles(const W8Plan& pl, const W8Act& act, const W8Weight& wt, const W8Geom& geo, void* y, int y_dtype,
                                  hipStream_t stream) {
    static_assert(w8_tiles_lds(SUBS) <= 64 * 1024, "the tile fits the LDS a kernel gets unasked");
    static_assert(kW8TileWaves * SUBS * 64 * 16 <= SUBS * 16 * kW8TileStride, "the split-K tiles fit the staging area");
    hipLaunchKernelGGL((qlinear_w8_tiles_kernel<SUBS, SPLITK>), dim3(static_cast<unsigned>(pl.grid)), dim3(kW8TileWaves * 64), pl.lds,
                       stream, act, wt, geo, y, y_dtype);
    return hipGetLastError();
}

template <bool SPLITK>
static hipError_t w8_subs(const W8Plan& pl, const W8Act& act, const W8Weight& wt, const W8Geom& geo, void* y, int y_dtype, hipStream_t s) {
    if (pl.subs == 2) return w8_launch_tiles<2, SPLITK>(pl, act, wt, geo, y, y_dtype, s);
    if (pl.subs == 4) return w8_launch_tiles<4, SPLITK>(pl, act, wt, geo, y, y_dtype, s);
    return w8_launch_tiles<kW8MaxSubs, SPLITK>(pl, act, wt, geo, y, y_dtype, s);
}

static hipError_t w8_launch(const W8Plan& pl, const W8Act& act, const W8Weight& wt, int64_t M, int64_t N, int64_t K, void* y, int y_dtype,
                            hipStream_t stream) {
    if (pl.shape == LSQ_W8_SHAPE_GENERIC) {
        hipLaunchKernelGGL(qlinear_w8_generic_kernel, dim3(static_cast<unsigned>(pl.grid)), dim3(kBlock), 0, stream, act, M, wt, N, K, y,
                           y_dtype);
        return hipGetLastError();
    }
    if (pl.shape == LSQ_W8_SHAPE_DECODE) {
        static LdsOnce once;
        if (const hipError_t e = allow_lds(once, reinterpret_cast<const void*>(&qlinear_w8_decode_kernel), kW8MaxDecodeLds)) return e;
        hipLaunchKernelGGL(qlinear_w8_decode_kernel, dim3(static_cast<unsigned>(pl.grid)), dim3(kW8Block), pl.lds, stream, act,
                           static_cast<int>(M), wt, N, K, pl.row_stride, y, y_dtype);
        return hipGetLastError();
    }
    const W8Geom geo{M, N, K, pl.row_tiles};
    return pl.shape == LSQ_W8_SHAPE_TILES_SPLIT_K ? w8_subs<true>(pl, act, wt, geo, y, y_dtype, stream)
                                                  : w8_subs<false>(pl, act, wt, geo, y, y_dtype, stream);
}

template <typename IO>
static hipError_t w8_levels(const void* x, int64_t n, const W8Act& act, void* ws, hipStream_t stream) {
    const int64_t cus = device_info().cu_count;
    const int64_t turns = (n + 15) / 16;
    const int grid = static_cast<int>(std::min(std::max<int64_t>(1, (turns + kBlock - 1) / kBlock), cus * 8));
    hipLaunchKernelGGL((qlinear_w8_levels_kernel<IO>), dim3(grid), dim3(kBlock), 0, stream, x, n, act.scale, act.shift, act.qmin, act.qmax,
                       act.tmin, act.tmax, act.off, static_cast<uint8_t*>(ws));
    return hipGetLastError();
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_qlinear_w8.h: validation, dtype dispatch, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

int check_w8_shape(int dtype, int64_t M, int64_t N, int64_t K, const char* what) {
    if (dtype == LSQ_F64) return fail(LSQ_EINVAL, "%s: float64 is not supported (the kernel computes in integers and float32)", what);
    if (dtype != LSQ_F32 && dtype != LSQ_BF16 && dtype != LSQ_F16) return fail(LSQ_EINVAL, "%s: unknown dtype code %d", what, dtype);
    const long long m = M, n = N, k = K;
    if (N < 0 || K < 0) return fail(LSQ_EINVAL, "%s: negative weight shape [%lld, %lld]", what, n, k);
    if (M < 1) return fail(LSQ_EINVAL, "%s: M = %lld rows of x, at least 1 is needed", what, m);
    if (M > INT64_MAX / std::max<int64_t>(1, std::max(N, K)) / 4 || N > INT64_MAX / std::max<int64_t>(1, K))
        return fail(LSQ_EINVAL, "%s: M = %lld rows of x on a [%lld, %lld] weight are beyond 64-bit offsets", what, m, n, k);
    return LSQ_OK;
}

int check_w8_level_dtype(const char* what, const char* name, int code) {
    if (code != LSQ_W8_U8 && code != LSQ_W8_I8)
        return fail(LSQ_EINVAL, "%s: %s must be LSQ_W8_U8 (0) or LSQ_W8_I8 (1), got %d", what, name, code);
    return LSQ_OK;
}

int check_w8_weights(const char* what, int y_dtype, int w_level_dtype, const void* w_levels, const void* w_scale, const void* w_zero,
                     const void* bias, int bias_dtype, const void* y) {
    if (int rc = check_w8_level_dtype(what, "w_level_dtype", w_level_dtype)) return rc;
    if (!w_levels || !w_scale || !w_zero || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (bias && bias_dtype != LSQ_F32 && bias_dtype != y_dtype)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of y's type, got dtype code %d", what, bias_dtype);
    if (!aligned_to(y, elem_bytes(y_dtype))) return fail(LSQ_EINVAL, "%s: x and y must be element-aligned", what);
    if (!aligned_to(w_scale, 4) || !aligned_to(w_zero, 4) || (bias && !aligned_to(bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: w_scale, w_zero and bias must be element-aligned", what);
    return LSQ_OK;
}

int checked_plan(const char* what, lsq::W8Plan& pl, int64_t M, int64_t N, int64_t K, bool aligned) {
    pl = lsq::plan_w8(M, N, K, aligned);
    if (pl.grid > INT32_MAX)
        return fail(LSQ_EINVAL, "%s: %lld row tiles by %lld column tiles are beyond a 31-bit grid", what,
                    static_cast<long long>(pl.row_tiles), static_cast<long long>(pl.col_tiles));
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_qlinear_w8_abi_version(void) { return LSQ_QLINEAR_W8_ABI_VERSION; }

const char* lsq_qlinear_w8_last_error(void) { return g_last_error; }

int lsq_qlinear_w8_forward_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, int w_level_dtype,
                                  const void* w_levels, int64_t N, int64_t K, const void* w_scale, const void* w_zero, const void* bias,
                                  int bias_dtype, void* y, int y_dtype, void* stream) {
    const char* what = "lsq_qlinear_w8_forward_levels";
    if (int rc = check_w8_shape(y_dtype, M, N, K, what)) return rc;
    if (int rc = check_w8_level_dtype(what, "level_dtype", level_dtype)) return rc;
    if (!x_levels || !s_x || !zx) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (int rc = check_w8_weights(what, y_dtype, w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype, y)) return rc;
    if (!aligned_to(s_x, 4) || !aligned_to(zx, 4)) return fail(LSQ_EINVAL, "%s: s_x and zx must be element-aligned", what);
    lsq::W8Plan pl;
    if (int rc = checked_plan(what, pl, M, N, K, aligned_to(w_levels, 16))) return rc;
    if (N == 0) return LSQ_OK;
    lsq::W8Act act{};
    act.a = static_cast<const uint8_t*>(x_levels);
    act.scale = static_cast<const float*>(s_x);
    act.zx = static_cast<const int32_t*>(zx);
    act.off = level_dtype == LSQ_W8_U8 ? 128 : 0;
    act.fused = 0;
    act.aligned = (aligned_to(x_levels, 16) && K % 16 == 0) ? 1 : 0;
    const lsq::W8Weight wt{static_cast<const uint8_t*>(w_levels), static_cast<const float*>(w_scale), static_cast<const int32_t*>(w_zero),
                           bias, bias_dtype, w_level_dtype == LSQ_W8_U8 ? 128 : 0};
    return hip_status(lsq::w8_launch(pl, act, wt, M, N, K, y, y_dtype, static_cast<hipStream_t>(stream)), what);
}

int lsq_qlinear_w8_forward(int dtype, const void* x, int64_t M, const void* scale, const void* shift, int64_t quant_min,
                           int64_t quant_max, int64_t type_min, int64_t type_max, int w_level_dtype, const void* w_levels, int64_t N,
                           int64_t K, const void* w_scale, const void* w_zero, const void* bias, int bias_dtype, void* y, void* levels_ws,
                           void* stream) {
    const char* what = "lsq_qlinear_w8_forward";
    if (int rc = check_w8_shape(dtype, M, N, K, what)) return rc;
    const long long lo = std::min(quant_min, type_min), hi = std::max(quant_max, type_max);
    if (quant_min > quant_max || type_min > type_max || !((lo >= 0 && hi <= 255) || (lo >= -128 && hi <= 127)))
        return fail(LSQ_EINVAL, "%s: [quant_min, quant_max] = [%lld, %lld] and [type_min, type_max] = [%lld, %lld] must lie within "
                    "0..255 or within -128..127", what, static_cast<long long>(quant_min), static_cast<long long>(quant_max),
                    static_cast<long long>(type_min), static_cast<long long>(type_max));
    if (!x || !scale || !shift) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (int rc = check_w8_weights(what, dtype, w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype, y)) return rc;
    if (!aligned_to(x, elem_bytes(dtype))) return fail(LSQ_EINVAL, "%s: x and y must be element-aligned", what);
    if (!aligned_to(scale, 4) || !aligned_to(shift, 4))
        return fail(LSQ_EINVAL, "%s: scale and shift must be element-aligned", what);
    lsq::W8Plan pl;
    if (int rc = checked_plan(what, pl, M, N, K, aligned_to(w_levels, 16))) return rc;
    if (!levels_ws || !aligned_to(levels_ws, 16))
        return fail(LSQ_EINVAL, "%s: levels_ws must be a 16-byte aligned device buffer of M * K bytes", what);
    if (N == 0) return LSQ_OK;
    lsq::W8Act act{};
    act.a = static_cast<const uint8_t*>(levels_ws);
    act.scale = static_cast<const float*>(scale);
    act.shift = static_cast<const float*>(shift);
    act.qmin = static_cast<float>(quant_min);
    act.qmax = static_cast<float>(quant_max);
    act.tmin = static_cast<float>(type_min);
    act.tmax = static_cast<float>(type_max);
    act.off = hi > 127 ? 128 : 0;
    act.fused = 1;
    act.aligned = K % 16 == 0 ? 1 : 0;
    const lsq::W8Weight wt{static_cast<const uint8_t*>(w_levels), static_cast<const float*>(w_scale), static_cast<const int32_t*>(w_zero),
                           bias, bias_dtype, w_level_dtype == LSQ_W8_U8 ? 128 : 0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    if (K > 0) {
        switch (dtype) {
            case LSQ_BF16: e = lsq::w8_levels<lsq::io_bf16>(x, M * K, act, levels_ws, s); break;
            case LSQ_F16: e = lsq::w8_levels<lsq::io_f16>(x, M * K, act, levels_ws, s); break;
            default: e = lsq::w8_levels<lsq::io_f32>(x, M * K, act, levels_ws, s); break;
        }
    }
    if (e != hipSuccess) return hip_status(e, what);
    return hip_status(lsq::w8_launch(pl, act, wt, M, N, K, y, dtype, s), what);
}

int lsq_qlinear_w8_plan(int64_t M, int64_t N, int64_t K, int w_aligned, int32_t* out8) {
    const char* what = "lsq_qlinear_w8_plan";
    if (int rc = check_w8_shape(LSQ_F32, M, N, K, what)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    lsq::W8Plan pl;
    if (int rc = checked_plan(what, pl, M, N, K, w_aligned != 0)) return rc;
    out8[0] = pl.form;
    out8[1] = pl.shape;
    out8[2] = static_cast<int32_t>(pl.grid);
    out8[3] = pl.block;
    out8[4] = pl.rows;
    out8[5] = pl.cols;
    out8[6] = pl.lds;
    out8[7] = pl.ksplit;
    return LSQ_OK;
}

}  // extern "C"
