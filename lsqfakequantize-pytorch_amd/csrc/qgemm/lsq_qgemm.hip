// lsq_qgemm.hip -- y = x @ w^T (+ bias) on packed 4- / 2-bit group-wise weights for any number of rows of x on gfx950
// (include/lsq_hip_qgemm.h, which states the contract and the arithmetic; the weight format is include/lsq_hip_pack.h's):
// the kernel and the C ABI of liblsq_hip_qgemm.so.  It borrows the pieces of the decode kernel that do not depend on how
// K is split -- the 16-byte code loads, the 4 x 4 transpose over the lanes, the per-packet scales (qlinear/lsq_qdecode.hpp)
// -- and is otherwise a tiled GEMM:
//  * TILES.  A workgroup owns kGRows = 128 rows of x by 16 * WAVES columns; wave w owns columns 16 w .. 16 w + 15 of the
//    tile and all its rows.  WAVES is 4, or 1 while 64-column tiles would not give every compute unit a tile (plan_qgemm).
//    SUBS is the number of 16-row sub-tiles a workgroup computes: 8, or 4 / 2 when all of M is at most 64 / 32 rows (one
//    row tile, which then has no more).
//    blockIdx.x = column tile * row tiles + row tile: the workgroups that read the same codes are neighbours.
//  * MAIN LOOP.  One step is 4 code packets of 16 bytes = KS = 4 * BE consecutive k (BE = 128 / bits).  The workgroup
//    stages x[rows of the tile, KS] in LDS (rows kQRowPad bytes further apart than their data; the rows beyond M are
//    zero); lane (n, q) of a wave has loaded packet 4 s + q of its column n one step ahead, and the
//    wave transposes the 4 x 4 dwords over its lanes (transpose_over_rows) so that the k of one MFMA lie in one packet.
//  * B REUSE.  Per packet the wave unpacks ONE B fragment (two at 2 bits) -- the integer code - qzero as bf16 / fp16, or
//    its three exact 8-bit pieces when a qzero of the wave's 16 columns lies beyond +-128 -- and runs it against the A
//    fragment of each of the SUBS 16-row sub-tiles (16 bytes per lane from LDS): up to 8 MFMAs per unpack.
//  * ORDER OF THE SUM.  Each output has one fp32 chain: the MFMAs of a group's packets in ascending k accumulate into
//    `part`; at the group's last packet acc = fma(part, qscale, acc).  K is never split, and nothing above depends on M,
//    WAVES or the row's place.  Bias in fp32, one rounding.
//  * RAGGED EDGES.  A column beyond N reads the codes of row N - 1 and stores nothing; rows beyond M are zero
//    operands and not stored; packets beyond K are not touched.
#include "../qlinear/lsq_qdecode.hpp"
#include "../../../include/lsq_hip_qgemm.h"

#include <climits>

namespace lsq {

constexpr int kGRows = 128;                         // rows of x per tile
constexpr int kGSub = kGRows / 16;                  // 16-row sub-tiles: MFMAs per unpacked B fragment
constexpr int kGWide = 4;                           // waves (16 columns each) of the wide tile

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

template <typename IO> struct GemmOp;
template <> struct GemmOp<io_bf16> {
    typedef bf16x8 vec;
    __device__ static __forceinline__ f32x4 mfma(vec a, vec b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct GemmOp<io_f16> {
    typedef f16x8 vec;
    __device__ static __forceinline__ f32x4 mfma(vec a, vec b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

// the j-th of the 8 codes of MFMA h of one dword
template <int BITS>
__device__ __forceinline__ int gemm_code_at(uint32_t w, int h, int j) {
    return static_cast<int>((w >> (h * 8 * BITS + j * BITS)) & ((1u << BITS) - 1u));
}

// bytes between rows of x in LDS
constexpr int gemm_row_stride(int bits) { return 4 * (128 / bits) * 2 + kQRowPad; }

// ppg: 16-byte packets per group (ppg_shift, ppg_div: the same for the group index of a packet)
template <typename IO, int BITS, int WAVES, int SUBS>
__global__ __launch_bounds__(WAVES * 64, 2) void qgemm_kernel(const void* __restrict__ x, int64_t M, const uint8_t* __restrict__ codes,
                                                          int64_t N, int64_t K, int64_t n_groups, int64_t ppg, int ppg_shift,
                                                          DivU64 ppg_div, int64_t row_tiles, const float* __restrict__ qscale,
                                                          const int32_t* __restrict__ qzero, const void* __restrict__ bias,
                                                          int bias_f32, void* __restrict__ y) {
    using OP = GemmOp<IO>;
    using Vec = typename OP::vec;
    constexpr int D = 32 / BITS;                    // elements per dword
    constexpr int BE = 4 * D;                       // elements per 16-byte packet
    constexpr int H = D / 8;                        // MFMAs per dword
    constexpr int KS = 4 * BE;                      // elements of K per step
    constexpr int XP = KS / 8;                      // 16-byte packets of x per row and step
    constexpr int kStride = gemm_row_stride(BITS);
    constexpr int kThreads = WAVES * 64;
    constexpr int kIters = SUBS * 16 * XP / kThreads;       // 16-byte packets of x per lane and step
    constexpr int kBatch = kIters < 8 ? kIters : 8;
    static_assert(kIters * kThreads == SUBS * 16 * XP && kIters % kBatch == 0, "the lanes share a step's packets of x evenly");
    extern __shared__ __attribute__((aligned(16))) unsigned char xs[];

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const int64_t tile = static_cast<int64_t>(blockIdx.x);
    const int64_t col_tile = tile / row_tiles, row_tile = tile - col_tile * row_tiles;
    const int64_t m0 = row_tile * kGRows;
    const int rows = static_cast<int>(std::min<int64_t>(kGRows, M - m0));      // >= 1
    const int64_t n0 = (col_tile * WAVES + wave) * 16;
    const int64_t row = std::min<int64_t>(n0 + nl, N - 1);                      // a clamped row computes a value nobody stores
    const int64_t n_packets = K / BE;               // per row; exact
    const int64_t steps = (n_packets + 3) / 4;
    const uint8_t* __restrict__ wrow = codes + row * (n_packets * 16);
    const float* __restrict__ qs_row = qscale + row * n_groups;
    const int32_t* __restrict__ qz_row = qzero + row * n_groups;

    f32x4 acc[SUBS], part[SUBS];
#pragma unroll
    for (int rt = 0; rt < SUBS; ++rt) {
        acc[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        part[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    int64_t rem = ppg;                              // packets left in the current group

    // the first step's codes and scales
    u32x4 raw_next = {0u, 0u, 0u, 0u};
    float qs_next[4];
    int32_t qz_next[4];
    if (q < n_packets) raw_next = load_code_packet(wrow, q);
#pragma unroll
    for (int t = 0; t < 4; ++t) load_packet_scale(qs_row, qz_row, t, n_packets, ppg_shift, ppg_div, qs_next[t], qz_next[t]);

    for (int64_t s = 0; s < steps; ++s) {
        const int64_t k0 = s * KS;
        const int ppr = static_cast<int>(std::min<int64_t>(KS, K - k0) / 8);   // 16-byte packets of x per row; exact, BE % 8 == 0
        __syncthreads();                            // the previous step's reads of xs are done
        // kBatch loads in flight per lane, then their LDS stores: one load at a time would pay its latency kIters times
#pragma unroll 1
        for (int it0 = 0; it0 < kIters; it0 += kBatch) {
            Packet<IO> pk[kBatch];
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                const int p = tid + (it0 + b) * kThreads, m = p / XP, i = p % XP;
                __builtin_memset(&pk[b], 0, 16);
                if (i < ppr && m < rows) pk[b] = load_packet<IO>(x, (m0 + m) * K + k0 + static_cast<int64_t>(i) * 8);
            }
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                const int p = tid + (it0 + b) * kThreads, m = p / XP, i = p % XP;
                if (i < ppr) *reinterpret_cast<Packet<IO>*>(xs + m * kStride + i * 16) = pk[b];
            }
        }
        __syncthreads();

        uint32_t r[4] = {raw_next.x, raw_next.y, raw_next.z, raw_next.w};
        float qsv[4];
        int32_t qzv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            qsv[t] = qs_next[t];
            qzv[t] = qz_next[t];
        }
        // the next step's codes and scales, in flight during this step's MFMAs
        {
            const int64_t pn = (s + 1) * 4;
            raw_next = u32x4{0u, 0u, 0u, 0u};
            if (pn + q < n_packets) raw_next = load_code_packet(wrow, pn + q);
#pragma unroll
            for (int t = 0; t < 4; ++t) load_packet_scale(qs_row, qz_row, pn + t, n_packets, ppg_shift, ppg_div, qs_next[t], qz_next[t]);
        }
        transpose_over_rows(r);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (s * 4 + t < n_packets) {            // the same for the whole workgroup
                const int32_t qz = qzv[t];
                const bool far = qz < -128 || qz > 128;
                const unsigned char* xa = xs + nl * kStride + (t * BE + q * D) * 2;   // this dword's first element, row nl
                if (__ballot(far) == 0) {
                    Vec b[H];
#pragma unroll
                    for (int h = 0; h < H; ++h)
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            b[h][j] = static_cast<typename IO::elem>(static_cast<float>(gemm_code_at<BITS>(r[t], h, j) - qz));
#pragma unroll
                    for (int rt = 0; rt < SUBS; ++rt) {
#pragma unroll
                        for (int h = 0; h < H; ++h) {
                            Vec a;
                            const u32x4 ax = *reinterpret_cast<const u32x4*>(xa + rt * 16 * kStride + h * 16);
                            __builtin_memcpy(&a, &ax, 16);
                            part[rt] = OP::mfma(a, b[h], part[rt]);
                        }
                    }
                } else {
                    // |code - qzero| in three exact pieces of 8 bits, each with the sign: exact operands, three exact tiles
                    Vec b0[H], b1[H], b2[H];
#pragma unroll
                    for (int h = 0; h < H; ++h)
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int64_t d = static_cast<int64_t>(gemm_code_at<BITS>(r[t], h, j)) - qz;
                            const int64_t mag = d < 0 ? -d : d;
                            const float sgn = d < 0 ? -1.0f : 1.0f;
                            b0[h][j] = static_cast<typename IO::elem>(sgn * static_cast<float>(static_cast<int>(mag & 0xff)));
                            b1[h][j] = static_cast<typename IO::elem>(sgn * static_cast<float>(static_cast<int>((mag >> 8) & 0xff)));
                            b2[h][j] = static_cast<typename IO::elem>(sgn * static_cast<float>(mag >> 16));
                        }
#pragma unroll
                    for (int rt = 0; rt < SUBS; ++rt) {
                        f32x4 p1 = {0.0f, 0.0f, 0.0f, 0.0f}, p2 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int h = 0; h < H; ++h) {
                            Vec a;
                            const u32x4 ax = *reinterpret_cast<const u32x4*>(xa + rt * 16 * kStride + h * 16);
                            __builtin_memcpy(&a, &ax, 16);
                            part[rt] = OP::mfma(a, b0[h], part[rt]);
                            p1 = OP::mfma(a, b1[h], p1);
                            p2 = OP::mfma(a, b2[h], p2);
                        }
                        part[rt] = part[rt] + (p1 * 256.0f + p2 * 65536.0f);
                    }
                }
                if (--rem == 0) {                   // the group's last packet: fold its partial tile in
                    rem = ppg;
                    const float qs = qsv[t];
#pragma unroll
                    for (int rt = 0; rt < SUBS; ++rt) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[rt][e] = __builtin_fmaf(part[rt][e], qs, acc[rt][e]);
                        part[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);      // one packet's LDS reads at a time: the registers of four would spill
        }
    }

    // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
    const int64_t n = n0 + nl;
    if (n < N) {
        const float b = bias_at<IO>(bias, bias_f32, n);
#pragma unroll
        for (int rt = 0; rt < SUBS; ++rt) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = rt * 16 + q * 4 + e;
                if (m < rows) store_out<IO, false>(y, (m0 + m) * N + n, acc[rt][e] + b);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launcher
// ------------------------------------------------------------------------------------------------
struct QGemmPlan {
    const char* unserved;           // NULL: served on the matrix cores; else why not
    int waves, subs, lds, ks;
    int64_t row_tiles, col_tiles, grid, packets_per_group;
};

inline QGemmPlan plan_qgemm(int dtype, int64_t M, int64_t N, int64_t K, int64_t G, int bits) {
    QGemmPlan pl = {};
    const int64_t packet_elems = 128 / bits;
    if (dtype != LSQ_BF16 && dtype != LSQ_F16) {
        pl.unserved = "float32 x is not served (the matrix-core GEMM takes bfloat16 / float16 x)";
        return pl;
    }
    if (G % packet_elems != 0) {
        pl.unserved = "group_size is not a multiple of the 128 / bits elements of one 16-byte code packet";
        return pl;
    }
    const int64_t cus = device_info().cu_count;
    pl.row_tiles = (M + kGRows - 1) / kGRows;
    const int64_t wide = (N + 16 * kGWide - 1) / (16 * kGWide);
    // 64-column tiles once they give every compute unit a tile; below that 16-column tiles, four times as many
    pl.waves = (wide <= INT64_MAX / pl.row_tiles && pl.row_tiles * wide < cus) ? 1 : kGWide;
    pl.col_tiles = (N + 16 * pl.waves - 1) / (16 * pl.waves);
    pl.grid = pl.col_tiles <= INT64_MAX / pl.row_tiles ? pl.row_tiles * pl.col_tiles : INT64_MAX;
    pl.ks = static_cast<int>(4 * packet_elems);
    pl.subs = M <= 32 ? 2 : (M <= 64 ? 4 : kGSub);
    pl.lds = pl.subs * 16 * gemm_row_stride(bits);
    pl.packets_per_group = G / packet_elems;
    return pl;
}

template <typename IO, int BITS, int WAVES, int SUBS>
static hipError_t qgemm_launch(const QGemmPlan& pl, const void* x, int64_t M, const void* codes, int64_t N, int64_t K, int64_t G,
                               const void* qscale, const void* qzero, const void* bias, int bias_f32, void* y, hipStream_t stream) {
    static LdsOnce once;            // the full 2-bit tile is beyond the 64 KiB a kernel gets unasked
    if (const hipError_t e = allow_lds(once, reinterpret_cast<const void*>(&qgemm_kernel<IO, BITS, WAVES, SUBS>),
                                       SUBS * 16 * gemm_row_stride(BITS)))
        return e;
    hipLaunchKernelGGL((qgemm_kernel<IO, BITS, WAVES, SUBS>), dim3(static_cast<unsigned>(pl.grid)), dim3(WAVES * 64), pl.lds, stream, x,
                       M, static_cast<const uint8_t*>(codes), N, K, K / G, pl.packets_per_group, log2_exact(pl.packets_per_group),
                       make_div(pl.packets_per_group), pl.row_tiles, static_cast<const float*>(qscale),
                       static_cast<const int32_t*>(qzero), bias, bias_f32, y);
    return hipGetLastError();
}

template <typename IO, int BITS, int WAVES>
static hipError_t qgemm_subs(const QGemmPlan& pl, const void* x, int64_t M, const void* codes, int64_t N, int64_t K, int64_t G,
                             const void* qscale, const void* qzero, const void* bias, int bias_f32, void* y, hipStream_t stream) {
#define ARGS (pl, x, M, codes, N, K, G, qscale, qzero, bias, bias_f32, y, stream)
    if (pl.subs == 2) return qgemm_launch<IO, BITS, WAVES, 2> ARGS;
    if (pl.subs == 4) return qgemm_launch<IO, BITS, WAVES, 4> ARGS;
    return qgemm_launch<IO, BITS, WAVES, kGSub> ARGS;
#undef ARGS
}

template <typename IO, int BITS>
static hipError_t qgemm_waves(const QGemmPlan& pl, const void* x, int64_t M, const void* codes, int64_t N, int64_t K, int64_t G,
                              const void* qscale, const void* qzero, const void* bias, int bias_f32, void* y, hipStream_t stream) {
    return pl.waves == 1 ? qgemm_subs<IO, BITS, 1>(pl, x, M, codes, N, K, G, qscale, qzero, bias, bias_f32, y, stream)
                         : qgemm_subs<IO, BITS, kGWide>(pl, x, M, codes, N, K, G, qscale, qzero, bias, bias_f32, y, stream);
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_qgemm.h: validation, dtype dispatch, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// the shape of a call: lsq_qdecode.hpp's check_shape with the GEMM's row rule
int check_gemm_shape(int dtype, int64_t M, int64_t N, int64_t K, int64_t G, int bits, const char* what) {
    if (dtype == LSQ_F64)
        return fail(LSQ_EINVAL, "%s: float64 is not supported (a packed weight with a float64 scale has no GPU linear)", what);
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
    if (M > INT64_MAX / std::max<int64_t>(1, std::max(N, K)) || N > INT64_MAX / std::max<int64_t>(1, K))
        return fail(LSQ_EINVAL, "%s: M = %lld rows of x on a [%lld, %lld] weight are beyond 64-bit offsets", what, m, n, k);
    return LSQ_OK;
}

int check_grid(const lsq::QGemmPlan& pl, const char* what) {
    if (pl.grid > INT32_MAX)
        return fail(LSQ_EINVAL, "%s: %lld row tiles by %lld column tiles are beyond a 31-bit grid", what,
                    static_cast<long long>(pl.row_tiles), static_cast<long long>(pl.col_tiles));
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_qgemm_abi_version(void) { return LSQ_QGEMM_ABI_VERSION; }

const char* lsq_qgemm_last_error(void) { return g_last_error; }

int lsq_qgemm_forward(int dtype, const void* x, int64_t M, const void* codes, int64_t N, int64_t K, int64_t group_size, int bits,
                      const void* qscale, const void* qzero, const void* bias, int bias_dtype, void* y, void* stream) {
    const char* what = "lsq_qgemm_forward";
    if (int rc = check_gemm_shape(dtype, M, N, K, group_size, bits, what)) return rc;
    if (!x || !codes || !qscale || !qzero || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (bias && bias_dtype != LSQ_F32 && bias_dtype != dtype)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of x's type, got dtype code %d", what, bias_dtype);
    if (!aligned_to(x, elem_bytes(dtype)) || !aligned_to(y, elem_bytes(dtype)))
        return fail(LSQ_EINVAL, "%s: x and y must be element-aligned", what);
    if (!aligned_to(qscale, 4) || !aligned_to(qzero, 4) || (bias && !aligned_to(bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: qscale, qzero and bias must be element-aligned", what);
    if (N == 0) return LSQ_OK;
    const lsq::QGemmPlan pl = lsq::plan_qgemm(dtype, M, N, K, group_size, bits);
    if (pl.unserved) return fail(LSQ_EINVAL, "%s: not served: %s (dequantize and call a GEMM)", what, pl.unserved);
    if (!aligned_to(codes, 16))
        return fail(LSQ_EINVAL, "%s: not served: codes are not 16-byte aligned (dequantize and call a GEMM)", what);
    if (int rc = check_grid(pl, what)) return rc;
    const int bias_f32 = bias_dtype == LSQ_F32 ? 1 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
#define ARGS (pl, x, M, codes, N, K, group_size, qscale, qzero, bias, bias_f32, y, s)
    if (dtype == LSQ_BF16)
        e = bits == 4 ? lsq::qgemm_waves<lsq::io_bf16, 4> ARGS : lsq::qgemm_waves<lsq::io_bf16, 2> ARGS;
    else
        e = bits == 4 ? lsq::qgemm_waves<lsq::io_f16, 4> ARGS : lsq::qgemm_waves<lsq::io_f16, 2> ARGS;
#undef ARGS
    return hip_status(e, what);
}

int lsq_qgemm_plan(int dtype, int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int32_t* out8) {
    const char* what = "lsq_qgemm_plan";
    if (int rc = check_gemm_shape(dtype, M, N, K, group_size, bits, what)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    const lsq::QGemmPlan pl = lsq::plan_qgemm(dtype, M, N, K, group_size, bits);
    if (pl.unserved) return LSQ_OK;
    if (int rc = check_grid(pl, what)) return rc;
    out8[0] = 1;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.waves * 64;
    out8[3] = lsq::kGRows;
    out8[4] = 16 * pl.waves;
    out8[5] = pl.lds;
    out8[6] = pl.ks;
    return LSQ_OK;
}

}  // extern "C"
