// lsq_qlinear.hip -- y = x @ w^T (+ bias) on packed 4- / 2-bit group-wise weights for up to 16 rows of x on gfx950
// (include/lsq_hip_qlinear.h, which states the arithmetic contract; the weight format is include/lsq_hip_pack.h's): the
// kernels and the C ABI of liblsq_hip_qlinear.so.  lsq_qdecode.hpp has the design both decode linears share -- tile
// ownership, K split by wave, the transpose, the order of the sum -- and its pieces; particular to float x:
//  * MATRIX-CORE form (bf16 / fp16 x, G a multiple of the BE = 128 / bits elements of one 16-byte code packet, codes 16-byte
//    aligned).  Load step s of a chunk belongs to wave s % 16: 2 steps per wave in flight at 4 bits, 1 at 2 bits, issued
//    before x is staged.  x is the A operand of mfma_f32_16x16x32 (row m = lane & 15), 16 bytes per lane and MFMA read
//    from LDS, where it is staged as it is in chunks of 4096 k; rows m >= M are zero registers.  The B operand is the
//    integer code - qzero as bf16 / fp16 -- exact for -128 <= qzero <= 128; a packet where any of the wave's 16 rows has a
//    qzero beyond that splits |code - qzero| into three exact 8-bit pieces and runs three MFMAs (the format allows
//    +-2^23).  The packet's fp32 partial tile is folded into the accumulator with one multiply by the column's qscale.
//    After the sum over the waves the bias is added in fp32, and the result is rounded once.
//  * GENERIC form (fp32 x, any other G, misaligned codes): one code byte per lane and step, w = float(code - qzero) * qscale
//    and one fp32 multiply-add per (row of x, element), a butterfly over the wave.
#include "lsq_qdecode.hpp"

namespace lsq {

constexpr int kQRowStride = kQChunk * 2 + kQRowPad; // bytes between rows of x in LDS

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

template <typename IO> struct MatOp;
template <> struct MatOp<io_bf16> {
    typedef bf16x8 vec;
    __device__ static __forceinline__ f32x4 mfma(vec a, vec b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct MatOp<io_f16> {
    typedef f16x8 vec;
    __device__ static __forceinline__ f32x4 mfma(vec a, vec b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

// the j-th of the 8 codes of MFMA h of one dword
template <int BITS>
__device__ __forceinline__ int code_at(uint32_t w, int h, int j) {
    return static_cast<int>((w >> (h * 8 * BITS + j * BITS)) & ((1u << BITS) - 1u));
}

// ------------------------------------------------------------------------------------------------
// matrix-core form
// ------------------------------------------------------------------------------------------------
// bpg: 16-byte packets per group (shift when a power of two, else the division)
template <typename IO, int BITS>
__global__ __launch_bounds__(kQBlock) void qlinear_mfma_kernel(const void* __restrict__ x, int M, const uint8_t* __restrict__ codes,
                                                              int64_t N, int64_t K, int64_t n_groups, int bpg_shift, DivU64 bpg,
                                                              const float* __restrict__ qscale, const int32_t* __restrict__ qzero,
                                                              const void* __restrict__ bias, int bias_f32, void* __restrict__ y) {
    using OP = MatOp<IO>;
    using Vec = typename OP::vec;
    constexpr int D = 32 / BITS;                    // elements per dword
    constexpr int BE = 4 * D;                       // elements per 16-byte packet
    constexpr int H = D / 8;                        // MFMAs per dword
    constexpr int U = BITS == 4 ? 2 : 1;            // steps per wave and chunk
    constexpr int kSteps = kQWaves * U;             // steps per chunk
    static_assert(kSteps * 4 * BE == kQChunk, "a chunk of x is what the waves' steps cover");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);
    unsigned char* xs = smem + kQRedBytes;

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const int64_t n_packets = K / BE;               // per row; exact
    const int64_t row_bytes = n_packets * 16;
    const int64_t n_chunks = (K + kQChunk - 1) / kQChunk;
    const int64_t tiles = (N + kQTile - 1) / kQTile;
    const int64_t first_tile = static_cast<int64_t>(blockIdx.x);

    for (int64_t tile = first_tile; tile < tiles; tile += static_cast<int64_t>(gridDim.x)) {
        const int64_t row = std::min<int64_t>(tile * kQTile + nl, N - 1);          // a clamped row computes a value nobody stores
        const uint8_t* __restrict__ wrow = codes + row * row_bytes;
        const float* __restrict__ qs_row = qscale + row * n_groups;
        const int32_t* __restrict__ qz_row = qzero + row * n_groups;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int64_t c = 0; c < n_chunks; ++c) {
            const int64_t kc0 = c * kQChunk;
            u32x4 raw[U];
            float qsv[U][4];
            int32_t qzv[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t p0 = (c * kSteps + u * kQWaves + wave) * 4;
                raw[u] = u32x4{0u, 0u, 0u, 0u};
                if (p0 + q < n_packets) raw[u] = load_code_packet(wrow, p0 + q);
#pragma unroll
                for (int t = 0; t < 4; ++t) load_packet_scale(qs_row, qz_row, p0 + t, n_packets, bpg_shift, bpg, qsv[u][t], qzv[u][t]);
            }
            if (n_chunks > 1 || tile == first_tile) {       // x stays in LDS across tiles when one chunk holds it
                __syncthreads();
                const int64_t kc_len = std::min<int64_t>(kQChunk, K - kc0);
                const int ppr = static_cast<int>(kc_len / 8);       // 16-byte packets of x per row; exact, BE % 8 == 0
                for (int p = tid; p < M * (kQChunk / 8); p += kQBlock) {
                    const int m = p / (kQChunk / 8), i = p % (kQChunk / 8);
                    if (i < ppr) {
                        const Packet<IO> pk = load_packet<IO>(x, static_cast<int64_t>(m) * K + kc0 + static_cast<int64_t>(i) * 8);
                        *reinterpret_cast<Packet<IO>*>(xs + m * kQRowStride + i * 16) = pk;
                    }
                }
                __syncthreads();
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t p0 = (c * kSteps + u * kQWaves + wave) * 4;
                uint32_t r[4] = {raw[u].x, raw[u].y, raw[u].z, raw[u].w};
                transpose_over_rows(r);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (p0 + t >= n_packets) continue;      // the same for the whole wave
                    const int32_t qz = qzv[u][t];
                    const bool far = qz < -128 || qz > 128;
                    const int koff = static_cast<int>((p0 + t) * BE - kc0) + q * D;      // this dword's first element in the chunk
                    const unsigned char* xa = xs + nl * kQRowStride + koff * 2;
                    f32x4 part = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (__ballot(far) == 0) {
#pragma unroll
                        for (int h = 0; h < H; ++h) {
                            Vec a, b;
                            u32x4 ax = {0u, 0u, 0u, 0u};
                            if (nl < M) ax = *reinterpret_cast<const u32x4*>(xa + h * 16);
                            __builtin_memcpy(&a, &ax, 16);
#pragma unroll
                            for (int j = 0; j < 8; ++j)
                                b[j] = static_cast<typename IO::elem>(static_cast<float>(code_at<BITS>(r[t], h, j) - qz));
                            part = OP::mfma(a, b, part);
                        }
                    } else {
                        // |code - qzero| in three exact pieces of 8 bits, each with the sign: exact operands, three exact tiles
                        f32x4 p1 = {0.0f, 0.0f, 0.0f, 0.0f}, p2 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int h = 0; h < H; ++h) {
                            Vec a, b0, b1, b2;
                            u32x4 ax = {0u, 0u, 0u, 0u};
                            if (nl < M) ax = *reinterpret_cast<const u32x4*>(xa + h * 16);
                            __builtin_memcpy(&a, &ax, 16);
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                const int64_t d = static_cast<int64_t>(code_at<BITS>(r[t], h, j)) - qz;
                                const int64_t mag = d < 0 ? -d : d;
                                const float sgn = d < 0 ? -1.0f : 1.0f;
                                b0[j] = static_cast<typename IO::elem>(sgn * static_cast<float>(static_cast<int>(mag & 0xff)));
                                b1[j] = static_cast<typename IO::elem>(sgn * static_cast<float>(static_cast<int>((mag >> 8) & 0xff)));
                                b2[j] = static_cast<typename IO::elem>(sgn * static_cast<float>(mag >> 16));
                            }
                            part = OP::mfma(a, b0, part);
                            p1 = OP::mfma(a, b1, p1);
                            p2 = OP::mfma(a, b2, p2);
                        }
                        part = part + (p1 * 256.0f + p2 * 65536.0f);
                    }
                    acc = acc + part * qsv[u][t];
                }
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
            const int m = (l >> 4) * 4 + reg;               // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
            if (m < M && n < N) store_out<IO, false>(y, static_cast<int64_t>(m) * N + n, sum + bias_at<IO>(bias, bias_f32, n));
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// generic form
// ------------------------------------------------------------------------------------------------
// bytes_per_group: division by the code bytes of one group
template <typename IO, int BITS>
__global__ __launch_bounds__(kBlock) void qlinear_generic_kernel(const void* __restrict__ x, int M, const uint8_t* __restrict__ codes,
                                                                 int64_t N, int64_t K, int64_t n_groups, DivU64 bytes_per_group,
                                                                 const float* __restrict__ qscale, const int32_t* __restrict__ qzero,
                                                                 const void* __restrict__ bias, int bias_f32, void* __restrict__ y) {
    constexpr int PB = 8 / BITS;
    constexpr int R = kQGenericRowsAtOnce;
    constexpr uint32_t kMask = (1u << BITS) - 1u;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    const int64_t row_bytes = K / PB;
    for (int64_t n = wave; n < N; n += waves) {
        const uint8_t* __restrict__ wrow = codes + n * row_bytes;
        for (int m0 = 0; m0 < M; m0 += R) {
            float acc[R];
#pragma unroll
            for (int i = 0; i < R; ++i) acc[i] = 0.0f;
            for (int64_t b = lane; b < row_bytes; b += 64) {
                const int64_t g = n * n_groups + bytes_per_group.div(b);
                const float qs = qscale[g];
                const int64_t qz = qzero[g];
                const uint32_t byte = wrow[b];
#pragma unroll
                for (int j = 0; j < PB; ++j) {
                    const float w = static_cast<float>(static_cast<int64_t>((byte >> (j * BITS)) & kMask) - qz) * qs;
                    const int64_t k = b * PB + j;
#pragma unroll
                    for (int i = 0; i < R; ++i)
                        if (m0 + i < M) acc[i] = acc[i] + IO::load1(x, static_cast<int64_t>(m0 + i) * K + k) * w;
                }
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) acc[i] = acc[i] + __shfl_xor(acc[i], s, 64);
                if (lane == 0 && m0 + i < M)
                    store_out<IO, false>(y, static_cast<int64_t>(m0 + i) * N + n, acc[i] + bias_at<IO>(bias, bias_f32, n));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launchers
// ------------------------------------------------------------------------------------------------
struct QLinearPlan {
    bool mfma;
    int grid, block, lds, chunk, waves, cols;
    int64_t packets_per_group;      // matrix-core form
};

inline QLinearPlan plan_qlinear(int dtype, int64_t M, int64_t N, int64_t K, int64_t G, int bits) {
    QLinearPlan pl;
    const int64_t cus = device_info().cu_count;
    const int64_t packet_elems = 128 / bits;
    pl.mfma = (dtype == LSQ_BF16 || dtype == LSQ_F16) && G % packet_elems == 0;
    if (pl.mfma) {
        pl.block = kQBlock;
        pl.lds = kQRedBytes + static_cast<int>(M) * kQRowStride;
        pl.chunk = kQChunk;
        pl.waves = kQWaves;
        pl.cols = kQTile;
        pl.packets_per_group = G / packet_elems;
        pl.grid = mfma_grid(N, cus);
    } else {
        pl.block = kBlock;
        pl.lds = 0;
        pl.chunk = 0;
        pl.waves = 1;
        pl.cols = 1;
        pl.packets_per_group = 0;
        pl.grid = generic_grid(N, cus);
    }
    return pl;
}

template <typename IO, int BITS>
static hipError_t qlinear_mfma(const QLinearPlan& pl, const void* x, int64_t M, const void* codes, int64_t N, int64_t K, int64_t G,
                               const void* qscale, const void* qzero, const void* bias, int bias_f32, void* y, hipStream_t stream) {
    static LdsOnce once;
    if (const hipError_t e = allow_lds(once, reinterpret_cast<const void*>(&qlinear_mfma_kernel<IO, BITS>),
                                       kQRedBytes + LSQ_QLINEAR_MAX_ROWS * kQRowStride))
        return e;
    hipLaunchKernelGGL((qlinear_mfma_kernel<IO, BITS>), dim3(pl.grid), dim3(pl.block), pl.lds, stream, x, static_cast<int>(M),
                       static_cast<const uint8_t*>(codes), N, K, K / G, log2_exact(pl.packets_per_group), make_div(pl.packets_per_group),
                       static_cast<const float*>(qscale), static_cast<const int32_t*>(qzero), bias, bias_f32, y);
    return hipGetLastError();
}

template <typename IO, int BITS>
static hipError_t qlinear_generic(const QLinearPlan& pl, const void* x, int64_t M, const void* codes, int64_t N, int64_t K, int64_t G,
                                  const void* qscale, const void* qzero, const void* bias, int bias_f32, void* y, hipStream_t stream) {
    hipLaunchKernelGGL((qlinear_generic_kernel<IO, BITS>), dim3(pl.grid), dim3(pl.block), 0, stream, x, static_cast<int>(M),
                       static_cast<const uint8_t*>(codes), N, K, K / G, make_div(G / (8 / BITS)), static_cast<const float*>(qscale),
                       static_cast<const int32_t*>(qzero), bias, bias_f32, y);
    return hipGetLastError();
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_qlinear.h: validation, dtype dispatch, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

int check_shape(int dtype, int64_t M, int64_t N, int64_t K, int64_t G, int bits, const char* what) {
    return check_shape(dtype, M, N, K, G, bits, what, "a packed weight with a float64 scale has no GPU linear",
                       "dequantize and call a GEMM beyond that");
}

}  // namespace

#define LSQ_QLINEAR_DISPATCH(dtype, bits, FN)                                                                                  \
    switch (dtype) {                                                                                                          \
        case LSQ_BF16: e = bits == 4 ? FN<lsq::io_bf16, 4> ARGS : FN<lsq::io_bf16, 2> ARGS; break;                               \
        case LSQ_F16: e = bits == 4 ? FN<lsq::io_f16, 4> ARGS : FN<lsq::io_f16, 2> ARGS; break;                                  \
        default: break;                                                                                                       \
    }

extern "C" {

int lsq_qlinear_abi_version(void) { return LSQ_QLINEAR_ABI_VERSION; }

const char* lsq_qlinear_last_error(void) { return g_last_error; }

int lsq_qlinear_forward(int dtype, const void* x, int64_t M, const void* codes, int64_t N, int64_t K, int64_t group_size, int bits,
                        const void* qscale, const void* qzero, const void* bias, int bias_dtype, void* y, void* stream) {
    const char* what = "lsq_qlinear_forward";
    if (int rc = check_shape(dtype, M, N, K, group_size, bits, what)) return rc;
    if (!x || !codes || !qscale || !qzero || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (bias && bias_dtype != LSQ_F32 && bias_dtype != dtype)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of x's type, got dtype code %d", what, bias_dtype);
    if (!aligned_to(x, elem_bytes(dtype)) || !aligned_to(y, elem_bytes(dtype)))
        return fail(LSQ_EINVAL, "%s: x and y must be element-aligned", what);
    if (!aligned_to(qscale, 4) || !aligned_to(qzero, 4) || (bias && !aligned_to(bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: qscale, qzero and bias must be element-aligned", what);
    if (N == 0) return LSQ_OK;
    lsq::QLinearPlan pl = lsq::plan_qlinear(dtype, M, N, K, group_size, bits);
    if (pl.mfma && !aligned_to(codes, 16)) pl = lsq::plan_qlinear(LSQ_F32, M, N, K, group_size, bits);   // the generic form
    const int bias_f32 = bias_dtype == LSQ_F32 ? 1 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
#define ARGS (pl, x, M, codes, N, K, group_size, qscale, qzero, bias, bias_f32, y, s)
    if (pl.mfma) {
        LSQ_QLINEAR_DISPATCH(dtype, bits, lsq::qlinear_mfma)
    } else if (dtype == LSQ_F32) {
        e = bits == 4 ? lsq::qlinear_generic<lsq::io_f32, 4> ARGS : lsq::qlinear_generic<lsq::io_f32, 2> ARGS;
    } else {
        LSQ_QLINEAR_DISPATCH(dtype, bits, lsq::qlinear_generic)
    }
#undef ARGS
    return hip_status(e, what);
}

int lsq_qlinear_plan(int dtype, int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int32_t* out8) {
    const char* what = "lsq_qlinear_plan";
    if (int rc = check_shape(dtype, M, N, K, group_size, bits, what)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::QLinearPlan pl = lsq::plan_qlinear(dtype, M, N, K, group_size, bits);
    lsq::write_plan8(out8, pl.mfma, pl.grid, pl.block, pl.lds, pl.chunk, pl.waves, pl.cols);
    return LSQ_OK;
}

}  // extern "C"
