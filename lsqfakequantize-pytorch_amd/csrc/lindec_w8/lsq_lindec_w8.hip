// lsq_lindec_w8.hip -- the decode shape (M <= 16) of the W8A8 linears with an 8-bit output on gfx950 (include/lsq_hip_lindec_w8.h,
// which states what is served): the kernel and the C ABI of liblsq_hip_lindec_w8.so.
//
// Nothing is defined here.  The exact integer is csrc/qlinear_w8/lsq_w8_shared.hpp's w8_exact on the raw sums, the byte is
// csrc/requant_w8/lsq_requant_w8_tiles.hpp's w8q_byte (no residual) or csrc/resadd_w8/lsq_resadd_w8_tiles.hpp's w8r_byte (a
// residual level and the optional pre-quantizer): the same device functions, compiled into this library.
//
// ONE KERNEL TEXT, lindec_w8_kernel<RES>, 1024 threads = 16 waves: the work split of csrc/qlinear_w8/'s decode kernel with a levels
// epilogue of its own.
//  * SPLIT.  A workgroup owns 16 output columns (rows of lw) and walks the tiles in a persistent grid of min(ceil(N / 16), CUs)
//    workgroups.  K is split over the waves: wave v takes the 256 k that start at 256 v of every chunk of at most 4096 k, four
//    16-byte non-temporal packets per lane in flight, issued before the staging barrier.  The packet is the MFMA's B operand as
//    it lies in memory (an xor for a uint8 weight).
//  * X.  The rows' level bytes are staged in LDS per chunk as the byte operand (^ 0x80 for uint8 while staging), rows 16 bytes
//    further apart than their data; when one chunk holds all of K they stay there across the workgroup's tiles.
//  * MFMA.  v_mfma_i32_16x16x64_i8: sum a w; an all-ones B operand gives sum_k a per row, an all-ones A operand sum_k w per
//    column.  The waves' int32 results meet in LDS (16 KB + 2 x 1 KB); one thread per output sums them in 64 bits.
//  * EPILOGUE.  That thread forms the byte in registers and writes it into a [16][16] byte tile in LDS; after one barrier lane
//    m < M of wave 0 stores row m of the tile as ONE 16-byte packet at y + m N + n0 (N % 16 == 0 and y 16-byte aligned), else
//    the tile goes out byte by byte, consecutive lanes on consecutive n.  Rows >= M and columns >= N are never written, neither to
//    LDS nor to memory.
//  * RESIDUAL (RES).  Lane m < M of wave 0 loads the 16 residual bytes of row m of this tile with the tile's first weight
//    packets (behind the weight stream), parks them in the byte tile after the K loop; the thread that forms output (m, c)
//    reads its residual byte there and overwrites it (csrc/resadd_w8/'s scheme).  Without N % 16 == 0 and a 16-byte aligned
//    residual the tile is filled byte by byte after the K loop.
// LDS: 18 KB of partial sums, 256 bytes of byte tile, M rows of x of at most 4096 + 16 bytes: above 64 KB from M = 12 on full
// chunks, behind lsq_qdecode.hpp's opt-in.
#include "../resadd_w8/lsq_resadd_w8_tiles.hpp"
#include "../requant_w8/lsq_requant_w8_checks.hpp"
#include "../../../include/lsq_hip_lindec_w8.h"

static_assert(LSQ_LINDEC_W8_MAX_ROWS == 16, "the rows of x are the 16 rows of one MFMA tile");

namespace lsq {

constexpr int kLdWaves = 16;                        // waves that split K
constexpr int kLdBlock = kLdWaves * 64;
constexpr int kLdChunk = 4096;                      // most elements of K per LDS chunk of x
constexpr int kLdRedBytes = kLdWaves * 256 * 4 + 2 * kLdWaves * 16 * 4;    // sum a w, sum a, sum w of every wave
constexpr int kLdTileBytes = kW8Tile * kW8Tile;     // the byte tile: residual in, y out
constexpr int kLdMaxLds = kLdRedBytes + kLdTileBytes + LSQ_LINDEC_W8_MAX_ROWS * (kLdChunk + kW8RowPad);
static_assert(kLdWaves * kW8Step == kLdChunk, "the waves' steps cover a chunk");

template <bool RES>
__global__ __launch_bounds__(kLdBlock) void lindec_w8_kernel(W8Act act, int M, W8Weight wt, int64_t N, int64_t K, int row_stride,
                                                            W8OutArg out, W8ResArg res, W8PreArg pre, uint8_t* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t* redP = reinterpret_cast<int32_t*>(smem);       // [wave][lane][register]
    int32_t* redS = redP + kLdWaves * 256;                  // [wave][row]
    int32_t* redC = redS + kLdWaves * 16;                   // [wave][column]
    unsigned char* tileb = smem + kLdRedBytes;              // [16][16]
    unsigned char* xs = tileb + kLdTileBytes;

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const W8Const ac = w8_constants(act);
    const uint32_t flipw = wt.off ? 0x80808080u : 0u;
    const int64_t n_p = K / 16;                             // 16-byte packets per row
    const int64_t tiles = (N + kW8Tile - 1) / kW8Tile;
    const int64_t n_chunks = (K + kLdChunk - 1) / kLdChunk;
    const int64_t first_tile = static_cast<int64_t>(blockIdx.x);
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const bool row_lane = wave == 0 && lane < M;            // the lane that moves row `lane` of the byte tile as one packet

    for (int64_t tile = first_tile; tile < tiles; tile += static_cast<int64_t>(gridDim.x)) {
        const int64_t n0 = tile * kW8Tile;
        const int64_t row = std::min<int64_t>(n0 + nl, N - 1);                     // a clamped row computes a value nobody stores
        const uint8_t* __restrict__ wrow = wt.w + row * K;
        i32x4 P = {0, 0, 0, 0}, S = {0, 0, 0, 0}, C = {0, 0, 0, 0};
        u32x4 rp = {0u, 0u, 0u, 0u};                        // RES: this lane's row of the residual tile
        for (int64_t c = 0; c < n_chunks; ++c) {
            const int64_t kc0 = c * kLdChunk;
            const int64_t k0 = kc0 + wave * kW8Step;        // this wave's 256 k of the chunk
            u32x4 b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int64_t p = k0 / 16 + 4 * t + q;
                b[t] = u32x4{0u, 0u, 0u, 0u};
                if (p < n_p) b[t] = load_code_packet(wrow, p) ^ flipw;
            }
            if constexpr (RES) {                            // N % 16 == 0: the packet at n0 < N lies inside N
                if (c == 0 && res.packets && row_lane) rp = *reinterpret_cast<const u32x4*>(res.l + static_cast<int64_t>(lane) * N + n0);
            }
            if (n_chunks > 1 || tile == first_tile) {       // x stays in LDS across tiles when one chunk holds it
                __syncthreads();
                const int kc_len = static_cast<int>(std::min<int64_t>(kLdChunk, K - kc0));
                const int nb = kc_len / 16;                 // blocks of 16 k per row; exact
                const int nbp = (nb + 15) & ~15;            // ... up to whole steps, zero beyond the row
                for (int it = tid; it < M * nbp; it += kLdBlock) {
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
        if constexpr (RES) {                                // the residual tile into the byte tile (the previous tile's stores are done)
            if (res.packets) {
                if (row_lane) *reinterpret_cast<u32x4*>(tileb + lane * kW8Tile) = rp;
            } else if (tid < kLdTileBytes) {                // byte by byte along n: consecutive lanes on consecutive bytes
                const int m = tid >> 4;
                const int64_t n = n0 + (tid & 15);
                if (m < M && n < N) tileb[tid] = res.l[static_cast<int64_t>(m) * N + n];
            }
        }
        __syncthreads();
        if (tid < 256) {                                    // one thread per output: the waves' sums in 64 bits, I, the byte
            const int l = tid & 63, reg = tid >> 6;
            const int col = l & 15, m = (l >> 4) * 4 + reg;
            const int64_t n = n0 + col;
            if (m < M && n < N) {
                int64_t sp = 0, ss = 0, sc = 0;
#pragma unroll
                for (int w = 0; w < kLdWaves; ++w) {
                    sp += redP[(w * 64 + l) * 4 + reg];
                    ss += redS[w * 16 + m];
                    sc += redC[w * 16 + col];
                }
                const int64_t I = w8_exact(sp, sc, ss, K, ac.z, wt.zero[n] - wt.off);
                const W8OutQ oq = w8q_constants(out);
                unsigned char* at_b = tileb + m * kW8Tile + col;    // no other thread touches this byte
                if constexpr (RES) *at_b = w8r_byte(I, wt, ac.s_x, n, oq, w8r_pre_constants(pre), w8r_res_constants(res), *at_b);
                else *at_b = w8q_byte(I, wt, ac.s_x, n, oq);
            }
        }
        __syncthreads();
        if (out.packets) {                                  // N % 16 == 0: the tile's 16 columns lie inside N
            if (row_lane) *reinterpret_cast<u32x4*>(y + static_cast<int64_t>(lane) * N + n0) = *reinterpret_cast<const u32x4*>(tileb + lane * kW8Tile);
        } else if (tid < kLdTileBytes) {
            const int m = tid >> 4;
            const int64_t n = n0 + (tid & 15);
            if (m < M && n < N) y[static_cast<int64_t>(m) * N + n] = tileb[tid];
        }
        __syncthreads();                                    // the byte tile and the sums are free for the next tile
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launcher
// ------------------------------------------------------------------------------------------------
struct LdPlan {
    int served, block, lds, chunks, x_resident, store, res_load, row_stride;
    int64_t grid;
};

inline LdPlan plan_lindec(int64_t M, int64_t N, int64_t K, bool aligned, bool y_aligned, bool res_aligned) {
    LdPlan pl = {};
    if (!(aligned && M >= 1 && M <= LSQ_LINDEC_W8_MAX_ROWS && K > 0 && K % 16 == 0 && K <= kW8MaxK)) return pl;
    const int64_t cus = device_info().cu_count;
    pl.served = 1;
    pl.block = kLdBlock;
    pl.chunks = static_cast<int>((K + kLdChunk - 1) / kLdChunk);
    pl.x_resident = pl.chunks == 1 ? 1 : 0;
    pl.row_stride = static_cast<int>(std::min<int64_t>((K + kW8Step - 1) / kW8Step * kW8Step, kLdChunk)) + kW8RowPad;
    pl.lds = kLdRedBytes + kLdTileBytes + static_cast<int>(M) * pl.row_stride;
    pl.grid = std::min<int64_t>(std::max<int64_t>(1, (N + kW8Tile - 1) / kW8Tile), cus);
    pl.store = (N % 16 == 0 && y_aligned) ? LSQ_LINDEC_W8_PACKETS : LSQ_LINDEC_W8_BYTES;
    pl.res_load = (N % 16 == 0 && res_aligned) ? LSQ_LINDEC_W8_PACKETS : LSQ_LINDEC_W8_BYTES;
    return pl;
}

template <bool RES>
static hipError_t lindec_launch(const LdPlan& pl, const W8Act& act, const W8Weight& wt, int64_t M, int64_t N, int64_t K, W8OutArg out,
                                W8ResArg res, const W8PreArg& pre, uint8_t* y, hipStream_t stream) {
    static LdsOnce once;
    if (const hipError_t e = allow_lds(once, reinterpret_cast<const void*>(&lindec_w8_kernel<RES>), kLdMaxLds)) return e;
    out.packets = pl.store == LSQ_LINDEC_W8_PACKETS ? 1 : 0;
    res.packets = pl.res_load == LSQ_LINDEC_W8_PACKETS ? 1 : 0;
    hipLaunchKernelGGL((lindec_w8_kernel<RES>), dim3(static_cast<unsigned>(pl.grid)), dim3(kLdBlock), pl.lds, stream, act,
                       static_cast<int>(M), wt, N, K, pl.row_stride, out, res, pre, y);
    return hipGetLastError();
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_lindec_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// the residual's and the pre-quantizer's checks, said as csrc/resadd_w8/lsq_resadd_w8.hip says them (a translation unit, not a
// header: a fix there belongs here too); `MN`: the bytes of y and of the residual
int check_res(const char* what, const lsq_resadd_w8_res* r, const void* y, int64_t MN, lsq::W8ResArg& arg) {
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

int check_pre(const char* what, const lsq_resadd_w8_pre* p, lsq::W8PreArg& arg) {
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

// what this form serves; everything else that is legal belongs to lsq_hip_requant_w8.h / lsq_hip_resadd_w8.h
int check_served(const char* what, int64_t M, int64_t K, bool aligned) {
    if (M > LSQ_LINDEC_W8_MAX_ROWS)
        return fail(LSQ_EINVAL, "%s: M = %lld rows of x, the decode kernel serves 1 to %d (more rows: lsq_hip_requant_w8.h / "
                    "lsq_hip_resadd_w8.h)", what, static_cast<ll>(M), LSQ_LINDEC_W8_MAX_ROWS);
    if (K <= 0 || K % 16 != 0 || K > lsq::kW8MaxK)
        return fail(LSQ_EINVAL, "%s: K = %lld, the decode kernel serves multiples of 16 up to %d (every other K: lsq_hip_requant_w8.h / "
                    "lsq_hip_resadd_w8.h)", what, static_cast<ll>(K), lsq::kW8MaxK);
    if (!aligned)
        return fail(LSQ_EINVAL, "%s: w_levels and x_levels must be 16-byte aligned (otherwise: lsq_hip_requant_w8.h / "
                    "lsq_hip_resadd_w8.h)", what);
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_lindec_w8_abi_version(void) { return LSQ_LINDEC_W8_ABI_VERSION; }

const char* lsq_lindec_w8_last_error(void) { return g_last_error; }

int lsq_lindec_w8_linear_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, int w_level_dtype,
                                const void* w_levels, int64_t N, int64_t K, const void* w_scale, const void* w_zero, const void* bias,
                                int bias_dtype, const lsq_requant_w8_out* out, const lsq_resadd_w8_res* res, const lsq_resadd_w8_pre* pre,
                                void* y, void* stream) {
    const char* what = "lsq_lindec_w8_linear_levels";
    int mid = 0;
    lsq::W8OutArg oa{};
    lsq::W8ResArg ra{};
    lsq::W8PreArg pa{};
    if (int rc = check_out(what, out, mid, oa)) return rc;
    if (int rc = check_linear_shape(what, M, N, K)) return rc;
    if (int rc = check_levels_in(what, kCodes, level_dtype, x_levels, s_x, zx)) return rc;
    if (int rc = check_weights(what, kCodes, mid, w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype, y)) return rc;
    if (res) {
        if (int rc = check_res(what, res, y, M * N, ra)) return rc;
    } else if (pre) {
        return fail(LSQ_EINVAL, "%s: a pre-quantizer without a residual (the layer's own quantizer is then the output quantizer)", what);
    }
    if (int rc = check_pre(what, pre, pa)) return rc;
    const bool aligned = aligned_to(w_levels, 16) && aligned_to(x_levels, 16);
    if (int rc = check_served(what, M, K, aligned)) return rc;
    const lsq::LdPlan pl = lsq::plan_lindec(M, N, K, aligned, aligned_to(y, 16), res && aligned_to(res->levels, 16));
    if (N == 0) return LSQ_OK;
    const lsq::W8Act act = levels_act(level_dtype, x_levels, s_x, zx);
    const lsq::W8Weight wt = weight_arg(w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* yb = static_cast<uint8_t*>(y);
    return hip_status(res ? lsq::lindec_launch<true>(pl, act, wt, M, N, K, oa, ra, pa, yb, st)
                          : lsq::lindec_launch<false>(pl, act, wt, M, N, K, oa, ra, pa, yb, st), what);
}

int lsq_lindec_w8_plan(int64_t M, int64_t N, int64_t K, int aligned, int y_aligned, int res_aligned, int32_t* out8) {
    const char* what = "lsq_lindec_w8_plan";
    if (int rc = check_linear_shape(what, M, N, K)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::LdPlan pl = lsq::plan_lindec(M, N, K, aligned != 0, y_aligned != 0, res_aligned != 0);
    out8[0] = pl.served;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.block;
    out8[3] = pl.lds;
    out8[4] = pl.chunks;
    out8[5] = pl.x_resident;
    out8[6] = pl.store;
    out8[7] = pl.res_load;
    return LSQ_OK;
}

}  // extern "C"
