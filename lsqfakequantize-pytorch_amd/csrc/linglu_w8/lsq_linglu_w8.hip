// lsq_linglu_w8.hip -- the gate and up projections of a gated MLP's decode step (M <= 16) with the gated product in their epilogue
// on gfx950 (include/lsq_hip_linglu_w8.h, which states what is served): the kernel and the C ABI of liblsq_hip_linglu_w8.so.
//
// Nothing is defined here.  The exact integer is csrc/qlinear_w8/lsq_w8_shared.hpp's w8_exact on the raw sums, the gate byte and
// the up byte are csrc/requant_w8/lsq_requant_w8_tiles.hpp's w8q_byte, the product is csrc/glu_w8/lsq_glu_w8_dev.hpp's glu_product
// on the table entry of the gate byte and glu_dequant of the up byte, its level csrc/lsq_w8_out_side.hpp's w8o_byte: the same
// device functions, compiled into this library.
//
// ONE KERNEL TEXT, linglu_w8_kernel, 1024 threads = 16 waves: csrc/lindec_w8/'s work split on a PAIR of weight strips.
//  * SPLIT.  A workgroup owns 16 product columns c0 .. c0 + 15 -- gate rows c0 + nl of the gate weight and up rows c0 + nl of the up
//    weight -- and walks the tiles in a persistent grid of min(ceil(C / 16), CUs) workgroups.  K is split over the waves: wave v
//    takes the 256 k that start at 256 v of every chunk of at most 4096 k and streams BOTH strips of them, eight 16-byte
//    non-temporal packets per lane in flight (four gate, four up), all issued before the staging barrier.
//  * X.  Staged as in lindec_w8: the rows' level bytes per chunk as the byte operand, rows 16 bytes further apart than their data;
//    when one chunk holds all of K they stay in LDS across the workgroup's tiles.
//  * MFMA.  v_mfma_i32_16x16x64_i8.  One ds_read of the x operand serves both strips, and so does the all-ones B operand that
//    gives sum_k a: five MFMAs per step (P_g, P_u, S, C_g, C_u) where two launches spend six.
//  * REDUCTION.  The waves' int32 tiles meet in LDS: two P regions of 16 KB, one S region, two C regions.  Threads 0..255 sum gate
//    output (m, col) in 64 bits and form its byte into a [16][16] gate tile; threads 256..511 do the same for up at the same
//    time (whole waves on either side of the select): one barrier.
//  * PRODUCT.  The table is staged once per workgroup into 1 KB of LDS, one entry per thread, rounded to mid as
//    glu_w8_packets_kernel rounds it.  Thread (m, col) reads its gate byte and its up byte from the two tiles and writes the
//    product's level into the output tile.
//  * STORE.  After one barrier lane m < M of wave 0 stores row m of the output tile as ONE 16-byte packet at y + m C + c0
//    (C % 16 == 0 and y 16-byte aligned), else the tile goes out byte by byte, consecutive lanes on consecutive columns.  Rows
//    >= M and columns >= C are never written, neither to LDS nor to memory.
//  * BARRIERS.  Three per tile (sums written, bytes written, levels written).  None behind the stores: a region is written
//    again only behind a later barrier than the one its readers have passed -- the sums behind "levels written" (read before
//    "bytes written"), the two byte tiles behind the next "sums written", the output tile behind the next "bytes written".
// LDS: 35 KB of partial sums, 768 bytes of tiles, 1 KB of table, M rows of x of at most 4096 + 16 bytes: at most 101 KB, behind
// lsq_qdecode.hpp's opt-in.
#include "../requant_w8/lsq_requant_w8_tiles.hpp"
#include "../requant_w8/lsq_requant_w8_checks.hpp"
#include "../glu_w8/lsq_glu_w8_dev.hpp"
#include "../../../include/lsq_hip_linglu_w8.h"

static_assert(LSQ_LINGLU_W8_MAX_ROWS == 16, "the rows of x are the 16 rows of one MFMA tile");
static_assert(LSQ_GLU_W8_U8 == LSQ_REQUANT_W8_U8 && LSQ_GLU_W8_I8 == LSQ_REQUANT_W8_I8, "one level type code for the three steps");

namespace lsq {

constexpr int kLgWaves = 16;                        // waves that split K
constexpr int kLgBlock = kLgWaves * 64;
constexpr int kLgChunk = 4096;                      // most elements of K per LDS chunk of x
constexpr int kLgRedP = kLgWaves * 256;             // int32 values of one P region
constexpr int kLgRedV = kLgWaves * 16;              // ... of the S region and of one C region
constexpr int kLgRedBytes = (2 * kLgRedP + 3 * kLgRedV) * 4;    // sum a w (gate, up), sum a, sum w (gate, up) of every wave
constexpr int kLgTile = kW8Tile * kW8Tile;          // one byte tile
constexpr int kLgTabBytes = 256 * 4;
constexpr int kLgFixedLds = kLgRedBytes + 3 * kLgTile + kLgTabBytes;
constexpr int kLgMaxLds = kLgFixedLds + LSQ_LINGLU_W8_MAX_ROWS * (kLgChunk + kW8RowPad);
static_assert(kLgWaves * kW8Step == kLgChunk, "the waves' steps cover a chunk");
static_assert(kLgFixedLds % 16 == 0, "the rows of x are read as 16-byte packets");

struct LgPair {             // kernel argument: the two projections
    W8Weight gate, up;
    W8OutArg gate_out, up_out;
};

__global__ __launch_bounds__(kLgBlock) void linglu_w8_kernel(W8Act act, int M, LgPair pr, int64_t C, int64_t K, int row_stride, GluArg ga,
                                                            const float* __restrict__ table, int packets, uint8_t* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t* redP = reinterpret_cast<int32_t*>(smem);       // [gate, up][wave][lane][register]
    int32_t* redS = redP + 2 * kLgRedP;                     // [wave][row]
    int32_t* redC = redS + kLgRedV;                         // [gate, up][wave][column]
    unsigned char* tiles = smem + kLgRedBytes;              // [gate, up, y][16][16]
    float* tab = reinterpret_cast<float*>(tiles + 3 * kLgTile);
    unsigned char* xs = smem + kLgFixedLds;

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const W8Const ac = w8_constants(act);
    const uint32_t flipg = pr.gate.off ? 0x80808080u : 0u, flipu = pr.up.off ? 0x80808080u : 0u;
    const int64_t n_p = K / 16;                             // 16-byte packets per row
    const int64_t tiles_n = (C + kW8Tile - 1) / kW8Tile;
    const int64_t n_chunks = (K + kLgChunk - 1) / kLgChunk;
    const int64_t first_tile = static_cast<int64_t>(blockIdx.x);
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};

    // a value of mid already (the contract): the identity, once per entry and not per element.  Read behind the first tile's barriers.
    if (tid < 256) tab[tid] = w8o_round_mid(table[tid], ga.mid);

    for (int64_t tile = first_tile; tile < tiles_n; tile += static_cast<int64_t>(gridDim.x)) {
        const int64_t c0 = tile * kW8Tile;
        const int64_t row = std::min<int64_t>(c0 + nl, C - 1);                     // a clamped row computes a value nobody stores
        const uint8_t* __restrict__ grow = pr.gate.w + row * K;
        const uint8_t* __restrict__ urow = pr.up.w + row * K;
        i32x4 Pg = {0, 0, 0, 0}, Pu = {0, 0, 0, 0}, S = {0, 0, 0, 0}, Cg = {0, 0, 0, 0}, Cu = {0, 0, 0, 0};
        for (int64_t c = 0; c < n_chunks; ++c) {
            const int64_t kc0 = c * kLgChunk;
            const int64_t k0 = kc0 + wave * kW8Step;        // this wave's 256 k of the chunk
            u32x4 bg[4], bu[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int64_t p = k0 / 16 + 4 * t + q;
                bg[t] = u32x4{0u, 0u, 0u, 0u};
                bu[t] = u32x4{0u, 0u, 0u, 0u};
                if (p < n_p) {
                    bg[t] = load_code_packet(grow, p) ^ flipg;
                    bu[t] = load_code_packet(urow, p) ^ flipu;
                }
            }
            if (n_chunks > 1 || tile == first_tile) {       // x stays in LDS across tiles when one chunk holds it
                __syncthreads();
                const int kc_len = static_cast<int>(std::min<int64_t>(kLgChunk, K - kc0));
                const int nb = kc_len / 16;                 // blocks of 16 k per row; exact
                const int nbp = (nb + 15) & ~15;            // ... up to whole steps, zero beyond the row
                for (int it = tid; it < M * nbp; it += kLgBlock) {
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
                    const i32x4 gt = w8_as_i32(bg[t]), ut = w8_as_i32(bu[t]);
                    Pg = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, gt, Pg, 0, 0, 0);
                    Pu = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, ut, Pu, 0, 0, 0);
                    S = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, ones, S, 0, 0, 0);
                    Cg = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, gt, Cg, 0, 0, 0);
                    Cu = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, ut, Cu, 0, 0, 0);
                }
            }
        }
        // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register.  S is the same in every column, C in every row.
        *reinterpret_cast<i32x4*>(redP + (wave * 64 + lane) * 4) = Pg;
        *reinterpret_cast<i32x4*>(redP + kLgRedP + (wave * 64 + lane) * 4) = Pu;
        if (nl == 0) *reinterpret_cast<i32x4*>(redS + wave * 16 + q * 4) = S;
        if (q == 0) {
            redC[wave * 16 + nl] = Cg[0];
            redC[kLgRedV + wave * 16 + nl] = Cu[0];
        }
        __syncthreads();                                    // sums written
        if (tid < 512) {                                    // one thread per output of either projection: whole waves take a side
            const int side = tid >> 8;                      // 0: gate, 1: up
            const int l = tid & 63, reg = (tid >> 6) & 3;
            const int col = l & 15, m = (l >> 4) * 4 + reg;
            const int64_t n = c0 + col;
            if (m < M && n < C) {
                const int32_t* rp = redP + side * kLgRedP;
                const int32_t* rc = redC + side * kLgRedV;
                int64_t sp = 0, ss = 0, sc = 0;
#pragma unroll
                for (int w = 0; w < kLgWaves; ++w) {
                    sp += rp[(w * 64 + l) * 4 + reg];
                    ss += redS[w * 16 + m];
                    sc += rc[w * 16 + col];
                }
                const W8Weight& wt = side ? pr.up : pr.gate;
                const int64_t I = w8_exact(sp, sc, ss, K, ac.z, wt.zero[n] - wt.off);
                const W8OutQ oq = w8q_constants(side ? pr.up_out : pr.gate_out);
                tiles[side * kLgTile + m * kW8Tile + col] = w8q_byte(I, wt, ac.s_x, n, oq);
            }
        }
        __syncthreads();                                    // bytes written
        if (tid < kLgTile) {                                // thread (m, col): consecutive lanes on consecutive columns
            const int m = tid >> 4;
            if (m < M && c0 + (tid & 15) < C) {
                const GluQ gq = glu_constants(ga);
                const uint32_t g = tiles[tid], u = static_cast<uint32_t>(tiles[kLgTile + tid]) ^ (ga.flip_u & 0xffu);
                tiles[2 * kLgTile + tid] = static_cast<unsigned char>(w8o_byte(glu_product(tab[g], glu_dequant<0>(u, gq), gq.mid), gq));
            }
        }
        __syncthreads();                                    // levels written
        const unsigned char* outb = tiles + 2 * kLgTile;
        if (packets) {                                      // C % 16 == 0: the tile's 16 columns lie inside C
            if (wave == 0 && lane < M)
                *reinterpret_cast<u32x4*>(y + static_cast<int64_t>(lane) * C + c0) = *reinterpret_cast<const u32x4*>(outb + lane * kW8Tile);
        } else if (tid < kLgTile) {
            const int m = tid >> 4;
            const int64_t n = c0 + (tid & 15);
            if (m < M && n < C) y[static_cast<int64_t>(m) * C + n] = outb[tid];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launcher
// ------------------------------------------------------------------------------------------------
struct LgPlan {
    int served, block, lds, chunks, x_resident, store, row_stride;
    int64_t grid;
};

inline LgPlan plan_linglu(int64_t M, int64_t C, int64_t K, bool aligned, bool y_aligned) {
    LgPlan pl = {};
    if (!(aligned && M >= 1 && M <= LSQ_LINGLU_W8_MAX_ROWS && K > 0 && K % 16 == 0 && K <= kW8MaxK)) return pl;
    const int64_t cus = device_info().cu_count;
    pl.served = 1;
    pl.block = kLgBlock;
    pl.chunks = static_cast<int>((K + kLgChunk - 1) / kLgChunk);
    pl.x_resident = pl.chunks == 1 ? 1 : 0;
    pl.row_stride = static_cast<int>(std::min<int64_t>((K + kW8Step - 1) / kW8Step * kW8Step, kLgChunk)) + kW8RowPad;
    pl.lds = kLgFixedLds + static_cast<int>(M) * pl.row_stride;
    pl.grid = std::min<int64_t>(std::max<int64_t>(1, (C + kW8Tile - 1) / kW8Tile), cus);
    pl.store = (C % 16 == 0 && y_aligned) ? LSQ_LINGLU_W8_PACKETS : LSQ_LINGLU_W8_BYTES;
    return pl;
}

static hipError_t linglu_launch(const LgPlan& pl, const W8Act& act, const LgPair& pr, int64_t M, int64_t C, int64_t K, const GluArg& ga,
                                const float* table, uint8_t* y, hipStream_t stream) {
    static LdsOnce once;
    if (const hipError_t e = allow_lds(once, reinterpret_cast<const void*>(&linglu_w8_kernel), kLgMaxLds)) return e;
    hipLaunchKernelGGL(linglu_w8_kernel, dim3(static_cast<unsigned>(pl.grid)), dim3(kLgBlock), pl.lds, stream, act, static_cast<int>(M), pr,
                       C, K, pl.row_stride, ga, table, pl.store == LSQ_LINGLU_W8_PACKETS ? 1 : 0, y);
    return hipGetLastError();
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_linglu_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// one projection's checks, said as csrc/requant_w8/ says them; `name`: "gate" / "up"
int check_proj(const char* what, const char* name, const lsq_linglu_w8_proj* p, const void* y, lsq::W8Weight& wt, lsq::W8OutArg& oa) {
    char who[96];
    snprintf(who, sizeof(who), "%s (%s projection)", what, name);
    if (!p) return fail(LSQ_EINVAL, "%s: NULL projection", who);
    int mid = 0;
    if (int rc = check_out(who, p->out, mid, oa)) return rc;
    if (oa.relu) return fail(LSQ_EINVAL, "%s: relu is set: the gated product takes the projection's own levels (not served)", who);
    if (int rc = check_weights(who, kCodes, mid, static_cast<int>(p->w_level_dtype), p->w_levels, p->w_scale, p->w_zero, p->bias,
                               static_cast<int>(p->bias_dtype), y))
        return rc;
    wt = weight_arg(static_cast<int>(p->w_level_dtype), p->w_levels, p->w_scale, p->w_zero, p->bias, static_cast<int>(p->bias_dtype));
    return LSQ_OK;
}

// the product's constants, said as csrc/glu_w8/lsq_glu_w8.hip says them (a translation unit, not a header: a fix there belongs
// here too); `up_signed`: the up projection's quantizer gives int8 levels
int check_consts(const char* what, const lsq_glu_w8_consts* c, bool up_signed, lsq::GluArg& arg) {
    if (!c) return fail(LSQ_EINVAL, "%s: NULL constants", what);
    if (!c->s_u || !c->z_u) return fail(LSQ_EINVAL, "%s: NULL s_u or z_u", what);
    if (!aligned_to(c->s_u, 4) || !aligned_to(c->z_u, 4)) return fail(LSQ_EINVAL, "%s: s_u and z_u must be element-aligned", what);
    int64_t y_elem = 1;
    if (int rc = check_out_side(what, *c, arg, y_elem)) return rc;
    if (!c->out_scale) return fail(LSQ_EINVAL, "%s: NULL out_scale and out_shift: a floating product is not served (lsq_hip_glu_w8.h)", what);
    arg.s_u = static_cast<const float*>(c->s_u);
    arg.z_u = static_cast<const int32_t*>(c->z_u);
    arg.flip_u = up_signed ? 0x80808080u : 0u;
    return LSQ_OK;
}

// what this library serves; everything else that is legal belongs to lsq_hip_requant_w8.h and lsq_hip_glu_w8.h
int check_served(const char* what, int64_t M, int64_t K, bool aligned) {
    if (M > LSQ_LINGLU_W8_MAX_ROWS)
        return fail(LSQ_EINVAL, "%s: M = %lld rows of x, the kernel serves 1 to %d (more rows: lsq_hip_requant_w8.h, then lsq_hip_glu_w8.h)",
                    what, static_cast<ll>(M), LSQ_LINGLU_W8_MAX_ROWS);
    if (K <= 0 || K % 16 != 0 || K > lsq::kW8MaxK)
        return fail(LSQ_EINVAL, "%s: K = %lld, the kernel serves multiples of 16 up to %d (every other K: lsq_hip_requant_w8.h, then "
                    "lsq_hip_glu_w8.h)", what, static_cast<ll>(K), lsq::kW8MaxK);
    if (!aligned)
        return fail(LSQ_EINVAL, "%s: x_levels and both w_levels must be 16-byte aligned (otherwise: lsq_hip_requant_w8.h, then "
                    "lsq_hip_glu_w8.h)", what);
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_linglu_w8_abi_version(void) { return LSQ_LINGLU_W8_ABI_VERSION; }

const char* lsq_linglu_w8_last_error(void) { return g_last_error; }

int lsq_linglu_w8(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, const lsq_linglu_w8_proj* gate,
                  const lsq_linglu_w8_proj* up, int64_t C, int64_t K, const void* table, const lsq_glu_w8_consts* consts, void* y,
                  void* stream) {
    const char* what = "lsq_linglu_w8";
    lsq::LgPair pr{};
    lsq::GluArg ga{};
    if (int rc = check_linear_shape(what, M, C, K)) return rc;
    if (int rc = check_levels_in(what, kCodes, level_dtype, x_levels, s_x, zx)) return rc;
    if (int rc = check_proj(what, "gate", gate, y, pr.gate, pr.gate_out)) return rc;
    if (int rc = check_proj(what, "up", up, y, pr.up, pr.up_out)) return rc;
    const bool up_signed = std::max(up->out->quant_max, up->out->type_max) <= 127;
    if (int rc = check_consts(what, consts, up_signed, ga)) return rc;
    if (!table) return fail(LSQ_EINVAL, "%s: NULL table", what);
    if (!aligned_to(table, 4)) return fail(LSQ_EINVAL, "%s: the table's 256 float32 values must be 4-byte aligned", what);
    if (overlap(y, M * C, table, 1024)) return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap the table's 1024", what, static_cast<ll>(M * C));
    const bool aligned = aligned_to(x_levels, 16) && aligned_to(gate->w_levels, 16) && aligned_to(up->w_levels, 16);
    if (int rc = check_served(what, M, K, aligned)) return rc;
    const lsq::LgPlan pl = lsq::plan_linglu(M, C, K, aligned, aligned_to(y, 16));
    if (C == 0) return LSQ_OK;
    const lsq::W8Act act = levels_act(level_dtype, x_levels, s_x, zx);
    return hip_status(lsq::linglu_launch(pl, act, pr, M, C, K, ga, static_cast<const float*>(table), static_cast<uint8_t*>(y),
                                         static_cast<hipStream_t>(stream)), what);
}

int lsq_linglu_w8_plan(int64_t M, int64_t C, int64_t K, int aligned, int y_aligned, int32_t* out8) {
    const char* what = "lsq_linglu_w8_plan";
    if (int rc = check_linear_shape(what, M, C, K)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::LgPlan pl = lsq::plan_linglu(M, C, K, aligned != 0, y_aligned != 0);
    out8[0] = pl.served;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.block;
    out8[3] = pl.lds;
    out8[4] = pl.chunks;
    out8[5] = pl.x_resident;
    out8[6] = pl.store;
    out8[7] = 0;
    return LSQ_OK;
}

}  // extern "C"
