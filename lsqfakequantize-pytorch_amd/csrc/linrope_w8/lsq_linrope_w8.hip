// lsq_linrope_w8.hip -- the qkv projection of an attention block's decode step (M <= 16) with the rotary embedding and the KV-cache
// append in its epilogue on gfx950 (include/lsq_hip_linrope_w8.h, which states what is served): the kernel and the C ABI of
// liblsq_hip_linrope_w8.so.
//
// Nothing is defined here.  The exact integer is csrc/qlinear_w8/lsq_w8_shared.hpp's w8_exact on the raw sums, the qkv byte is
// csrc/requant_w8/lsq_requant_w8_tiles.hpp's w8q_byte, the rotation is rope_dequant and rope_pair on two qkv bytes, its level
// csrc/lsq_w8_out_side.hpp's w8o_byte.  The rotation's device functions, the placement of the rows, the decoding of an item and
// the geometry's checks are csrc/linrope_w8/lsq_linrope_shared.hpp's, which csrc/linrope_w4/lsq_linrope_w4.hip compiles too.
//
// ONE KERNEL TEXT, linrope_w8_kernel, 1024 threads = 16 waves: csrc/linglu_w8/'s skeleton on a pair of strips of ONE weight.
//  * ITEMS.  HF's rotate_half pairs feature i with i + R / 2: two different 16-column tiles of the qkv output.  A work item is
//    therefore always TWO 16-row strips of the weight, so every item costs the same: ROTATE the features f0 .. f0 + 15 (f0 < R / 2)
//    and f0 + R / 2 .. of one q or k head, PASS two adjacent strips of a q or k head beyond R (u = d(l)), COPY two adjacent strips
//    of a v head.  D % 32 == 0 and R % 32 == 0: the (H + 2 Hkv) D / 32 items tile the columns exactly, no row is clamped.  The
//    grid is persistent, min(items, CUs) workgroups.
//  * PLACEMENT.  Before the first item 16 threads compute, per row m = b T + t: p = positions[b] + t, the three write flags and
//    the byte offsets of the row in rq, k and v -- dense from strides, paged from ONE block-table read -- into 512 bytes of LDS.
//    From there dense and paged are the same kernel text, and the epilogue never touches `positions` or the table again.
//  * STREAM, X, MFMA, REDUCTION.  As linglu_w8_kernel: K split over the waves in chunks of at most 4096, eight non-temporal 16-byte
//    weight packets per lane in flight (four per strip), x staged in LDS and resident across items when one chunk holds K,
//    v_mfma_i32_16x16x64_i8 with the shared all-ones operand, five MFMAs per step, the waves' int32 tiles meet in LDS and threads
//    0..511 sum them in 64 bits and form the two qkv byte tiles [16][16].
//  * COS / SIN.  Thread (m, col) of the 256 that rotate issues its cos[p_m, f0 + col] and sin[p_m, f0 + col] loads BEFORE the K
//    loop of a ROTATE item: they land behind the weight stream.
//  * ROTATION.  After one barrier thread (m, col) reads l_i and l_j from the two byte tiles, forms u_i and u_j (PASS: d(l) of both;
//    COPY: the bytes themselves) and writes two output byte tiles.
//  * STORE.  After one more barrier lane m < M of wave 0 stores row m of strip A as ONE 16-byte packet at its destination, wave 1
//    strip B.  Rows whose flag is off and rows >= M are written neither to the output tiles nor to memory.
//  * BARRIERS.  One behind the placement, then three per item (sums written, bytes written, levels written).  None behind the
//    stores: a region is written again only behind a later barrier than the one its readers have passed -- the sums behind
//    "levels written" (read before "bytes written"), the two qkv byte tiles behind the next "sums written" (read before "levels
//    written"), the two output tiles behind the next "bytes written" (the stores that read them stand before the next "sums
//    written").  The placement is written once and only read afterwards.
// LDS: 35 KB of partial sums, 1 KB of tiles, 512 bytes of placement, M rows of x of at most 4096 + 16 bytes: at most 101.5 KB,
// behind lsq_qdecode.hpp's opt-in.
#include "../requant_w8/lsq_requant_w8_tiles.hpp"
#include "../requant_w8/lsq_requant_w8_checks.hpp"
#include "lsq_linrope_shared.hpp"

static_assert(LSQ_LINROPE_W8_MAX_ROWS == 16, "the rows of x are the 16 rows of one MFMA tile");
static_assert(LSQ_ROPE_W8_U8 == LSQ_REQUANT_W8_U8 && LSQ_ROPE_W8_I8 == LSQ_REQUANT_W8_I8, "one level type code for the two steps");

namespace lsq {

constexpr int kLrWaves = 16;                        // waves that split K
constexpr int kLrBlock = kLrWaves * 64;
constexpr int kLrChunk = 4096;                      // most elements of K per LDS chunk of x
constexpr int kLrRedP = kLrWaves * 256;             // int32 values of one P region
constexpr int kLrRedV = kLrWaves * 16;              // ... of the S region and of one C region
constexpr int kLrRedBytes = (2 * kLrRedP + 3 * kLrRedV) * 4;    // sum a w (strip A, B), sum a, sum w (strip A, B) of every wave
constexpr int kLrTile = kW8Tile * kW8Tile;          // one byte tile
constexpr int kLrFixedLds = kLrRedBytes + 4 * kLrTile + kLrPlaceBytes;
constexpr int kLrMaxLds = kLrFixedLds + LSQ_LINROPE_W8_MAX_ROWS * (kLrChunk + kW8RowPad);
static_assert(kLrWaves * kW8Step == kLrChunk, "the waves' steps cover a chunk");
static_assert(kLrFixedLds % 16 == 0, "the rows of x are read as 16-byte packets");

__global__ __launch_bounds__(kLrBlock) void linrope_w8_kernel(W8Act act, int M, W8Weight wt, W8OutArg qkv_out, int64_t K, int row_stride,
                                                             LrGeom g, RopeArg ra, const float* __restrict__ cos_t,
                                                             const float* __restrict__ sin_t, const int32_t* __restrict__ pos,
                                                             const int32_t* __restrict__ bt, LrDst dst) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t* redP = reinterpret_cast<int32_t*>(smem);       // [strip A, B][wave][lane][register]
    int32_t* redS = redP + 2 * kLrRedP;                     // [wave][row]
    int32_t* redC = redS + kLrRedV;                         // [strip A, B][wave][column]
    unsigned char* tiles = smem + kLrRedBytes;              // [qkv A, qkv B, out A, out B][16][16]
    const LrPlace place = lr_place_at(tiles + 4 * kLrTile);
    int64_t* pl_off = place.off;
    int32_t* pl_p = place.p;
    int32_t* pl_flags = place.flags;
    unsigned char* xs = smem + kLrFixedLds;

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const W8Const ac = w8_constants(act);
    const uint32_t flipw = wt.off ? 0x80808080u : 0u;
    const int64_t n_p = K / 16;                             // 16-byte packets per row
    const int64_t n_chunks = (K + kLrChunk - 1) / kLrChunk;
    const int first_item = static_cast<int>(blockIdx.x);
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};

    // where the rows go, once per workgroup
    if (tid < 16) lr_place_row(g, M, pos, bt, place, tid);
    __syncthreads();                                        // placement written

    for (int item = first_item; item < g.items; item += static_cast<int>(gridDim.x)) {
        const LrItem it = lr_item(g, item);
        const int kind = it.kind, hh = it.hh, fA = it.fA, fB = it.fB, bit = it.bit;
        const bool rot = it.rot;
        const int64_t nA = it.nA, nB = it.nB;
        const uint8_t* __restrict__ arow = wt.w + (nA + nl) * K;
        const uint8_t* __restrict__ brow = wt.w + (nB + nl) * K;

        float cs = 0.0f, sn = 0.0f;                         // in flight during the K loop
        if (rot && tid < kLrTile && (tid >> 4) < M && (pl_flags[tid >> 4] & bit)) {
            const int64_t col = static_cast<int64_t>(pl_p[tid >> 4]) * (g.R / 2) + fA + (tid & 15);
            cs = cos_t[col];
            sn = sin_t[col];
        }

        i32x4 Pa = {0, 0, 0, 0}, Pb = {0, 0, 0, 0}, S = {0, 0, 0, 0}, Ca = {0, 0, 0, 0}, Cb = {0, 0, 0, 0};
        for (int64_t c = 0; c < n_chunks; ++c) {
            const int64_t kc0 = c * kLrChunk;
            const int64_t k0 = kc0 + wave * kW8Step;        // this wave's 256 k of the chunk
            u32x4 ba[4], bb[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int64_t p = k0 / 16 + 4 * t + q;
                ba[t] = u32x4{0u, 0u, 0u, 0u};
                bb[t] = u32x4{0u, 0u, 0u, 0u};
                if (p < n_p) {
                    ba[t] = load_code_packet(arow, p) ^ flipw;
                    bb[t] = load_code_packet(brow, p) ^ flipw;
                }
            }
            if (n_chunks > 1 || item == first_item) {       // x stays in LDS across items when one chunk holds it
                __syncthreads();
                const int kc_len = static_cast<int>(std::min<int64_t>(kLrChunk, K - kc0));
                const int nb = kc_len / 16;                 // blocks of 16 k per row; exact
                const int nbp = (nb + 15) & ~15;            // ... up to whole steps, zero beyond the row
                for (int it = tid; it < M * nbp; it += kLrBlock) {
                    const int m = it / nbp, blk = it - m * nbp;
                    u32x4 v = {0u, 0u, 0u, 0u};
                    if (blk < nb) v = w8_load16(act, ac.flip, static_cast<int64_t>(m) * K + kc0 + blk * 16);
                    *reinterpret_cast<u32x4*>(xs + m * row_stride + blk * 16) = v;
                }
                __syncthreads();
            }
            if (k0 < K) {                                   // the same for the whole wave
                const unsigned char* xa = xs + nl * row_stride + wave * kW8Step + q * 16;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    i32x4 a = {0, 0, 0, 0};
                    if (nl < M) a = *reinterpret_cast<const i32x4*>(xa + t * 64);
                    const i32x4 at = w8_as_i32(ba[t]), bt4 = w8_as_i32(bb[t]);
                    Pa = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, at, Pa, 0, 0, 0);
                    Pb = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bt4, Pb, 0, 0, 0);
                    S = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, ones, S, 0, 0, 0);
                    Ca = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, at, Ca, 0, 0, 0);
                    Cb = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bt4, Cb, 0, 0, 0);
                }
            }
        }
        // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register.  S is the same in every column, C in every row.
        *reinterpret_cast<i32x4*>(redP + (wave * 64 + lane) * 4) = Pa;
        *reinterpret_cast<i32x4*>(redP + kLrRedP + (wave * 64 + lane) * 4) = Pb;
        if (nl == 0) *reinterpret_cast<i32x4*>(redS + wave * 16 + q * 4) = S;
        if (q == 0) {
            redC[wave * 16 + nl] = Ca[0];
            redC[kLrRedV + wave * 16 + nl] = Cb[0];
        }
        __syncthreads();                                    // sums written
        if (tid < 512) {                                    // one thread per qkv output of either strip: whole waves take a side
            const int side = tid >> 8;                      // 0: strip A, 1: strip B
            const int l = tid & 63, reg = (tid >> 6) & 3;
            const int col = l & 15, m = (l >> 4) * 4 + reg;
            if (m < M) {
                const int64_t n = (side ? nB : nA) + col;
                const int32_t* rp = redP + side * kLrRedP;
                const int32_t* rc = redC + side * kLrRedV;
                int64_t sp = 0, ss = 0, sc = 0;
#pragma unroll
                for (int w = 0; w < kLrWaves; ++w) {
                    sp += rp[(w * 64 + l) * 4 + reg];
                    ss += redS[w * 16 + m];
                    sc += rc[w * 16 + col];
                }
                const int64_t I = w8_exact(sp, sc, ss, K, ac.z, wt.zero[n] - wt.off);
                tiles[side * kLrTile + m * kW8Tile + col] = w8q_byte(I, wt, ac.s_x, n, w8q_constants(qkv_out));
            }
        }
        __syncthreads();                                    // bytes written
        if (tid < kLrTile) {                                // thread (m, col): consecutive lanes on consecutive columns
            const int m = tid >> 4;
            if (m < M && (pl_flags[m] & bit)) {
                const uint32_t la = tiles[tid], lb = tiles[kLrTile + tid];
                uint32_t oa = la, ob = lb;                  // COPY: y byte = x byte
                if (kind < 2) {
                    const RopeQ rq = rope_constants(ra, g.flip);
                    const float da = rope_dequant<0>(la ^ g.flip, rq), db = rope_dequant<0>(lb ^ g.flip, rq);
                    float ua = da, ub = db;                 // PASS: u = d(l)
                    if (rot) rope_pair(da, db, cs, sn, rq.mid, ua, ub);
                    oa = w8o_byte(ua, rq);
                    ob = w8o_byte(ub, rq);
                }
                tiles[2 * kLrTile + tid] = static_cast<unsigned char>(oa);
                tiles[3 * kLrTile + tid] = static_cast<unsigned char>(ob);
            }
        }
        __syncthreads();                                    // levels written
        if (wave < 2 && lane < M && (pl_flags[lane] & bit)) {       // wave 0: strip A, wave 1: strip B; one 16-byte packet per row
            uint8_t* at = dst.p[kind] + pl_off[kind * 16 + lane] + hh * g.head_s[kind] + (wave ? fB : fA);
            *reinterpret_cast<u32x4*>(at) = *reinterpret_cast<const u32x4*>(tiles + (2 + wave) * kLrTile + lane * kW8Tile);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launcher
// ------------------------------------------------------------------------------------------------
struct LrPlan {
    int served, block, lds, chunks, x_resident, row_stride, rotate, pass, copy;
    int64_t grid;
};

inline LrPlan plan_linrope(const lsq_linrope_w8_geom& ge, int64_t K, bool aligned) {
    LrPlan pl = {};
    const int64_t M = ge.B * ge.T;
    if (!(aligned && lr_geom_served(ge) && K > 0 && K % 16 == 0 && K <= kW8MaxK)) return pl;
    const int64_t cus = device_info().cu_count;
    pl.served = 1;
    pl.block = kLrBlock;
    pl.chunks = static_cast<int>((K + kLrChunk - 1) / kLrChunk);
    pl.x_resident = pl.chunks == 1 ? 1 : 0;
    pl.row_stride = static_cast<int>(std::min<int64_t>((K + kW8Step - 1) / kW8Step * kW8Step, kLrChunk)) + kW8RowPad;
    pl.lds = kLrFixedLds + static_cast<int>(M) * pl.row_stride;
    lr_item_counts(ge, pl.rotate, pl.pass, pl.copy);
    pl.grid = std::min<int64_t>(pl.rotate + pl.pass + pl.copy, cus);
    return pl;
}

static hipError_t linrope_launch(const LrPlan& pl, const W8Act& act, int M, const W8Weight& wt, const W8OutArg& qo, int64_t K, const LrGeom& g,
                                 const RopeArg& ra, const float* cos_t, const float* sin_t, const int32_t* pos, const int32_t* bt,
                                 const LrDst& dst, hipStream_t stream) {
    static LdsOnce once;
    if (const hipError_t e = allow_lds(once, reinterpret_cast<const void*>(&linrope_w8_kernel), kLrMaxLds)) return e;
    hipLaunchKernelGGL(linrope_w8_kernel, dim3(static_cast<unsigned>(pl.grid)), dim3(kLrBlock), pl.lds, stream, act, M, wt, qo, K,
                       pl.row_stride, g, ra, cos_t, sin_t, pos, bt, dst);
    return hipGetLastError();
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_linrope_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// what this library serves; everything else that is legal belongs to lsq_hip_lindec_w8.h, lsq_hip_rope_w8.h and lsq_hip_attn_paged_w8.h
int check_served(const char* what, const lsq_linrope_w8_geom& g, int64_t K, bool aligned, const Dest (&d)[3]) {
    const char* other = "the composition of lsq_hip_lindec_w8.h, lsq_hip_rope_w8.h and lsq_hip_attn_paged_w8.h serves it";
    if (int rc = check_rows_served(what, g, other)) return rc;
    if (K <= 0 || K % 16 != 0 || K > lsq::kW8MaxK)
        return fail(LSQ_EINVAL, "%s: K = %lld, the kernel serves multiples of 16 up to %d (%s)", what, static_cast<ll>(K), lsq::kW8MaxK, other);
    if (int rc = check_geom_served(what, g, d, other)) return rc;
    if (!aligned)
        return fail(LSQ_EINVAL, "%s: x_levels, w_levels, cos, sin, rq, k and v must be 16-byte aligned (%s)", what, other);
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_linrope_w8_abi_version(void) { return LSQ_LINROPE_W8_ABI_VERSION; }

const char* lsq_linrope_w8_last_error(void) { return g_last_error; }

int lsq_linrope_w8(int level_dtype, const void* x_levels, const void* s_x, const void* zx, const lsq_linrope_w8_proj* proj, int64_t N,
                   int64_t K, const lsq_linrope_w8_geom* geom, const lsq_rope_w8_in* qkv, const lsq_rope_w8_out* rot, const void* cos,
                   const void* sin, const void* positions, const void* block_table, void* rq, void* k, void* v, void* stream) {
    const char* what = "lsq_linrope_w8";
    Dest d[3];
    if (int rc = check_geom(what, geom, d)) return rc;
    const int64_t M = geom->B * geom->T;
    if (int rc = check_linear_shape(what, M, N, K)) return rc;
    if (N != (geom->H + 2 * geom->Hkv) * geom->D)
        return fail(LSQ_EINVAL, "%s: the weight has N = %lld rows, (H + 2 Hkv) D = %lld are needed", what, static_cast<ll>(N),
                    static_cast<ll>((geom->H + 2 * geom->Hkv) * geom->D));
    if (int rc = check_levels_in(what, kCodes, level_dtype, x_levels, s_x, zx)) return rc;
    // the projection, said as csrc/requant_w8/ says it
    if (!proj) return fail(LSQ_EINVAL, "%s: NULL projection", what);
    if (!rq || !k || !v) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    int mid = 0;
    lsq::W8OutArg qo{};
    if (int rc = check_out(what, proj->out, mid, qo)) return rc;
    if (qo.relu) return fail(LSQ_EINVAL, "%s: relu is set: the rotation takes the projection's own levels (not served)", what);
    if (int rc = check_weights(what, kCodes, mid, static_cast<int>(proj->w_level_dtype), proj->w_levels, proj->w_scale, proj->w_zero, proj->bias,
                               static_cast<int>(proj->bias_dtype), rq))
        return rc;
    // the rotation's sides and tables, said as csrc/rope_w8/ says them
    lsq::RopeArg ra{};
    if (int rc = check_rotation(what, geom, mid, qkv, rot, cos, sin, positions, block_table, ra)) return rc;
    // the destinations against everything that is read, and against each other
    void* const dp[3] = {rq, k, v};
    if (int rc = check_dest_overlap(what, geom, d, dp, x_levels, M * K, proj->w_levels, N * K, cos, sin, positions, block_table)) return rc;
    const bool aligned = aligned_to(x_levels, 16) && aligned_to(proj->w_levels, 16) && aligned_to(cos, 16) && aligned_to(sin, 16) &&
                         aligned_to(rq, 16) && aligned_to(k, 16) && aligned_to(v, 16);
    if (int rc = check_served(what, *geom, K, aligned, d)) return rc;
    const lsq::LrPlan pl = lsq::plan_linrope(*geom, K, aligned);
    const lsq::W8Weight wt = weight_arg(static_cast<int>(proj->w_level_dtype), proj->w_levels, proj->w_scale, proj->w_zero, proj->bias,
                                        static_cast<int>(proj->bias_dtype));
    const lsq::W8Act act = levels_act(level_dtype, x_levels, s_x, zx);
    const bool qkv_signed = std::max(proj->out->quant_max, proj->out->type_max) <= 127;
    const lsq::LrGeom g = kernel_geom(geom, d, pl.rotate + pl.pass + pl.copy, qkv_signed);
    const lsq::LrDst dst{{static_cast<uint8_t*>(rq), static_cast<uint8_t*>(k), static_cast<uint8_t*>(v)}};
    return hip_status(lsq::linrope_launch(pl, act, static_cast<int>(M), wt, qo, K, g, ra, static_cast<const float*>(cos),
                                          static_cast<const float*>(sin), static_cast<const int32_t*>(positions),
                                          static_cast<const int32_t*>(block_table), dst, static_cast<hipStream_t>(stream)), what);
}

int lsq_linrope_w8_plan(const lsq_linrope_w8_geom* geom, int64_t K, int aligned, int32_t* out9) {
    const char* what = "lsq_linrope_w8_plan";
    Dest d[3];
    if (int rc = check_geom(what, geom, d)) return rc;
    if (K < 0) return fail(LSQ_EINVAL, "%s: negative K = %lld", what, static_cast<ll>(K));
    if (!out9) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::LrPlan pl = lsq::plan_linrope(*geom, K, aligned != 0);
    out9[0] = pl.served;
    out9[1] = static_cast<int32_t>(pl.grid);
    out9[2] = pl.block;
    out9[3] = pl.lds;
    out9[4] = pl.chunks;
    out9[5] = pl.x_resident;
    out9[6] = pl.rotate;
    out9[7] = pl.pass;
    out9[8] = pl.copy;
    return LSQ_OK;
}

}  // extern "C"
