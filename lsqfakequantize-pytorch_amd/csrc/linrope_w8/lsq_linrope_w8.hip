// lsq_linrope_w8.hip -- the qkv projection of an attention block's decode step (M <= 16) with the rotary embedding and the KV-cache
// append in its epilogue on gfx950 (include/lsq_hip_linrope_w8.h, which states what is served): the kernel and the C ABI of
// liblsq_hip_linrope_w8.so.
//
// Nothing is defined here.  The exact integer is csrc/qlinear_w8/lsq_w8_shared.hpp's w8_exact on the raw sums, the qkv byte is
// csrc/requant_w8/lsq_requant_w8_tiles.hpp's w8q_byte, the rotation is rope_dequant and rope_pair on two qkv bytes, its level
// csrc/lsq_w8_out_side.hpp's w8o_byte.  rope_dequant, rope_pair and their constants are TWIN COPIES of those in
// csrc/rope_w8/lsq_rope_w8.hip, a translation unit: a fix there belongs here too.
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
#include "../lsq_w8_out_side.hpp"
#include "../../../include/lsq_hip_linrope_w8.h"

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
constexpr int kLrPlaceBytes = 16 * (4 + 4 + 3 * 8); // p, flags and three offsets of 16 rows
constexpr int kLrFixedLds = kLrRedBytes + 4 * kLrTile + kLrPlaceBytes;
constexpr int kLrMaxLds = kLrFixedLds + LSQ_LINROPE_W8_MAX_ROWS * (kLrChunk + kW8RowPad);
constexpr int kLrQ = 1, kLrK = 2, kLrV = 4;         // the write flags of a row
static_assert(kLrWaves * kW8Step == kLrChunk, "the waves' steps cover a chunk");
static_assert(kLrFixedLds % 16 == 0, "the rows of x are read as 16-byte packets");

// ---- TWIN COPIES of csrc/rope_w8/lsq_rope_w8.hip's RopeArg, RopeQ, rope_constants, rope_dequant and rope_pair ----
struct RopeArg {            // kernel argument: the constants
    const float* s_x;
    const int32_t* zx;
    const float* scale;     // the output quantizer
    const float* shift;
    float qmin, qmax, tmin, tmax;
    int mid;                // LSQ_F32 / LSQ_BF16 / LSQ_F16
};

struct RopeQ : W8OutSide {  // the constants, read once per thread
    float s_x, zx, off;     // off: 128.0f for int8 levels, what the flipped byte carries too much; 0.0f for uint8
};

__device__ __forceinline__ RopeQ rope_constants(const RopeArg& a, uint32_t flip) {
    RopeQ q;
    w8o_constants(q, a);
    q.s_x = a.s_x[0];
    q.zx = static_cast<float>(a.zx[0]);
    q.off = flip ? 128.0f : 0.0f;
    return q;
}

// LevelsTensor.dequantize(mid) of byte I of a packet's word `w`, flipped by 0x80 per byte for int8 levels so that it holds
// level + off as an unsigned byte: float(level) = float(byte) - off exactly, then (float(level) - float(zero)) * scale, rounded to mid
template <int I>
__device__ __forceinline__ float rope_dequant(uint32_t w, const RopeQ& q) {
    const float l = __fsub_rn(static_cast<float>((w >> (8 * I)) & 0xffu), q.off);
    return w8o_round_mid(__fmul_rn(__fsub_rn(l, q.zx), q.s_x), q.mid);
}

// the pair of the contract: two rounded fp32 products and one rounded fp32 difference / sum, each rounded to mid; never an fma
__device__ __forceinline__ void rope_pair(float di, float dj, float c, float s, int mid, float& ui, float& uj) {
    const float ic = w8o_round_mid(__fmul_rn(di, c), mid), js = w8o_round_mid(__fmul_rn(dj, s), mid);
    const float jc = w8o_round_mid(__fmul_rn(dj, c), mid), is = w8o_round_mid(__fmul_rn(di, s), mid);
    ui = w8o_round_mid(__fsub_rn(ic, js), mid);
    uj = w8o_round_mid(__fadd_rn(jc, is), mid);
}
// ---- end of the twin copies ----

struct LrGeom {             // kernel argument; the host has checked that every offset fits 63 bits
    int64_t row_s[3];       // q: batch; k, v: batch (dense) or page (paged)
    int64_t tok_s[3];       // q: token; k, v: token (dense) or slot (paged)
    int64_t head_s[3];
    int T, H, Hkv, D, R, P;
    int limit;              // tokens a sequence can hold: Tmax (dense) or Mp ps (paged)
    int paged, Np, ps, bt_ld;
    int items;
    uint32_t flip;          // 0x80 for int8 qkv levels (biased by 128 before rope_dequant), 0 for uint8
};

struct LrDst {              // kernel argument: rq, k, v
    uint8_t* p[3];
};

__global__ __launch_bounds__(kLrBlock) void linrope_w8_kernel(W8Act act, int M, W8Weight wt, W8OutArg qkv_out, int64_t K, int row_stride,
                                                             LrGeom g, RopeArg ra, const float* __restrict__ cos_t,
                                                             const float* __restrict__ sin_t, const int32_t* __restrict__ pos,
                                                             const int32_t* __restrict__ bt, LrDst dst) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t* redP = reinterpret_cast<int32_t*>(smem);       // [strip A, B][wave][lane][register]
    int32_t* redS = redP + 2 * kLrRedP;                     // [wave][row]
    int32_t* redC = redS + kLrRedV;                         // [strip A, B][wave][column]
    unsigned char* tiles = smem + kLrRedBytes;              // [qkv A, qkv B, out A, out B][16][16]
    int64_t* pl_off = reinterpret_cast<int64_t*>(tiles + 4 * kLrTile);     // [q, k, v][row]
    int32_t* pl_p = reinterpret_cast<int32_t*>(pl_off + 3 * 16);           // [row]
    int32_t* pl_flags = pl_p + 16;                                         // [row]
    unsigned char* xs = smem + kLrFixedLds;

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const W8Const ac = w8_constants(act);
    const uint32_t flipw = wt.off ? 0x80808080u : 0u;
    const int64_t n_p = K / 16;                             // 16-byte packets per row
    const int64_t n_chunks = (K + kLrChunk - 1) / kLrChunk;
    const int first_item = static_cast<int>(blockIdx.x);
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const int ipd = g.D / 32, ur = g.R / 32;                // items of a head, and those of them that rotate

    // where the rows go, once per workgroup
    if (tid < 16) {
        int flags = 0, p = 0;
        int64_t oq = 0, ok = 0, ov = 0;
        if (tid < M) {
            const int b = tid / g.T, t = tid - b * g.T;
            const int64_t pp = (pos ? static_cast<int64_t>(pos[b]) : 0) + t;
            const bool in_tables = pp >= 0 && pp < g.P;
            if (in_tables) {
                flags |= kLrQ;
                p = static_cast<int>(pp);
                oq = b * g.row_s[0] + t * g.tok_s[0];
            }
            if (pp >= 0 && pp < g.limit) {
                int64_t outer = b, tok = pp;
                bool there = true;
                if (g.paged) {
                    const int e = bt[static_cast<int64_t>(b) * g.bt_ld + pp / g.ps];
                    there = e >= 0 && e < g.Np;             // a wrong entry must not land in another sequence's page
                    outer = e;
                    tok = pp % g.ps;
                }
                if (there) {
                    flags |= kLrV | (in_tables ? kLrK : 0);
                    ok = outer * g.row_s[1] + tok * g.tok_s[1];
                    ov = outer * g.row_s[2] + tok * g.tok_s[2];
                }
            }
        }
        pl_off[tid] = oq;
        pl_off[16 + tid] = ok;
        pl_off[32 + tid] = ov;
        pl_p[tid] = p;
        pl_flags[tid] = flags;
    }
    __syncthreads();                                        // placement written

    for (int item = first_item; item < g.items; item += static_cast<int>(gridDim.x)) {
        const int head = item / ipd, u = item - head * ipd;
        const int kind = head < g.H ? 0 : (head < g.H + g.Hkv ? 1 : 2);    // q, k, v
        const int hh = head - (kind == 0 ? 0 : (kind == 1 ? g.H : g.H + g.Hkv));
        const bool rot = kind < 2 && u < ur;
        const int fA = rot ? 16 * u : 32 * u;               // (R = 32 ur: the strips beyond R start at 32 u too)
        const int fB = rot ? fA + g.R / 2 : fA + 16;
        const int bit = 1 << kind;
        const int64_t nA = static_cast<int64_t>(head) * g.D + fA, nB = static_cast<int64_t>(head) * g.D + fB;
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
    const bool strides = ge.q_sb % 16 == 0 && ge.q_st % 16 == 0 && ge.q_sh % 16 == 0 && ge.k_so % 16 == 0 && ge.k_st % 16 == 0 &&
                         ge.k_sh % 16 == 0 && ge.v_so % 16 == 0 && ge.v_st % 16 == 0 && ge.v_sh % 16 == 0;
    if (!(aligned && strides && M >= 1 && M <= LSQ_LINROPE_W8_MAX_ROWS && K > 0 && K % 16 == 0 && K <= kW8MaxK &&
          ge.style == LSQ_ROPE_W8_HALF && ge.D % 32 == 0 && ge.R % 32 == 0 && ge.R >= 32))
        return pl;
    const int64_t cus = device_info().cu_count;
    pl.served = 1;
    pl.block = kLrBlock;
    pl.chunks = static_cast<int>((K + kLrChunk - 1) / kLrChunk);
    pl.x_resident = pl.chunks == 1 ? 1 : 0;
    pl.row_stride = static_cast<int>(std::min<int64_t>((K + kW8Step - 1) / kW8Step * kW8Step, kLrChunk)) + kW8RowPad;
    pl.lds = kLrFixedLds + static_cast<int>(M) * pl.row_stride;
    pl.rotate = static_cast<int>((ge.H + ge.Hkv) * (ge.R / 32));
    pl.pass = static_cast<int>((ge.H + ge.Hkv) * ((ge.D - ge.R) / 32));
    pl.copy = static_cast<int>(ge.Hkv * (ge.D / 32));
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

constexpr int64_t kMaxExtent = INT32_MAX / 4;       // 29 bits, as lsq_hip_rope_w8.h
constexpr int64_t kMaxOffset = int64_t{1} << 58;

// the (outer, token, head) rows of a destination must not overlap each other: rope_self_overlap of csrc/rope_w8/lsq_rope_w8.hip
bool rows_overlap(const int64_t (&strides)[3], const int64_t (&extents)[3], int64_t cols) {
    int64_t st[3] = {strides[0], strides[1], strides[2]}, ex[3] = {extents[0], extents[1], extents[2]};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (st[j] < st[i]) {
                std::swap(st[i], st[j]);
                std::swap(ex[i], ex[j]);
            }
    int64_t span = cols;
    for (int i = 0; i < 3; ++i) {
        if (ex[i] == 1) continue;
        if (st[i] < span) return true;
        span += (ex[i] - 1) * st[i];
    }
    return false;
}

struct Dest {               // one destination: its name, strides and extents (outer, token, head) and its bytes
    const char* name;
    int64_t st[3], ex[3], bytes;
};

// the geometry's checks, host only (the plan makes them too); fills the three destinations
int check_geom(const char* what, const lsq_linrope_w8_geom* g, Dest (&d)[3]) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (g->B < 1 || g->T < 1 || g->H < 1 || g->Hkv < 1 || g->D < 1)
        return fail(LSQ_EINVAL, "%s: B = %lld, T = %lld, H = %lld, Hkv = %lld, D = %lld: every extent must be at least 1", what,
                    static_cast<ll>(g->B), static_cast<ll>(g->T), static_cast<ll>(g->H), static_cast<ll>(g->Hkv), static_cast<ll>(g->D));
    if (g->B > kMaxExtent || g->T > kMaxExtent || g->H > kMaxExtent || g->Hkv > kMaxExtent || g->D > kMaxExtent ||
        (g->H + 2 * g->Hkv) * g->D > kMaxExtent)
        return fail(LSQ_EINVAL, "%s: an extent is beyond 29 bits", what);
    if (g->style != LSQ_ROPE_W8_HALF && g->style != LSQ_ROPE_W8_INTERLEAVED)
        return fail(LSQ_EINVAL, "%s: style must be LSQ_ROPE_W8_HALF (0) or LSQ_ROPE_W8_INTERLEAVED (1), got %lld", what, static_cast<ll>(g->style));
    if (g->P < 1) return fail(LSQ_EINVAL, "%s: the tables hold P = %lld positions, at least 1 is needed", what, static_cast<ll>(g->P));
    if (g->P > kMaxExtent) return fail(LSQ_EINVAL, "%s: P = %lld is beyond 29 bits", what, static_cast<ll>(g->P));
    if (g->R < 2 || g->R % 2 != 0 || g->R > g->D)
        return fail(LSQ_EINVAL, "%s: the rotary dimension R = %lld must be even, at least 2 and at most D = %lld", what, static_cast<ll>(g->R),
                    static_cast<ll>(g->D));
    if (g->paged != 0 && g->paged != 1) return fail(LSQ_EINVAL, "%s: paged must be 0 or 1, got %lld", what, static_cast<ll>(g->paged));
    int64_t outer = g->B, toks = g->Tmax;
    if (g->paged) {
        const lsq_attn_paged_w8_pages& pg = g->pages;
        if (pg.Np < 1 || pg.ps < 1 || pg.Mp < 1)
            return fail(LSQ_EINVAL, "%s: Np = %lld pages of ps = %lld slots and Mp = %lld table entries: every extent must be at least 1", what,
                        static_cast<ll>(pg.Np), static_cast<ll>(pg.ps), static_cast<ll>(pg.Mp));
        if (pg.Np > kMaxExtent || pg.ps > kMaxExtent || pg.Mp > kMaxExtent || pg.Mp > kMaxExtent / pg.ps)
            return fail(LSQ_EINVAL, "%s: Np, or the Mp ps = %lld x %lld tokens of a sequence, are beyond 29 bits", what, static_cast<ll>(pg.Mp),
                        static_cast<ll>(pg.ps));
        if (pg.bt_ld < pg.Mp || pg.bt_ld > kMaxExtent)
            return fail(LSQ_EINVAL, "%s: the block table's rows are bt_ld = %lld apart, at least Mp = %lld (and at most 2^29) is needed", what,
                        static_cast<ll>(pg.bt_ld), static_cast<ll>(pg.Mp));
        outer = pg.Np;
        toks = pg.ps;
    } else if (g->Tmax < 1 || g->Tmax > kMaxExtent) {
        return fail(LSQ_EINVAL, "%s: the caches hold Tmax = %lld tokens, 1 to 2^29 are served", what, static_cast<ll>(g->Tmax));
    }
    d[0] = Dest{"rq", {g->q_sb, g->q_st, g->q_sh}, {g->B, g->T, g->H}, 0};
    d[1] = Dest{"k", {g->k_so, g->k_st, g->k_sh}, {outer, toks, g->Hkv}, 0};
    d[2] = Dest{"v", {g->v_so, g->v_st, g->v_sh}, {outer, toks, g->Hkv}, 0};
    for (Dest& t : d) {
        t.bytes = g->D;
        for (int i = 0; i < 3; ++i) {
            if (t.st[i] < 0 || t.st[i] > kMaxOffset / t.ex[i])
                return fail(LSQ_EINVAL, "%s: the strides (%lld, %lld, %lld) of %s must not be negative and must keep every offset within 2^58",
                            what, static_cast<ll>(t.st[0]), static_cast<ll>(t.st[1]), static_cast<ll>(t.st[2]), t.name);
            t.bytes += (t.ex[i] - 1) * t.st[i];
        }
        if (rows_overlap(t.st, t.ex, g->D))
            return fail(LSQ_EINVAL, "%s: under %s's strides (%lld, %lld, %lld) two rows of D = %lld bytes overlap", what, t.name,
                        static_cast<ll>(t.st[0]), static_cast<ll>(t.st[1]), static_cast<ll>(t.st[2]), static_cast<ll>(g->D));
    }
    return LSQ_OK;
}

// what this library serves; everything else that is legal belongs to lsq_hip_lindec_w8.h, lsq_hip_rope_w8.h and lsq_hip_attn_paged_w8.h
int check_served(const char* what, const lsq_linrope_w8_geom& g, int64_t K, bool aligned, const Dest (&d)[3]) {
    const char* other = "the composition of lsq_hip_lindec_w8.h, lsq_hip_rope_w8.h and lsq_hip_attn_paged_w8.h serves it";
    if (g.B * g.T > LSQ_LINROPE_W8_MAX_ROWS)
        return fail(LSQ_EINVAL, "%s: B T = %lld rows of x, the kernel serves 1 to %d (%s)", what, static_cast<ll>(g.B * g.T),
                    LSQ_LINROPE_W8_MAX_ROWS, other);
    if (K <= 0 || K % 16 != 0 || K > lsq::kW8MaxK)
        return fail(LSQ_EINVAL, "%s: K = %lld, the kernel serves multiples of 16 up to %d (%s)", what, static_cast<ll>(K), lsq::kW8MaxK, other);
    if (g.style != LSQ_ROPE_W8_HALF) return fail(LSQ_EINVAL, "%s: the interleaved pairing is not served (%s)", what, other);
    if (g.D % 32 != 0 || g.R % 32 != 0)
        return fail(LSQ_EINVAL, "%s: D = %lld and R = %lld, the kernel serves multiples of 32 (%s)", what, static_cast<ll>(g.D),
                    static_cast<ll>(g.R), other);
    for (const Dest& t : d)
        if (t.st[0] % 16 || t.st[1] % 16 || t.st[2] % 16)
            return fail(LSQ_EINVAL, "%s: the strides (%lld, %lld, %lld) of %s must be multiples of 16 bytes (%s)", what, static_cast<ll>(t.st[0]),
                        static_cast<ll>(t.st[1]), static_cast<ll>(t.st[2]), t.name, other);
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
    int64_t y_elem = 1;
    if (!qkv || !qkv->s_x || !qkv->zx) return fail(LSQ_EINVAL, "%s: NULL input side of the rotation, s_x or zx", what);
    if (!rot) return fail(LSQ_EINVAL, "%s: NULL output description of the rotation", what);
    if (!cos || !sin) return fail(LSQ_EINVAL, "%s: NULL cos or sin", what);
    if (!aligned_to(qkv->s_x, 4) || !aligned_to(qkv->zx, 4)) return fail(LSQ_EINVAL, "%s: the rotation's s_x and zx must be element-aligned", what);
    if (!aligned_to(cos, 4) || !aligned_to(sin, 4)) return fail(LSQ_EINVAL, "%s: cos and sin must be element-aligned", what);
    if (int rc = check_out_side(what, *rot, ra, y_elem)) return rc;
    if (!rot->out_scale) return fail(LSQ_EINVAL, "%s: NULL out_scale and out_shift: a floating rq is not served (lsq_hip_rope_w8.h)", what);
    if (rot->mid_dtype != mid) return fail(LSQ_EINVAL, "%s: the projection and the rotation must have one mid_dtype", what);
    ra.s_x = static_cast<const float*>(qkv->s_x);
    ra.zx = static_cast<const int32_t*>(qkv->zx);
    if (positions && !aligned_to(positions, 4)) return fail(LSQ_EINVAL, "%s: positions must be 4-byte aligned", what);
    if (geom->paged && (!block_table || !aligned_to(block_table, 4)))
        return fail(LSQ_EINVAL, "%s: a paged call needs a block table, 4-byte aligned", what);
    // the destinations against everything that is read, and against each other
    void* const dp[3] = {rq, k, v};
    const int64_t t_bytes = geom->P * (geom->R / 2) * 4;
    const int64_t bt_bytes = geom->paged ? ((geom->B - 1) * geom->pages.bt_ld + geom->pages.Mp) * 4 : 0;
    struct In { const char* name; const void* p; int64_t bytes; };
    const In ins[] = {{"x", x_levels, M * K}, {"the weight", proj->w_levels, N * K}, {"cos", cos, t_bytes}, {"sin", sin, t_bytes},
                      {"positions", positions, 4 * geom->B}, {"the block table", block_table, bt_bytes}};
    for (int i = 0; i < 3; ++i) {
        for (const In& in : ins)
            if (in.p && in.bytes && overlap(dp[i], d[i].bytes, in.p, in.bytes))
                return fail(LSQ_EINVAL, "%s: %s's %lld bytes overlap %s", what, d[i].name, static_cast<ll>(d[i].bytes), in.name);
        for (int j = i + 1; j < 3; ++j)
            if (overlap(dp[i], d[i].bytes, dp[j], d[j].bytes))
                return fail(LSQ_EINVAL, "%s: %s's %lld bytes overlap %s's %lld", what, d[i].name, static_cast<ll>(d[i].bytes), d[j].name,
                            static_cast<ll>(d[j].bytes));
    }
    const bool aligned = aligned_to(x_levels, 16) && aligned_to(proj->w_levels, 16) && aligned_to(cos, 16) && aligned_to(sin, 16) &&
                         aligned_to(rq, 16) && aligned_to(k, 16) && aligned_to(v, 16);
    if (int rc = check_served(what, *geom, K, aligned, d)) return rc;
    const lsq::LrPlan pl = lsq::plan_linrope(*geom, K, aligned);
    const lsq::W8Weight wt = weight_arg(static_cast<int>(proj->w_level_dtype), proj->w_levels, proj->w_scale, proj->w_zero, proj->bias,
                                        static_cast<int>(proj->bias_dtype));
    const lsq::W8Act act = levels_act(level_dtype, x_levels, s_x, zx);
    const bool qkv_signed = std::max(proj->out->quant_max, proj->out->type_max) <= 127;
    const int64_t limit = geom->paged ? geom->pages.Mp * geom->pages.ps : geom->Tmax;
    lsq::LrGeom g{};
    for (int i = 0; i < 3; ++i) {
        g.row_s[i] = d[i].st[0];
        g.tok_s[i] = d[i].st[1];
        g.head_s[i] = d[i].st[2];
    }
    g.T = static_cast<int>(geom->T);
    g.H = static_cast<int>(geom->H);
    g.Hkv = static_cast<int>(geom->Hkv);
    g.D = static_cast<int>(geom->D);
    g.R = static_cast<int>(geom->R);
    g.P = static_cast<int>(geom->P);
    g.limit = static_cast<int>(limit);
    g.paged = static_cast<int>(geom->paged);
    g.Np = geom->paged ? static_cast<int>(geom->pages.Np) : 0;
    g.ps = geom->paged ? static_cast<int>(geom->pages.ps) : 1;
    g.bt_ld = geom->paged ? static_cast<int>(geom->pages.bt_ld) : 0;
    g.items = pl.rotate + pl.pass + pl.copy;
    g.flip = qkv_signed ? 0x80u : 0u;
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
