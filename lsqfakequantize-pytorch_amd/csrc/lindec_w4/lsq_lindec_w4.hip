// lsq_lindec_w4.hip -- the decode shape (M <= 16) of the W4A8 / W2A8 linears with an 8-bit output on gfx950
// (include/lsq_hip_lindec_w4.h, which states the contract and what is served): the kernel and the C ABI of liblsq_hip_lindec_w4.so.
//
// Nothing is defined here.  v, the fp32 value before the output side, is csrc/qlinear_a8/lsq_qlinear_a8.hip's matrix-core kernel's:
// the same exact integer I per group, one conversion, acc + qscale * f, the same assignment of spans to waves, the same order of
// the sum over the waves, * s_x, + bias.  The byte is csrc/requant_w8/'s w8q_byte or csrc/resadd_w8/'s w8r_byte from their v on
// (lsq_lindec_w4_shared.hpp's w4q_byte and w4r_byte: those functions' steps after v, as functions of v; the constants are those
// headers').  What csrc/linglu_w4/ needs too -- the cut of K, the staging of x, the cursor and step structs -- lies in that header.
//
// ONE KERNEL TEXT, lindec_w4_kernel<BITS, PAIR, RES>, 1024 threads = 16 waves, a persistent grid of min(ceil(N / 16), CUs)
// workgroups on tiles of 16 output columns (rows of the weight); lane (n = lane & 15, q = lane >> 4) reads row tile * 16 + n.
//  * WEIGHT STREAM.  A load step is 4 packets of 16 bytes of each of the 16 rows (lane: packet p0 + q, non-temporal).  FOUR steps
//    are in flight per wave, 64 bytes per lane; a step is reissued as soon as its MFMAs are done.  A chunk's first four are issued
//    before x is staged, and the NEXT TILE's first four before this tile's epilogue, so the stream does not stop at the epilogue's
//    three barriers.  A group's qscale and qzero are fetched ONCE, with the step that holds the group's last packet, by ONE of
//    the row's four lanes: lane (n, q) fetches for the group that ends at place q of the step (a place is one MFMA: PAIR two per
//    step, else four), and hands the pair to the row's other lanes over the LDS crossbar when the group ends.  A step in flight is
//    six registers whatever the format, and a group of 128 four-bit elements costs one pair of loads per four packets, not four.
//  * X.  Staged once per workgroup and chunk (at most 4096 k, whole spans) from 16-byte loads of the level bytes, ^ 0x80 for
//    uint8, each block of 16 bytes permuted into the order in which the nibble / crumb masks hand the codes of a dword to the
//    MFMA (w4_lds_pos: csrc/qlinear_a8/'s a8_lds_pos); rows 16 bytes further apart than their data.  sum a - G z per (row, group)
//    is formed from the staged bytes.  When one chunk holds K, x and those sums stay in LDS across the workgroup's tiles.
//  * MFMA.  v_mfma_i32_16x16x64_i8 on the codes as unsigned nibbles / crumbs after the 4 x 4 lane transpose of a step
//    (transpose_over_rows), PAIR: two adjacent packets of one group per MFMA; an all-ones A operand gives sum c.  When a group ends
//    I = P - z C - qzero (sum a - G z) in 32 bits if every |qzero| of the wave's columns is at most 256, else in 64.
//  * EPILOGUE.  The waves' fp32 tiles meet in LDS; thread tid < 256 sums one output in wave order, forms the byte and writes it into
//    a [16][16] byte tile; after a barrier lane m < M of wave 0 stores row m as ONE 16-byte packet (N % 16 == 0 and y 16-byte
//    aligned), else the tile goes out byte by byte along n.
//  * RESIDUAL (RES).  Lane m < M of wave 0 loads the 16 residual bytes of row m at the top of the tile -- behind the weight
//    packets already in flight -- and parks them in the byte tile at once (no register is held across the K loop); the thread that
//    forms output (m, c) reads its residual byte there and overwrites it (csrc/lindec_w8/'s scheme).  Otherwise the tile is filled
//    byte by byte after the K loop.
//  * REGISTERS.  1024 threads leave 128 VGPRs; four steps in flight take 24 of them, and one MFMA's operands are read at a time
//    (a scheduling barrier per MFMA).  No instantiation has scratch (profiles/r38_lindec_w4_isa.txt).
//  Rows >= M and columns >= N are never written, neither to LDS nor to memory.
// LDS: 16 KB of partial sums, 256 bytes of byte tile, M rows of x of at most 4096 + 16 bytes, M * groups-per-chunk int32: up to
// 88.5 KB, behind lsq_qdecode.hpp's opt-in.
#include "lsq_lindec_w4_shared.hpp"
#include "../../../include/lsq_hip_lindec_w4.h"

static_assert(LSQ_LINDEC_W4_MAX_ROWS == 16, "the rows of x are the 16 rows of one MFMA tile");
static_assert(LSQ_A8_U8 == LSQ_REQUANT_W8_U8 && LSQ_A8_I8 == LSQ_REQUANT_W8_I8, "one pair of level codes");

namespace lsq {

// LDS: the partial sums, the byte tile (residual in, y out), the rows of x, the table of sum a - G z
constexpr int kW4MaxLds = kQRedBytes + kW4TileBytes + LSQ_LINDEC_W4_MAX_ROWS * (kQChunk + kQRowPad) + LSQ_LINDEC_W4_MAX_ROWS * (kQChunk / 32) * 4;

template <int BITS, bool PAIR, bool RES>
__global__ __launch_bounds__(kQBlock) void lindec_w4_kernel(W8Act act, int M, W4Weight wt, W4Geom geo, W8OutArg out, W8ResArg res,
                                                           W8PreArg pre, uint8_t* __restrict__ y) {
    constexpr int D = 32 / BITS;                    // elements per dword
    constexpr int BE = 4 * D;                       // elements per 16-byte packet
    constexpr int PER = PAIR ? 2 : 1;               // packets per MFMA
    constexpr int NS = 4 / PER;                     // MFMAs, and so places where a group can end, per step
    static_assert(!PAIR || BITS == 4, "two packets per MFMA only at 4 bits: a 2-bit packet is 64 elements already");
    typedef W4Step Step;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);            // [wave][lane][register]
    unsigned char* tileb = smem + kQRedBytes;               // [16][16]
    unsigned char* xs = tileb + kW4TileBytes;
    int32_t* aeff = reinterpret_cast<int32_t*>(xs + M * geo.row_stride);       // [M][gstride]: sum a - G z

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const W8Const ac = w8_constants(act);
    const int64_t N = geo.N;
    const int n_chunks = geo.n_chunks, chunk_p = geo.chunk_spans * geo.span_p;
    const int tiles = static_cast<int>((N + kQTile - 1) / kQTile), first_tile = static_cast<int>(blockIdx.x);
    const int span_jump = (kQWaves - 1) * geo.span_p, group_jump = (kQWaves - 1) * geo.groups_per_span;
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const bool row_lane = wave == 0 && lane < M;            // the lane that moves row `lane` of the byte tile as one packet

    // the row the lane's load steps read: this tile's, from the prefetch before the epilogue on the next tile's
    const uint8_t* __restrict__ wrow = nullptr;
    int64_t grow = 0;                                       // the row's first group
    auto rows_of = [&](int tile) {
        const int64_t row = std::min<int64_t>(static_cast<int64_t>(tile) * kQTile + nl, N - 1);   // a clamped row computes a value nobody stores
        wrow = wt.codes + row * (geo.n_packets * 16);
        grow = row * geo.n_groups;
    };

    // the load step the cursor points at, and the cursor one step further.  c: the chunk; np: its packets
    auto load_step = [&](Step& s, W4Cursor& cur, int c, int np) {
        s.p = cur.p < np ? cur.p : -1;
        s.raw = u32x4{0u, 0u, 0u, 0u};
        s.qs = 0.0f;
        s.qz = 0;
        if (s.p >= 0) {
            if (s.p + q < np) s.raw = load_code_packet(wrow, static_cast<int64_t>(c) * chunk_p + s.p + q);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                if (s.p + j * PER >= np) continue;
                cur.pig += PER;
                if (cur.pig == geo.ppg) {                   // the group's last packet is in this step: its constants, once
                    const int64_t g = grow + static_cast<int64_t>(c) * geo.chunk_groups + cur.g;
                    if (q == j) {
                        s.qs = wt.qscale[g];
                        s.qz = wt.qzero[g];
                    }
                    cur.pig = 0;
                    ++cur.g;
                }
            }
        }
        cur.p += 4;
        if (++cur.l == geo.steps_per_span) {                // the wave's next span: 16 spans on; a span starts a group and ends one
            cur.l = 0;
            cur.p += span_jump;
            cur.g += group_jump;
        }
    };

    // packets of chunk c
    auto packets_of = [&](int c) { return static_cast<int>(std::min<int64_t>(chunk_p, geo.n_packets - static_cast<int64_t>(c) * chunk_p)); };

    Step s0, s1, s2, s3;
    W4Cursor ld = {0, 0, 0, 0};
    auto prime = [&](int c) {                               // a chunk's first four steps
        ld = W4Cursor{wave * geo.span_p, 0, 0, wave * geo.groups_per_span};
        const int np = packets_of(c);
        load_step(s0, ld, c, np);
        load_step(s1, ld, c, np);
        load_step(s2, ld, c, np);
        load_step(s3, ld, c, np);
    };

    if (first_tile < tiles) {
        rows_of(first_tile);
        prime(0);
    }
    for (int tile = first_tile; tile < tiles; tile += static_cast<int>(gridDim.x)) {
        const int64_t n0 = static_cast<int64_t>(tile) * kQTile;
        if constexpr (RES) {                                // N % 16 == 0: the packet at n0 < N lies inside N.  Parked in the byte tile at
            if (res.packets && row_lane)                    // once (the previous tile's stores are done): no register across the K loop
                *reinterpret_cast<u32x4*>(tileb + lane * kQTile) = *reinterpret_cast<const u32x4*>(res.l + static_cast<int64_t>(lane) * N + n0);
        }
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = 0; c < n_chunks; ++c) {
            const int64_t kc0 = static_cast<int64_t>(c) * geo.chunk_k;
            const int np = packets_of(c);
            if (c > 0) prime(c);                            // (chunk 0: before the loop or before the previous tile's epilogue)
            if (n_chunks > 1 || tile == first_tile) {       // x stays in LDS across tiles when one chunk holds it
                __syncthreads();
                w4_stage_chunk<BITS>(act, ac, M, geo, kc0, np, xs, aeff, tid);
            }

            // the wave's steps of this chunk: spans wave, wave + 16, ...
            i32x4 P = {0, 0, 0, 0}, C = {0, 0, 0, 0};
            int pig = 0, g_local = wave * geo.groups_per_span, sl = 0;      // the compute side's cursor: as ld's, four steps behind
            const unsigned char* xrow = xs + nl * geo.row_stride;
            auto compute_step = [&](const Step& s) {
                uint32_t r[4] = {s.raw.x, s.raw.y, s.raw.z, s.raw.w};
                transpose_over_rows(r);
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const int t = j * PER;
                    if (s.p + t >= np) continue;            // the same for the whole wave
                    const unsigned char* xa = xrow + (s.p + t) * BE;       // this packet's first element in the chunk
                    i32x4 a = {0, 0, 0, 0}, b;
                    if constexpr (BITS == 2) {
                        if (nl < M) a = *reinterpret_cast<const i32x4*>(xa + q * 16);
                        const uint32_t v = r[t];
                        b = i32x4{static_cast<int>(v & 0x03030303u), static_cast<int>((v >> 2) & 0x03030303u),
                                  static_cast<int>((v >> 4) & 0x03030303u), static_cast<int>((v >> 6) & 0x03030303u)};
                    } else {
                        if (nl < M) {
                            const u32x2 lo = *reinterpret_cast<const u32x2*>(xa + q * 8);
                            a.x = static_cast<int>(lo.x);
                            a.y = static_cast<int>(lo.y);
                            if constexpr (PAIR) {
                                const u32x2 hi = *reinterpret_cast<const u32x2*>(xa + BE + q * 8);
                                a.z = static_cast<int>(hi.x);
                                a.w = static_cast<int>(hi.y);
                            }
                        }
                        const uint32_t v = r[t], v2 = PAIR ? r[t + PER - 1] : 0u;
                        b = i32x4{static_cast<int>(v & 0x0F0F0F0Fu), static_cast<int>((v >> 4) & 0x0F0F0F0Fu),
                                  static_cast<int>(v2 & 0x0F0F0F0Fu), static_cast<int>((v2 >> 4) & 0x0F0F0F0Fu)};
                    }
                    P = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, P, 0, 0, 0);
                    C = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b, C, 0, 0, 0);
                    pig += PER;
                    if (pig == geo.ppg) {                   // the group is complete: the same for the whole wave
                        const int32_t qz = w4_from_place(s.qz, lane, j);
                        const float qs = w4_from_place(s.qs, lane, j);
                        const bool far = qz < -kW4FastZero || qz > kW4FastZero;
                        const bool any_far = __ballot(far) != 0;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int m = q * 4 + i;        // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
                            const int ae = m < M ? aeff[m * geo.gstride + g_local] : 0;
                            float f;
                            if (!any_far) {
                                f = static_cast<float>(P[i] - ac.z * C[i] - qz * ae);
                            } else {
                                f = static_cast<float>(static_cast<int64_t>(P[i]) - static_cast<int64_t>(ac.z) * C[i] -
                                                       static_cast<int64_t>(qz) * ae);
                            }
                            acc[i] = __fadd_rn(acc[i], __fmul_rn(qs, f));
                        }
                        P = i32x4{0, 0, 0, 0};
                        C = i32x4{0, 0, 0, 0};
                        pig = 0;
                        ++g_local;
                    }
                    __builtin_amdgcn_sched_barrier(0);      // one MFMA's operands at a time: the registers go to the steps in flight
                }
                if (++sl == geo.steps_per_span) {
                    sl = 0;
                    g_local += group_jump;
                }
            };
            while (s0.p >= 0) {                             // the same for the whole wave; a step is reissued behind its MFMAs
                compute_step(s0);
                load_step(s0, ld, c, np);
                if (s1.p < 0) break;
                compute_step(s1);
                load_step(s1, ld, c, np);
                if (s2.p < 0) break;
                compute_step(s2);
                load_step(s2, ld, c, np);
                if (s3.p < 0) break;
                compute_step(s3);
                load_step(s3, ld, c, np);
            }
        }
        // the next tile's first steps, in flight across this tile's epilogue
        const int next_tile = tile + static_cast<int>(gridDim.x);
        if (next_tile < tiles) {
            rows_of(next_tile);
            prime(0);
        }

        // the waves' tiles, summed in wave order
        *reinterpret_cast<f32x4*>(red + (wave * 64 + lane) * 4) = acc;
        if constexpr (RES) {                                // without packets: the residual tile into the byte tile byte by byte along n
            if (!res.packets && tid < kW4TileBytes) {       // (consecutive lanes on consecutive bytes)
                const int m = tid >> 4;
                const int64_t n = n0 + (tid & 15);
                if (m < M && n < N) tileb[tid] = res.l[static_cast<int64_t>(m) * N + n];
            }
        }
        __syncthreads();
        if (tid < 256) {                                    // one thread per output
            const int l = tid & 63, reg = tid >> 6;
            const int col = l & 15, m = (l >> 4) * 4 + reg;
            const int64_t n = n0 + col;
            if (m < M && n < N) {
                float sum = 0.0f;
#pragma unroll
                for (int w = 0; w < kQWaves; ++w) sum = __fadd_rn(sum, red[(w * 64 + l) * 4 + reg]);
                const float bias = wt.bias ? w8_bias_at(wt.bias, wt.bias_dtype, n) : 0.0f;
                const float v = __fadd_rn(__fmul_rn(sum, ac.s_x), bias);
                const W8OutQ oq = w8q_constants(out);
                unsigned char* at_b = tileb + m * kQTile + col;    // no other thread touches this byte
                if constexpr (RES) *at_b = w4r_byte(v, oq, w8r_pre_constants(pre), w8r_res_constants(res), *at_b);
                else *at_b = w4q_byte(v, oq);
            }
        }
        __syncthreads();
        if (out.packets) {                                  // N % 16 == 0: the tile's 16 columns lie inside N
            if (row_lane) *reinterpret_cast<u32x4*>(y + static_cast<int64_t>(lane) * N + n0) = *reinterpret_cast<const u32x4*>(tileb + lane * kQTile);
        } else if (tid < kW4TileBytes) {
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
struct W4Plan {
    int served, block, lds, chunks, x_resident, store, res_load;
    bool pair;
    int64_t grid;
    W4Geom geo;
};

// the cut of K is csrc/qlinear_a8/'s plan_a8 (matrix-core form): the order of the sum is fixed by it
inline W4Plan plan_lindec_w4(int64_t M, int64_t N, int64_t K, int64_t G, int bits, bool aligned, bool y_aligned, bool res_aligned) {
    W4Plan pl{};
    if (!w4_cut(M, N, K, G, bits, aligned, LSQ_LINDEC_W4_MAX_ROWS, pl.geo, pl.pair)) return pl;
    const W4Geom& g = pl.geo;
    pl.served = 1;
    pl.block = kQBlock;
    pl.lds = kQRedBytes + kW4TileBytes + static_cast<int>(M) * g.row_stride + static_cast<int>(M) * g.gstride * 4;
    pl.chunks = g.n_chunks;
    pl.x_resident = pl.chunks == 1 ? 1 : 0;
    pl.grid = mfma_grid(N, device_info().cu_count);
    pl.store = (N % 16 == 0 && y_aligned) ? LSQ_LINDEC_W4_PACKETS : LSQ_LINDEC_W4_BYTES;
    pl.res_load = (N % 16 == 0 && res_aligned) ? LSQ_LINDEC_W4_PACKETS : LSQ_LINDEC_W4_BYTES;
    return pl;
}

struct W4Call {             // what every instantiation's launcher takes
    W8Act act;
    W4Weight wt;
    W8OutArg out;
    W8ResArg res;
    W8PreArg pre;
    uint8_t* y;
    int M;
};

template <int BITS, bool PAIR, bool RES>
static hipError_t w4_launch(const W4Plan& pl, const W4Call& c, hipStream_t stream) {
    static LdsOnce once;
    if (const hipError_t e = allow_lds(once, reinterpret_cast<const void*>(&lindec_w4_kernel<BITS, PAIR, RES>), kW4MaxLds)) return e;
    hipLaunchKernelGGL((lindec_w4_kernel<BITS, PAIR, RES>), dim3(static_cast<unsigned>(pl.grid)), dim3(kQBlock), pl.lds, stream, c.act,
                       c.M, c.wt, pl.geo, c.out, c.res, c.pre, c.y);
    return hipGetLastError();
}

template <bool RES>
static hipError_t w4_launch_format(const W4Plan& pl, int bits, const W4Call& c, hipStream_t stream) {
    if (bits == 2) return w4_launch<2, false, RES>(pl, c, stream);
    return pl.pair ? w4_launch<4, true, RES>(pl, c, stream) : w4_launch<4, false, RES>(pl, c, stream);
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_lindec_w4.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// what this form serves; everything else that is legal belongs to lsq_hip_qlinear_a8.h and the ops after it
int check_served(const char* what, const lsq::W4Plan& pl, int64_t M, int64_t K, int64_t G, int bits, bool aligned) {
    const char* other = "compose lsq_hip_qlinear_a8.h / lsq_hip_qgemm_a8.h with the per-tensor levels forward";
    if (M > LSQ_LINDEC_W4_MAX_ROWS)
        return fail(LSQ_EINVAL, "%s: M = %lld rows of x, the decode kernel serves 1 to %d (more rows: %s)", what, static_cast<ll>(M),
                    LSQ_LINDEC_W4_MAX_ROWS, other);
    if (!aligned) return fail(LSQ_EINVAL, "%s: codes and x_levels must be 16-byte aligned (otherwise: %s)", what, other);
    if (!pl.served)
        return fail(LSQ_EINVAL, "%s: K = %lld, group_size %lld at %d bits: the decode kernel serves K > 0 and groups of whole 16-byte "
                    "code packets (%d elements) with lcm(group_size, 4 packets) <= %d elements (otherwise: %s)", what, static_cast<ll>(K),
                    static_cast<ll>(G), bits, 128 / bits, lsq::kQChunk, other);
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_lindec_w4_abi_version(void) { return LSQ_LINDEC_W4_ABI_VERSION; }

const char* lsq_lindec_w4_last_error(void) { return g_last_error; }

int lsq_lindec_w4_linear_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, const void* codes,
                                int64_t N, int64_t K, int64_t group_size, int bits, const void* qscale, const void* qzero,
                                const void* bias, int bias_dtype, const lsq_requant_w8_out* out, const lsq_resadd_w8_res* res,
                                const lsq_resadd_w8_pre* pre, void* y, void* stream) {
    const char* what = "lsq_lindec_w4_linear_levels";
    int mid = 0;
    lsq::W4Call c{};
    if (int rc = check_out(what, out, mid, c.out)) return rc;
    if (int rc = check_format(what, M, N, K, group_size, bits)) return rc;
    if (int rc = check_levels_in(what, kCodes, level_dtype, x_levels, s_x, zx)) return rc;
    if (!codes || !qscale || !qzero || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (bias && bias_dtype != LSQ_F32 && bias_dtype != mid)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of mid_dtype, got dtype code %d", what, bias_dtype);
    if (!aligned_to(qscale, 4) || !aligned_to(qzero, 4) || (bias && !aligned_to(bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: qscale, qzero and bias must be element-aligned", what);
    if (res) {
        if (int rc = check_res(what, res, y, M * N, c.res)) return rc;
    } else if (pre) {
        return fail(LSQ_EINVAL, "%s: a pre-quantizer without a residual (the layer's own quantizer is then the output quantizer)", what);
    }
    if (int rc = check_pre(what, pre, c.pre)) return rc;
    const bool aligned = aligned_to(codes, 16) && aligned_to(x_levels, 16);
    const lsq::W4Plan pl = lsq::plan_lindec_w4(M, N, K, group_size, bits, aligned, aligned_to(y, 16), res && aligned_to(res->levels, 16));
    if (int rc = check_served(what, pl, M, K, group_size, bits, aligned)) return rc;
    if (N == 0) return LSQ_OK;
    c.act = levels_act(level_dtype, x_levels, s_x, zx);
    c.wt = lsq::W4Weight{static_cast<const uint8_t*>(codes), static_cast<const float*>(qscale), static_cast<const int32_t*>(qzero), bias,
                         bias_dtype};
    c.out.packets = pl.store == LSQ_LINDEC_W4_PACKETS ? 1 : 0;
    c.res.packets = pl.res_load == LSQ_LINDEC_W4_PACKETS ? 1 : 0;
    c.y = static_cast<uint8_t*>(y);
    c.M = static_cast<int>(M);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return hip_status(res ? lsq::w4_launch_format<true>(pl, bits, c, st) : lsq::w4_launch_format<false>(pl, bits, c, st), what);
}

int lsq_lindec_w4_plan(int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int aligned, int y_aligned, int res_aligned,
                       int32_t* out8) {
    const char* what = "lsq_lindec_w4_plan";
    if (int rc = check_format(what, M, N, K, group_size, bits)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::W4Plan pl = lsq::plan_lindec_w4(M, N, K, group_size, bits, aligned != 0, y_aligned != 0, res_aligned != 0);
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
