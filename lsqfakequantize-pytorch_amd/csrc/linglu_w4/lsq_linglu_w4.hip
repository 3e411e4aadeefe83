// lsq_linglu_w4.hip -- the gate and up projections of a gated MLP's decode step (M <= 16) on packed 4- / 2-bit codes with the gated
// product in their epilogue on gfx950 (include/lsq_hip_linglu_w4.h, which states the contract and what is served): the kernel and
// the C ABI of liblsq_hip_linglu_w4.so.
//
// Nothing is defined here.  For each strip v is csrc/lindec_w4/'s (csrc/qlinear_a8/'s matrix-core kernel's): the same exact integer I
// per group, one conversion, acc + qscale * f, the same assignment of spans to waves, the same order of the sum over the waves,
// * s_x, + bias.  The gate byte and the up byte are csrc/lindec_w4/lsq_lindec_w4_shared.hpp's w4q_byte, the product is
// csrc/glu_w8/lsq_glu_w8_dev.hpp's glu_product on the table entry of the gate byte and glu_dequant of the up byte, its level
// csrc/lsq_w8_out_side.hpp's w8o_byte: the same device functions, compiled into this library.
//
// ONE KERNEL TEXT, linglu_w4_kernel<BITS, PAIR>, 1024 threads = 16 waves: csrc/lindec_w4/'s work split on a PAIR of code strips.
//  * SPLIT.  A workgroup owns 16 product columns c0 .. c0 + 15 -- rows c0 + n of the gate strip and rows c0 + n of the up strip --
//    and walks the tiles in a persistent grid of min(ceil(C / 16), CUs) workgroups.  Lane (n = lane & 15, q = lane >> 4).  The two
//    strips have ONE format and ONE K, so ONE cursor walks both: a PAIR STEP is a load step (4 packets of each of the 16 rows) of
//    the gate strip and the same step of the up strip.
//  * WEIGHT STREAM.  TWO pair steps are in flight per wave: four non-temporal 16-byte packets per lane, lindec_w4's 64 bytes, two of
//    either strip.  A pair step is reissued as soon as its MFMAs are done; a chunk's first two are issued before x is staged, and
//    the NEXT TILE's first two before this tile's epilogue.  A group's qscale and qzero of both strips are fetched once, with the
//    step that holds the group's last packet, by lane (n, q) for the group that ends at place q, and handed to the row's other
//    lanes over the LDS crossbar (w4_from_place) when the group ends.
//  * X.  Staged ONCE per chunk for both strips (w4_stage_chunk: the permuted layout of w4_lds_pos, sum a - G z per (row, group),
//    which does not depend on the strip).  When one chunk holds K both stay in LDS across the workgroup's tiles.
//  * MFMA.  v_mfma_i32_16x16x64_i8 on the codes as unsigned nibbles / crumbs after the 4 x 4 lane transpose of either strip's
//    step.  ONE ds_read of the x operand per place feeds both strips: P_g and C_g (the all-ones A operand), then P_u and C_u -- four
//    MFMAs on four independent accumulators, back to back.  When a group ends, I = P - z C - qzero (sum a - G z) is formed PER STRIP
//    in 32 bits if every |qzero| of the wave's columns in THAT strip is at most 256, else in 64; gate first, then up.
//  * ORDER OF THE SUM.  Each strip has its own fp32 accumulator and its own partial-sum region.  The shared cursor visits the
//    groups of the wave's spans in ascending order, chunk after chunk, exactly as lindec_w4's does, and at every group end each
//    strip's accumulator takes that strip's one rounded product and one rounded add: the interleaving puts the two strips' steps
//    next to each other but never reorders the steps of ONE strip, and no value of one strip enters the other's chain.  The
//    epilogue adds each region in wave order.
//  * EPILOGUE.  Threads 0..255 sum gate output (m, col) in wave order, form v and its byte into a [16][16] gate tile; threads
//    256..511 do the same for up at the same time (whole waves on either side of the select): one barrier.  Thread (m, col) of
//    the first 256 then reads its gate byte and its up byte and writes the product's level into the output tile.  The table is
//    staged once per workgroup into 1 KB of LDS, rounded to mid as glu_w8_packets_kernel rounds it.
//  * STORE.  After one barrier lane m < M of wave 0 stores row m of the output tile as ONE 16-byte packet at y + m C + c0
//    (C % 16 == 0 and y 16-byte aligned), else the tile goes out byte by byte, consecutive lanes on consecutive columns.  Rows
//    >= M and columns >= C are never written, neither to LDS nor to memory.
//  * BARRIERS.  Three per tile (sums written, bytes written, levels written) besides the staging's.  None behind the stores: a
//    region is written again only behind a later barrier than the one its readers have passed -- the sums behind "levels
//    written" (read before "bytes written"), the two byte tiles behind the next "sums written", the output tile behind the next
//    "bytes written".  x and the group sums are rewritten (more than one chunk) behind the staging's own first barrier, which
//    every wave reaches after its last MFMA of the previous chunk.
//  * REGISTERS.  1024 threads leave 128 VGPRs: two pair steps in flight take 24, six accumulators 24, and one place's operands
//    are read at a time (a scheduling barrier per place).  The wave index is read with readfirstlane, so both cursors are scalars,
//    and a lane holds ONE byte offset (its row's packet q) and ONE group index for both strips; what a load adds is a scalar.
//    No instantiation has scratch (profiles/r39_linglu_w4_isa.txt: 104 to 110 VGPRs).
// LDS: 32 KB of partial sums, 768 bytes of tiles, 1 KB of table, M rows of x of at most 4096 + 16 bytes, M * groups-per-chunk int32:
// up to 106 KB, behind lsq_qdecode.hpp's opt-in.
#include "../lindec_w4/lsq_lindec_w4_shared.hpp"
#include "../glu_w8/lsq_glu_w8_dev.hpp"
#include "../../../include/lsq_hip_linglu_w4.h"

static_assert(LSQ_LINGLU_W4_MAX_ROWS == 16, "the rows of x are the 16 rows of one MFMA tile");
static_assert(LSQ_A8_U8 == LSQ_REQUANT_W8_U8 && LSQ_A8_I8 == LSQ_REQUANT_W8_I8, "one pair of level codes");
static_assert(LSQ_GLU_W8_U8 == LSQ_REQUANT_W8_U8 && LSQ_GLU_W8_I8 == LSQ_REQUANT_W8_I8, "one level type code for the three steps");

namespace lsq {

constexpr int kG4RedFloats = kQRedBytes / 4;        // fp32 values of one strip's partial sums
constexpr int kG4TabBytes = 256 * 4;
constexpr int kG4FixedLds = 2 * kQRedBytes + 3 * kW4TileBytes + kG4TabBytes;
constexpr int kG4MaxLds = kG4FixedLds + LSQ_LINGLU_W4_MAX_ROWS * (kQChunk + kQRowPad) + LSQ_LINGLU_W4_MAX_ROWS * (kQChunk / 32) * 4;
static_assert(kG4FixedLds % 16 == 0, "the rows of x are read and written as 16-byte packets");
static_assert(kG4MaxLds <= 160 * 1024, "the LDS of one CDNA4 compute unit");

struct G4Pair {             // kernel argument: the two projections
    W4Weight gate, up;
    W8OutArg gate_out, up_out;
};

template <int BITS, bool PAIR>
__global__ __launch_bounds__(kQBlock) void linglu_w4_kernel(W8Act act, int M, G4Pair pr, W4Geom geo, GluArg ga, const float* __restrict__ table,
                                                           int packets, uint8_t* __restrict__ y) {
    constexpr int D = 32 / BITS;                    // elements per dword
    constexpr int BE = 4 * D;                       // elements per 16-byte packet
    constexpr int PER = PAIR ? 2 : 1;               // packets per MFMA
    constexpr int NS = 4 / PER;                     // MFMAs of one strip, and so places where a group can end, per step
    static_assert(!PAIR || BITS == 4, "two packets per MFMA only at 4 bits: a 2-bit packet is 64 elements already");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);            // [gate, up][wave][lane][register]
    unsigned char* tilesb = smem + 2 * kQRedBytes;          // [gate, up, y][16][16]
    float* tab = reinterpret_cast<float*>(tilesb + 3 * kW4TileBytes);
    unsigned char* xs = smem + kG4FixedLds;
    int32_t* aeff = reinterpret_cast<int32_t*>(xs + M * geo.row_stride);       // [M][gstride]: sum a - G z

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // said to the compiler: the cursors below are scalars
    const int nl = lane & 15, q = lane >> 4;
    const W8Const ac = w8_constants(act);
    const int64_t C = geo.N;
    const int n_chunks = geo.n_chunks, chunk_p = geo.chunk_spans * geo.span_p;
    const int tiles = static_cast<int>((C + kQTile - 1) / kQTile), first_tile = static_cast<int>(blockIdx.x);
    const int span_jump = (kQWaves - 1) * geo.span_p, group_jump = (kQWaves - 1) * geo.groups_per_span;
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};

    // a value of mid already (the contract): the identity, once per entry and not per element.  Read behind the first tile's barriers.
    if (tid < 256) tab[tid] = w8o_round_mid(table[tid], ga.mid);

    // the rows the lane's load steps read: this tile's, from the prefetch before the epilogue on the next tile's
    // (one byte offset and one group index serve both strips: they have one shape)
    // lane_byte: packet q of the row; what a load adds to either is the same for the whole wave
    int64_t lane_byte = 0, row_group = 0;
    auto rows_of = [&](int tile) {
        const int64_t row = std::min<int64_t>(static_cast<int64_t>(tile) * kQTile + nl, C - 1);   // a clamped row computes a value nobody stores
        lane_byte = row * (geo.n_packets * 16) + q * 16;
        row_group = row * geo.n_groups;
    };

    // the pair step the cursor points at, and the cursor one step further.  c: the chunk; np: its packets
    auto load_step = [&](W4Step& sg, W4Step& su, W4Cursor& cur, int c, int np) {
        sg.p = su.p = cur.p < np ? cur.p : -1;
        sg.raw = su.raw = u32x4{0u, 0u, 0u, 0u};
        sg.qs = su.qs = 0.0f;
        sg.qz = su.qz = 0;
        if (sg.p >= 0) {
            if (sg.p + q < np) {
                const int64_t at = lane_byte + static_cast<uint32_t>(c * chunk_p + sg.p) * 16u;      // a row is at most 2^29 bytes
                sg.raw = load_code_packet(pr.gate.codes + at, 0);
                su.raw = load_code_packet(pr.up.codes + at, 0);
            }
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                if (sg.p + j * PER >= np) continue;
                cur.pig += PER;
                if (cur.pig == geo.ppg) {                   // the group's last packet is in this step: both strips' constants, once
                    const int64_t g = row_group + (c * geo.chunk_groups + cur.g);       // a row has at most 2^25 groups
                    if (q == j) {
                        sg.qs = pr.gate.qscale[g];
                        sg.qz = pr.gate.qzero[g];
                        su.qs = pr.up.qscale[g];
                        su.qz = pr.up.qzero[g];
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

    W4Step g0, u0, g1, u1;
    W4Cursor ld = {0, 0, 0, 0};
    auto prime = [&](int c) {                               // a chunk's first two pair steps
        ld = W4Cursor{wave * geo.span_p, 0, 0, wave * geo.groups_per_span};
        const int np = packets_of(c);
        load_step(g0, u0, ld, c, np);
        load_step(g1, u1, ld, c, np);
    };

    if (first_tile < tiles) {
        rows_of(first_tile);
        prime(0);
    }
    for (int tile = first_tile; tile < tiles; tile += static_cast<int>(gridDim.x)) {
        const int64_t c0 = static_cast<int64_t>(tile) * kQTile;
        f32x4 accg = {0.0f, 0.0f, 0.0f, 0.0f}, accu = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = 0; c < n_chunks; ++c) {
            const int np = packets_of(c);
            if (c > 0) prime(c);                            // (chunk 0: before the loop or before the previous tile's epilogue)
            if (n_chunks > 1 || tile == first_tile) {       // x and the group sums stay in LDS across tiles when one chunk holds K
                __syncthreads();
                w4_stage_chunk<BITS>(act, ac, M, geo, static_cast<int64_t>(c) * geo.chunk_k, np, xs, aeff, tid);
            }

            // the wave's steps of this chunk: spans wave, wave + 16, ...
            i32x4 Pg = {0, 0, 0, 0}, Pu = {0, 0, 0, 0}, Cg = {0, 0, 0, 0}, Cu = {0, 0, 0, 0};
            int pig = 0, g_local = wave * geo.groups_per_span, sl = 0;      // the compute side's cursor: as ld's, two pair steps behind
            const unsigned char* xrow = xs + nl * geo.row_stride;
            // the codes of MFMA j of a transposed step as unsigned bytes
            auto codes_of = [&](const uint32_t (&r)[4], int t) {
                const uint32_t v = r[t];
                if constexpr (BITS == 2) {
                    return i32x4{static_cast<int>(v & 0x03030303u), static_cast<int>((v >> 2) & 0x03030303u),
                                 static_cast<int>((v >> 4) & 0x03030303u), static_cast<int>((v >> 6) & 0x03030303u)};
                } else {
                    const uint32_t v2 = PAIR ? r[t + PER - 1] : 0u;
                    return i32x4{static_cast<int>(v & 0x0F0F0F0Fu), static_cast<int>((v >> 4) & 0x0F0F0F0Fu),
                                 static_cast<int>(v2 & 0x0F0F0F0Fu), static_cast<int>((v2 >> 4) & 0x0F0F0F0Fu)};
                }
            };
            // one strip's group is complete: its I in the width its own zero points ask for, its one product and one add per row
            auto end_group = [&](const W4Step& s, int j, const int (&ae)[4], i32x4& P, i32x4& Cs, f32x4& acc) {
                const int32_t qz = w4_from_place(s.qz, lane, j);
                const float qs = w4_from_place(s.qs, lane, j);
                const bool far = qz < -kW4FastZero || qz > kW4FastZero;
                const bool any_far = __ballot(far) != 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float f;
                    if (!any_far) {
                        f = static_cast<float>(P[i] - ac.z * Cs[i] - qz * ae[i]);
                    } else {
                        f = static_cast<float>(static_cast<int64_t>(P[i]) - static_cast<int64_t>(ac.z) * Cs[i] -
                                               static_cast<int64_t>(qz) * ae[i]);
                    }
                    acc[i] = __fadd_rn(acc[i], __fmul_rn(qs, f));
                }
                P = i32x4{0, 0, 0, 0};
                Cs = i32x4{0, 0, 0, 0};
            };
            auto compute_step = [&](const W4Step& sg, const W4Step& su) {
                uint32_t rg[4] = {sg.raw.x, sg.raw.y, sg.raw.z, sg.raw.w};
                uint32_t ru[4] = {su.raw.x, su.raw.y, su.raw.z, su.raw.w};
                transpose_over_rows(rg);
                transpose_over_rows(ru);
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const int t = j * PER;
                    if (sg.p + t >= np) continue;           // the same for the whole wave
                    const unsigned char* xa = xrow + (sg.p + t) * BE;      // this packet's first element in the chunk
                    i32x4 a = {0, 0, 0, 0};                 // ONE read of the x operand for both strips
                    if constexpr (BITS == 2) {
                        if (nl < M) a = *reinterpret_cast<const i32x4*>(xa + q * 16);
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
                    }
                    const i32x4 bg = codes_of(rg, t);
                    Pg = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bg, Pg, 0, 0, 0);
                    Cg = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bg, Cg, 0, 0, 0);
                    const i32x4 bu = codes_of(ru, t);
                    Pu = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bu, Pu, 0, 0, 0);
                    Cu = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bu, Cu, 0, 0, 0);
                    pig += PER;
                    if (pig == geo.ppg) {                   // the group is complete in both strips: the same for the whole wave
                        int ae[4];                          // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
                        for (int i = 0; i < 4; ++i) ae[i] = q * 4 + i < M ? aeff[(q * 4 + i) * geo.gstride + g_local] : 0;
                        end_group(sg, j, ae, Pg, Cg, accg);
                        end_group(su, j, ae, Pu, Cu, accu);
                        pig = 0;
                        ++g_local;
                    }
                    __builtin_amdgcn_sched_barrier(0);      // one place's operands at a time: the registers go to the steps in flight
                }
                if (++sl == geo.steps_per_span) {
                    sl = 0;
                    g_local += group_jump;
                }
            };
            while (g0.p >= 0) {                             // the same for the whole wave; a pair step is reissued behind its MFMAs
                compute_step(g0, u0);
                load_step(g0, u0, ld, c, np);
                if (g1.p < 0) break;
                compute_step(g1, u1);
                load_step(g1, u1, ld, c, np);
            }
        }
        // the next tile's first steps, in flight across this tile's epilogue
        const int next_tile = tile + static_cast<int>(gridDim.x);
        if (next_tile < tiles) {
            rows_of(next_tile);
            prime(0);
        }

        // the waves' tiles of either strip, each summed in wave order
        *reinterpret_cast<f32x4*>(red + (wave * 64 + lane) * 4) = accg;
        *reinterpret_cast<f32x4*>(red + kG4RedFloats + (wave * 64 + lane) * 4) = accu;
        __syncthreads();                                    // sums written
        if (tid < 512) {                                    // one thread per output of either projection: whole waves take a side
            const int side = tid >> 8;                      // 0: gate, 1: up
            const int l = tid & 63, reg = (tid >> 6) & 3;
            const int col = l & 15, m = (l >> 4) * 4 + reg;
            const int64_t n = c0 + col;
            if (m < M && n < C) {
                const float* rs = red + side * kG4RedFloats;
                float sum = 0.0f;
#pragma unroll
                for (int w = 0; w < kQWaves; ++w) sum = __fadd_rn(sum, rs[(w * 64 + l) * 4 + reg]);
                const W4Weight& wt = side ? pr.up : pr.gate;
                const float bias = wt.bias ? w8_bias_at(wt.bias, wt.bias_dtype, n) : 0.0f;
                const float v = __fadd_rn(__fmul_rn(sum, ac.s_x), bias);
                tilesb[side * kW4TileBytes + m * kQTile + col] = w4q_byte(v, w8q_constants(side ? pr.up_out : pr.gate_out));
            }
        }
        __syncthreads();                                    // bytes written
        if (tid < kW4TileBytes) {                           // thread (m, col): consecutive lanes on consecutive columns
            const int m = tid >> 4;
            if (m < M && c0 + (tid & 15) < C) {
                const GluQ gq = glu_constants(ga);
                const uint32_t g = tilesb[tid], u = static_cast<uint32_t>(tilesb[kW4TileBytes + tid]) ^ (ga.flip_u & 0xffu);
                tilesb[2 * kW4TileBytes + tid] = static_cast<unsigned char>(w8o_byte(glu_product(tab[g], glu_dequant<0>(u, gq), gq.mid), gq));
            }
        }
        __syncthreads();                                    // levels written
        const unsigned char* outb = tilesb + 2 * kW4TileBytes;
        if (packets) {                                      // C % 16 == 0: the tile's 16 columns lie inside C
            if (wave == 0 && lane < M)
                *reinterpret_cast<u32x4*>(y + static_cast<int64_t>(lane) * C + c0) = *reinterpret_cast<const u32x4*>(outb + lane * kQTile);
        } else if (tid < kW4TileBytes) {
            const int m = tid >> 4;
            const int64_t n = c0 + (tid & 15);
            if (m < M && n < C) y[static_cast<int64_t>(m) * C + n] = outb[tid];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launcher
// ------------------------------------------------------------------------------------------------
struct G4Plan {
    int served, block, lds, chunks, x_resident, store;
    bool pair;
    int64_t grid;
    W4Geom geo;
};

// the cut of K is csrc/lindec_w4/'s (w4_cut): the order of either strip's sum is fixed by it
inline G4Plan plan_linglu_w4(int64_t M, int64_t C, int64_t K, int64_t G, int bits, bool aligned, bool y_aligned) {
    G4Plan pl{};
    if (!w4_cut(M, C, K, G, bits, aligned, LSQ_LINGLU_W4_MAX_ROWS, pl.geo, pl.pair)) return pl;
    pl.served = 1;
    pl.block = kQBlock;
    pl.lds = kG4FixedLds + static_cast<int>(M) * pl.geo.row_stride + static_cast<int>(M) * pl.geo.gstride * 4;
    pl.chunks = pl.geo.n_chunks;
    pl.x_resident = pl.chunks == 1 ? 1 : 0;
    pl.grid = mfma_grid(C, device_info().cu_count);
    pl.store = (C % 16 == 0 && y_aligned) ? LSQ_LINGLU_W4_PACKETS : LSQ_LINGLU_W4_BYTES;
    return pl;
}

struct G4Call {             // what every instantiation's launcher takes
    W8Act act;
    G4Pair pr;
    GluArg ga;
    const float* table;
    uint8_t* y;
    int M;
};

template <int BITS, bool PAIR>
static hipError_t g4_launch(const G4Plan& pl, const G4Call& c, hipStream_t stream) {
    static LdsOnce once;
    if (const hipError_t e = allow_lds(once, reinterpret_cast<const void*>(&linglu_w4_kernel<BITS, PAIR>), kG4MaxLds)) return e;
    hipLaunchKernelGGL((linglu_w4_kernel<BITS, PAIR>), dim3(static_cast<unsigned>(pl.grid)), dim3(kQBlock), pl.lds, stream, c.act, c.M,
                       c.pr, pl.geo, c.ga, c.table, pl.store == LSQ_LINGLU_W4_PACKETS ? 1 : 0, c.y);
    return hipGetLastError();
}

static hipError_t g4_launch_format(const G4Plan& pl, int bits, const G4Call& c, hipStream_t stream) {
    if (bits == 2) return g4_launch<2, false>(pl, c, stream);
    return pl.pair ? g4_launch<4, true>(pl, c, stream) : g4_launch<4, false>(pl, c, stream);
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_linglu_w4.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// one projection's checks, said as csrc/lindec_w4/ says them of its weight; `name`: "gate" / "up"
int check_proj(const char* what, const char* name, const lsq_linglu_w4_proj* p, lsq::W4Weight& wt, lsq::W8OutArg& oa) {
    char who[96];
    snprintf(who, sizeof(who), "%s (%s projection)", what, name);
    if (!p) return fail(LSQ_EINVAL, "%s: NULL projection", who);
    int mid = 0;
    if (int rc = check_out(who, p->out, mid, oa)) return rc;
    if (oa.relu) return fail(LSQ_EINVAL, "%s: relu is set: the gated product takes the projection's own levels (not served)", who);
    if (!p->codes || !p->qscale || !p->qzero) return fail(LSQ_EINVAL, "%s: NULL buffer", who);
    const int bias_dtype = static_cast<int>(p->bias_dtype);
    if (p->bias && bias_dtype != LSQ_F32 && bias_dtype != mid)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of mid_dtype, got dtype code %d", who, bias_dtype);
    if (!aligned_to(p->qscale, 4) || !aligned_to(p->qzero, 4) || (p->bias && !aligned_to(p->bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: qscale, qzero and bias must be element-aligned", who);
    wt = lsq::W4Weight{static_cast<const uint8_t*>(p->codes), static_cast<const float*>(p->qscale), static_cast<const int32_t*>(p->qzero),
                       p->bias, bias_dtype};
    return LSQ_OK;
}

// the product's constants, said as csrc/glu_w8/lsq_glu_w8.hip and csrc/linglu_w8/lsq_linglu_w8.hip say them (translation units,
// not headers: a fix there belongs here too); `up_signed`: the up projection's quantizer gives int8 levels
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

// what this library serves; everything else that is legal belongs to lsq_hip_lindec_w4.h / lsq_hip_qlinear_a8.h and lsq_hip_glu_w8.h
int check_served(const char* what, const lsq::G4Plan& pl, int64_t M, int64_t K, int64_t G, int bits, bool aligned) {
    const char* other = "compose the packed levels-out linears with lsq_hip_glu_w8.h";
    if (M > LSQ_LINGLU_W4_MAX_ROWS)
        return fail(LSQ_EINVAL, "%s: M = %lld rows of x, the kernel serves 1 to %d (more rows: %s)", what, static_cast<ll>(M),
                    LSQ_LINGLU_W4_MAX_ROWS, other);
    if (!aligned) return fail(LSQ_EINVAL, "%s: x_levels and both projections' codes must be 16-byte aligned (otherwise: %s)", what, other);
    if (!pl.served)
        return fail(LSQ_EINVAL, "%s: K = %lld, group_size %lld at %d bits: the kernel serves K > 0 and groups of whole 16-byte code "
                    "packets (%d elements) with lcm(group_size, 4 packets) <= %d elements (otherwise: %s)", what, static_cast<ll>(K),
                    static_cast<ll>(G), bits, 128 / bits, lsq::kQChunk, other);
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_linglu_w4_abi_version(void) { return LSQ_LINGLU_W4_ABI_VERSION; }

const char* lsq_linglu_w4_last_error(void) { return g_last_error; }

int lsq_linglu_w4(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, const lsq_linglu_w4_proj* gate,
                  const lsq_linglu_w4_proj* up, int64_t C, int64_t K, int64_t group_size, int bits, const void* table,
                  const lsq_glu_w8_consts* consts, void* y, void* stream) {
    const char* what = "lsq_linglu_w4";
    lsq::G4Call c{};
    if (int rc = check_format(what, M, C, K, group_size, bits)) return rc;
    if (int rc = check_levels_in(what, kCodes, level_dtype, x_levels, s_x, zx)) return rc;
    if (int rc = check_proj(what, "gate", gate, c.pr.gate, c.pr.gate_out)) return rc;
    if (int rc = check_proj(what, "up", up, c.pr.up, c.pr.up_out)) return rc;
    const bool up_signed = std::max(up->out->quant_max, up->out->type_max) <= 127;
    if (int rc = check_consts(what, consts, up_signed, c.ga)) return rc;
    if (!table || !y) return fail(LSQ_EINVAL, "%s: NULL table or y", what);
    if (!aligned_to(table, 4)) return fail(LSQ_EINVAL, "%s: the table's 256 float32 values must be 4-byte aligned", what);
    if (overlap(y, M * C, table, 1024)) return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap the table's 1024", what, static_cast<ll>(M * C));
    const bool aligned = aligned_to(x_levels, 16) && aligned_to(gate->codes, 16) && aligned_to(up->codes, 16);
    const lsq::G4Plan pl = lsq::plan_linglu_w4(M, C, K, group_size, bits, aligned, aligned_to(y, 16));
    if (int rc = check_served(what, pl, M, K, group_size, bits, aligned)) return rc;
    if (C == 0) return LSQ_OK;
    c.act = levels_act(level_dtype, x_levels, s_x, zx);
    c.table = static_cast<const float*>(table);
    c.y = static_cast<uint8_t*>(y);
    c.M = static_cast<int>(M);
    return hip_status(lsq::g4_launch_format(pl, bits, c, static_cast<hipStream_t>(stream)), what);
}

int lsq_linglu_w4_plan(int64_t M, int64_t C, int64_t K, int64_t group_size, int bits, int aligned, int y_aligned, int32_t* out8) {
    const char* what = "lsq_linglu_w4_plan";
    if (int rc = check_format(what, M, C, K, group_size, bits)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::G4Plan pl = lsq::plan_linglu_w4(M, C, K, group_size, bits, aligned != 0, y_aligned != 0);
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
