// lsq_linrope_w4.hip -- the qkv projection of an attention block's decode step (M <= 16) on packed 4- / 2-bit codes with the rotary
// embedding and the KV-cache append in its epilogue on gfx950 (include/lsq_hip_linrope_w4.h, which states the contract and what is
// served): the kernel and the C ABI of liblsq_hip_linrope_w4.so.
//
// Nothing is defined here.  For each strip v is csrc/lindec_w4/'s: the same exact integer I per group, one conversion,
// acc + qscale * f, the same assignment of spans to waves, the same order of the sum over the waves, * s_x, + bias.  The qkv byte is
// csrc/lindec_w4/lsq_lindec_w4_shared.hpp's w4q_byte, the rotation csrc/linrope_w8/lsq_linrope_shared.hpp's rope_dequant and
// rope_pair on two of those bytes, its level csrc/lsq_w8_out_side.hpp's w8o_byte: the same device functions, compiled into this
// library.
//
// ONE KERNEL TEXT, linrope_w4_kernel<BITS, PAIR>, 1024 threads = 16 waves: csrc/linglu_w4/'s K loop on csrc/linrope_w8/'s items.
//  * ITEMS (lr_item).  Two 16-row strips of the ONE code tensor: ROTATE the features f0 .. f0 + 15 (f0 < R / 2) and f0 + R / 2 .. of a
//    q or k head, PASS two adjacent strips beyond R, COPY two adjacent strips of a v head.  D % 32 == 0 and R % 32 == 0: the
//    (H + 2 Hkv) D / 32 items tile the rows exactly, no row is clamped.  A persistent grid of min(items, CUs) workgroups.
//  * PLACEMENT (lr_place_row).  Before the first item 16 threads compute per row the position, three write flags and three
//    destination offsets -- dense from strides, paged from ONE block-table read -- into 512 bytes of LDS.  From there dense and paged
//    are one text.
//  * K LOOP.  Both strips have one format and one K, so ONE cursor walks both.  A lane holds ONE byte offset (row nA + n, packet q)
//    and ONE group index; strip B differs by a wave-uniform row offset into `codes`, `qscale` and `qzero`.  TWO pair steps of
//    non-temporal 16-byte packets are in flight per wave; a pair step is reissued behind its MFMAs; a chunk's first two are issued
//    before the staging barrier and the NEXT ITEM's first two before this item's epilogue.  A group's constants of both strips are
//    fetched once, with the step that holds the group's last packet, by lane (n, q) for the group that ends at place q, and handed
//    over with ds_bpermute_b32 (w4_from_place).  x and the sum a - G z table are staged once per chunk for both strips
//    (w4_stage_chunk) and stay in LDS across items when one chunk holds K.  Per place ONE ds_read of the x operand feeds four
//    v_mfma_i32_16x16x64_i8: P_a, C_a (the all-ones A operand), P_b, C_b.  When a group ends, I = P - z C - qzero (sum a - G z) is
//    formed PER STRIP, in 32 bits if every |qzero| of the wave's columns in THAT strip is at most 256, else in 64.
//  * ORDER OF THE SUM.  Each strip has its own fp32 accumulator and its own 16 KB region of partial sums.  The shared cursor visits
//    the groups of the wave's spans in ascending order, chunk after chunk, exactly as lindec_w4's does; at every group end each
//    strip's accumulator takes that strip's one rounded product and one rounded add.  The epilogue adds each region in wave order.
//  * COS / SIN.  Thread (m, col) of the 256 that rotate issues its two table loads BEFORE the K loop of a ROTATE item.
//  * EPILOGUE.  Threads 0..255 add strip A in wave order and form its qkv byte into a [16][16] tile, threads 256..511 strip B (whole
//    waves on either side of the select).  After a barrier thread (m, col) forms the two output bytes (rotated, passed or copied)
//    into two output tiles.  After a barrier lane m < M of wave 0 stores row m of strip A as ONE 16-byte packet at its destination,
//    wave 1 strip B.  Rows whose flag is off, and rows >= M, are written neither to the output tiles nor to memory.
//  * BARRIERS.  One behind the placement, then three per item (sums written, bytes written, levels written) besides the staging's.
//    None behind the stores: a region is rewritten only behind a later barrier than the one its readers have passed -- the sums
//    behind the next item's K loop, so behind "levels written" (they are read before "bytes written"); the two qkv byte tiles behind
//    the next "sums written" (read before "levels written"); the two output tiles behind the next "bytes written" (the stores that
//    read them stand before the next "sums written").  x and the group sums are rewritten (more than one chunk) behind the
//    staging's own first barrier, which every wave reaches after its last MFMA of the previous chunk.  The placement is written
//    once, behind no reader, and only read afterwards.
//  * REGISTERS.  1024 threads leave 128 VGPRs.  The wave index is read with v_readfirstlane_b32, so both cursors are scalars.  No
//    instantiation has scratch (profiles/r40_linrope_w4_isa.txt).
// LDS: 32 KB of partial sums, 1 KB of tiles, 512 bytes of placement, M rows of x of at most 4096 + 16 bytes, M * groups-per-chunk
// int32: at most 106.5 KB, behind lsq_qdecode.hpp's opt-in.
#include "../lindec_w4/lsq_lindec_w4_shared.hpp"
#include "../linrope_w8/lsq_linrope_shared.hpp"
#include "../../../include/lsq_hip_linrope_w4.h"

static_assert(LSQ_LINROPE_W4_MAX_ROWS == 16 && LSQ_LINROPE_W8_MAX_ROWS == 16, "the rows of x are the 16 rows of one MFMA tile");
static_assert(LSQ_A8_U8 == LSQ_REQUANT_W8_U8 && LSQ_A8_I8 == LSQ_REQUANT_W8_I8, "one pair of level codes");
static_assert(LSQ_ROPE_W8_U8 == LSQ_REQUANT_W8_U8 && LSQ_ROPE_W8_I8 == LSQ_REQUANT_W8_I8, "one level type code for the two steps");

namespace lsq {

constexpr int kR4RedFloats = kQRedBytes / 4;        // fp32 values of one strip's partial sums
constexpr int kR4FixedLds = 2 * kQRedBytes + 4 * kW4TileBytes + kLrPlaceBytes;
constexpr int kR4MaxLds = kR4FixedLds + LSQ_LINROPE_W4_MAX_ROWS * (kQChunk + kQRowPad) + LSQ_LINROPE_W4_MAX_ROWS * (kQChunk / 32) * 4;
static_assert(kR4FixedLds % 16 == 0, "the rows of x are read and written as 16-byte packets");
static_assert(kR4MaxLds <= 160 * 1024, "the LDS of one CDNA4 compute unit");

template <int BITS, bool PAIR>
__global__ __launch_bounds__(kQBlock) void linrope_w4_kernel(W8Act act, int M, W4Weight wt, W8OutArg qkv_out, W4Geom geo, LrGeom g, RopeArg ra,
                                                            const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                            const int32_t* __restrict__ pos, const int32_t* __restrict__ bt, LrDst dst) {
    constexpr int D = 32 / BITS;                    // elements per dword
    constexpr int BE = 4 * D;                       // elements per 16-byte packet
    constexpr int PER = PAIR ? 2 : 1;               // packets per MFMA
    constexpr int NS = 4 / PER;                     // MFMAs of one strip, and so places where a group can end, per step
    static_assert(!PAIR || BITS == 4, "two packets per MFMA only at 4 bits: a 2-bit packet is 64 elements already");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);            // [strip A, B][wave][lane][register]
    unsigned char* tiles = smem + 2 * kQRedBytes;           // [qkv A, qkv B, out A, out B][16][16]
    const LrPlace place = lr_place_at(tiles + 4 * kW4TileBytes);
    unsigned char* xs = smem + kR4FixedLds;
    int32_t* aeff = reinterpret_cast<int32_t*>(xs + M * geo.row_stride);       // [M][gstride]: sum a - G z

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // said to the compiler: the cursors below are scalars
    const int nl = lane & 15, q = lane >> 4;
    const W8Const ac = w8_constants(act);
    const int n_chunks = geo.n_chunks, chunk_p = geo.chunk_spans * geo.span_p;
    const int first_item = static_cast<int>(blockIdx.x);
    const int span_jump = (kQWaves - 1) * geo.span_p, group_jump = (kQWaves - 1) * geo.groups_per_span;
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};

    // the rows the lane's load steps read: this item's, from the prefetch before the epilogue on the next item's.  lane_byte: packet q
    // of row nA + n; strip B lies a wave-uniform number of rows further in `codes`, `qscale` and `qzero`
    int64_t lane_byte = 0, row_group = 0, b_byte = 0, b_group = 0;
    auto rows_of = [&](const LrItem& it) {
        lane_byte = (it.nA + nl) * (geo.n_packets * 16) + q * 16;
        row_group = (it.nA + nl) * geo.n_groups;
        b_byte = (it.nB - it.nA) * (geo.n_packets * 16);
        b_group = (it.nB - it.nA) * geo.n_groups;
    };

    // the pair step the cursor points at, and the cursor one step further.  c: the chunk; np: its packets
    auto load_step = [&](W4Step& sa, W4Step& sb, W4Cursor& cur, int c, int np) {
        sa.p = sb.p = cur.p < np ? cur.p : -1;
        sa.raw = sb.raw = u32x4{0u, 0u, 0u, 0u};
        sa.qs = sb.qs = 0.0f;
        sa.qz = sb.qz = 0;
        if (sa.p >= 0) {
            if (sa.p + q < np) {
                const uint8_t* at = wt.codes + lane_byte + static_cast<uint32_t>(c * chunk_p + sa.p) * 16u;     // a row is at most 2^29 bytes
                sa.raw = load_code_packet(at, 0);
                sb.raw = load_code_packet(at + b_byte, 0);
            }
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                if (sa.p + j * PER >= np) continue;
                cur.pig += PER;
                if (cur.pig == geo.ppg) {                   // the group's last packet is in this step: both strips' constants, once
                    const int64_t gi = row_group + (c * geo.chunk_groups + cur.g);      // a row has at most 2^25 groups
                    if (q == j) {
                        sa.qs = wt.qscale[gi];
                        sa.qz = wt.qzero[gi];
                        sb.qs = wt.qscale[gi + b_group];
                        sb.qz = wt.qzero[gi + b_group];
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

    W4Step a0, b0, a1, b1;
    W4Cursor ld = {0, 0, 0, 0};
    auto prime = [&](int c) {                               // a chunk's first two pair steps
        ld = W4Cursor{wave * geo.span_p, 0, 0, wave * geo.groups_per_span};
        const int np = packets_of(c);
        load_step(a0, b0, ld, c, np);
        load_step(a1, b1, ld, c, np);
    };

    if (first_item < g.items) {
        rows_of(lr_item(g, first_item));
        prime(0);
    }
    // where the rows go, once per workgroup
    if (tid < 16) lr_place_row(g, M, pos, bt, place, tid);
    __syncthreads();                                        // placement written

    for (int item = first_item; item < g.items; item += static_cast<int>(gridDim.x)) {
        const LrItem it = lr_item(g, item);

        float cs = 0.0f, sn = 0.0f;                         // in flight during the K loop
        if (it.rot && tid < kW4TileBytes && (tid >> 4) < M && (place.flags[tid >> 4] & it.bit)) {
            const int64_t col = static_cast<int64_t>(place.p[tid >> 4]) * (g.R / 2) + it.fA + (tid & 15);
            cs = cos_t[col];
            sn = sin_t[col];
        }

        f32x4 acca = {0.0f, 0.0f, 0.0f, 0.0f}, accb = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = 0; c < n_chunks; ++c) {
            const int np = packets_of(c);
            if (c > 0) prime(c);                            // (chunk 0: before the loop or before the previous item's epilogue)
            if (n_chunks > 1 || item == first_item) {       // x and the group sums stay in LDS across items when one chunk holds K
                __syncthreads();
                w4_stage_chunk<BITS>(act, ac, M, geo, static_cast<int64_t>(c) * geo.chunk_k, np, xs, aeff, tid);
            }

            // the wave's steps of this chunk: spans wave, wave + 16, ...
            i32x4 Pa = {0, 0, 0, 0}, Pb = {0, 0, 0, 0}, Ca = {0, 0, 0, 0}, Cb = {0, 0, 0, 0};
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
            auto compute_step = [&](const W4Step& sa, const W4Step& sb) {
                uint32_t rA[4] = {sa.raw.x, sa.raw.y, sa.raw.z, sa.raw.w};
                uint32_t rB[4] = {sb.raw.x, sb.raw.y, sb.raw.z, sb.raw.w};
                transpose_over_rows(rA);
                transpose_over_rows(rB);
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const int t = j * PER;
                    if (sa.p + t >= np) continue;           // the same for the whole wave
                    const unsigned char* xa = xrow + (sa.p + t) * BE;      // this packet's first element in the chunk
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
                    const i32x4 ba = codes_of(rA, t);
                    Pa = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, ba, Pa, 0, 0, 0);
                    Ca = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, ba, Ca, 0, 0, 0);
                    const i32x4 bb = codes_of(rB, t);
                    Pb = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bb, Pb, 0, 0, 0);
                    Cb = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bb, Cb, 0, 0, 0);
                    pig += PER;
                    if (pig == geo.ppg) {                   // the group is complete in both strips: the same for the whole wave
                        int ae[4];                          // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
                        for (int i = 0; i < 4; ++i) ae[i] = q * 4 + i < M ? aeff[(q * 4 + i) * geo.gstride + g_local] : 0;
                        end_group(sa, j, ae, Pa, Ca, acca);
                        end_group(sb, j, ae, Pb, Cb, accb);
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
            while (a0.p >= 0) {                             // the same for the whole wave; a pair step is reissued behind its MFMAs
                compute_step(a0, b0);
                load_step(a0, b0, ld, c, np);
                if (a1.p < 0) break;
                compute_step(a1, b1);
                load_step(a1, b1, ld, c, np);
            }
        }
        // the next item's first steps, in flight across this item's epilogue
        const int next_item = item + static_cast<int>(gridDim.x);
        if (next_item < g.items) {
            rows_of(lr_item(g, next_item));
            prime(0);
        }

        // the waves' tiles of either strip, each summed in wave order
        *reinterpret_cast<f32x4*>(red + (wave * 64 + lane) * 4) = acca;
        *reinterpret_cast<f32x4*>(red + kR4RedFloats + (wave * 64 + lane) * 4) = accb;
        __syncthreads();                                    // sums written
        if (tid < 512) {                                    // one thread per qkv output of either strip: whole waves take a side
            const int side = tid >> 8;                      // 0: strip A, 1: strip B
            const int l = tid & 63, reg = (tid >> 6) & 3;
            const int col = l & 15, m = (l >> 4) * 4 + reg;
            if (m < M) {
                const int64_t n = (side ? it.nB : it.nA) + col;
                const float* rs = red + side * kR4RedFloats;
                float sum = 0.0f;
#pragma unroll
                for (int w = 0; w < kQWaves; ++w) sum = __fadd_rn(sum, rs[(w * 64 + l) * 4 + reg]);
                const float bias = wt.bias ? w8_bias_at(wt.bias, wt.bias_dtype, n) : 0.0f;
                const float v = __fadd_rn(__fmul_rn(sum, ac.s_x), bias);
                tiles[side * kW4TileBytes + m * kQTile + col] = w4q_byte(v, w8q_constants(qkv_out));
            }
        }
        __syncthreads();                                    // bytes written
        if (tid < kW4TileBytes) {                           // thread (m, col): consecutive lanes on consecutive columns
            const int m = tid >> 4;
            if (m < M && (place.flags[m] & it.bit)) {
                const uint32_t la = tiles[tid], lb = tiles[kW4TileBytes + tid];
                uint32_t oa = la, ob = lb;                  // COPY: y byte = x byte
                if (it.kind < 2) {
                    const RopeQ rq = rope_constants(ra, g.flip);
                    const float da = rope_dequant<0>(la ^ g.flip, rq), db = rope_dequant<0>(lb ^ g.flip, rq);
                    float ua = da, ub = db;                 // PASS: u = d(l)
                    if (it.rot) rope_pair(da, db, cs, sn, rq.mid, ua, ub);
                    oa = w8o_byte(ua, rq);
                    ob = w8o_byte(ub, rq);
                }
                tiles[2 * kW4TileBytes + tid] = static_cast<unsigned char>(oa);
                tiles[3 * kW4TileBytes + tid] = static_cast<unsigned char>(ob);
            }
        }
        __syncthreads();                                    // levels written
        if (wave < 2 && lane < M && (place.flags[lane] & it.bit)) {     // wave 0: strip A, wave 1: strip B; one 16-byte packet per row
            uint8_t* at = dst.p[it.kind] + place.off[it.kind * 16 + lane] + it.hh * g.head_s[it.kind] + (wave ? it.fB : it.fA);
            *reinterpret_cast<u32x4*>(at) = *reinterpret_cast<const u32x4*>(tiles + (2 + wave) * kW4TileBytes + lane * kQTile);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launcher
// ------------------------------------------------------------------------------------------------
struct R4Plan {
    int served, block, lds, chunks, x_resident, rotate, pass, copy;
    bool pair;
    int64_t grid;
    W4Geom geo;
};

// the cut of K is csrc/lindec_w4/'s (w4_cut): the order of either strip's sum is fixed by it
inline R4Plan plan_linrope_w4(const lsq_linrope_w8_geom& ge, int64_t K, int64_t G, int bits, bool aligned) {
    R4Plan pl{};
    const int64_t M = ge.B * ge.T, N = (ge.H + 2 * ge.Hkv) * ge.D;
    if (!lr_geom_served(ge) || !w4_cut(M, N, K, G, bits, aligned, LSQ_LINROPE_W4_MAX_ROWS, pl.geo, pl.pair)) return pl;
    pl.served = 1;
    pl.block = kQBlock;
    pl.lds = kR4FixedLds + static_cast<int>(M) * pl.geo.row_stride + static_cast<int>(M) * pl.geo.gstride * 4;
    pl.chunks = pl.geo.n_chunks;
    pl.x_resident = pl.chunks == 1 ? 1 : 0;
    lr_item_counts(ge, pl.rotate, pl.pass, pl.copy);
    pl.grid = std::min<int64_t>(pl.rotate + pl.pass + pl.copy, device_info().cu_count);
    return pl;
}

struct R4Call {             // what every instantiation's launcher takes
    W8Act act;
    W4Weight wt;
    W8OutArg qo;
    LrGeom g;
    RopeArg ra;
    const float *cos_t, *sin_t;
    const int32_t *pos, *bt;
    LrDst dst;
    int M;
};

template <int BITS, bool PAIR>
static hipError_t r4_launch(const R4Plan& pl, const R4Call& c, hipStream_t stream) {
    static LdsOnce once;
    if (const hipError_t e = allow_lds(once, reinterpret_cast<const void*>(&linrope_w4_kernel<BITS, PAIR>), kR4MaxLds)) return e;
    hipLaunchKernelGGL((linrope_w4_kernel<BITS, PAIR>), dim3(static_cast<unsigned>(pl.grid)), dim3(kQBlock), pl.lds, stream, c.act, c.M,
                       c.wt, c.qo, pl.geo, c.g, c.ra, c.cos_t, c.sin_t, c.pos, c.bt, c.dst);
    return hipGetLastError();
}

static hipError_t r4_launch_format(const R4Plan& pl, int bits, const R4Call& c, hipStream_t stream) {
    if (bits == 2) return r4_launch<2, false>(pl, c, stream);
    return pl.pair ? r4_launch<4, true>(pl, c, stream) : r4_launch<4, false>(pl, c, stream);
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_linrope_w4.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// the projection's checks, said as csrc/linglu_w4/lsq_linglu_w4.hip says them of either of its two (a translation unit, not a
// header: a fix there belongs here too)
int check_proj(const char* what, const lsq_linrope_w4_proj* p, int& mid, lsq::W4Weight& wt, lsq::W8OutArg& oa) {
    if (!p) return fail(LSQ_EINVAL, "%s: NULL projection", what);
    if (int rc = check_out(what, p->out, mid, oa)) return rc;
    if (oa.relu) return fail(LSQ_EINVAL, "%s: relu is set: the rotation takes the projection's own levels (not served)", what);
    if (!p->codes || !p->qscale || !p->qzero) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    const int bias_dtype = static_cast<int>(p->bias_dtype);
    if (p->bias && bias_dtype != LSQ_F32 && bias_dtype != mid)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of mid_dtype, got dtype code %d", what, bias_dtype);
    if (!aligned_to(p->qscale, 4) || !aligned_to(p->qzero, 4) || (p->bias && !aligned_to(p->bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: qscale, qzero and bias must be element-aligned", what);
    wt = lsq::W4Weight{static_cast<const uint8_t*>(p->codes), static_cast<const float*>(p->qscale), static_cast<const int32_t*>(p->qzero),
                       p->bias, bias_dtype};
    return LSQ_OK;
}

// what this library serves; everything else that is legal belongs to lsq_hip_lindec_w4.h, lsq_hip_rope_w8.h and lsq_hip_attn_paged_w8.h
int check_served(const char* what, const lsq::R4Plan& pl, const lsq_linrope_w8_geom& g, int64_t K, int64_t G, int bits, bool aligned,
                 const Dest (&d)[3]) {
    const char* other = "the composition of lsq_hip_lindec_w4.h, lsq_hip_rope_w8.h and lsq_hip_attn_paged_w8.h serves it";
    if (int rc = check_rows_served(what, g, other)) return rc;
    if (int rc = check_geom_served(what, g, d, other)) return rc;
    if (g.R < 32) return fail(LSQ_EINVAL, "%s: R = %lld, the kernel serves 32 <= R (%s)", what, static_cast<ll>(g.R), other);
    if (!aligned) return fail(LSQ_EINVAL, "%s: x_levels, codes, cos, sin, rq, k and v must be 16-byte aligned (%s)", what, other);
    if (!pl.served)
        return fail(LSQ_EINVAL, "%s: K = %lld, group_size %lld at %d bits: the kernel serves K > 0 and groups of whole 16-byte code "
                    "packets (%d elements) with lcm(group_size, 4 packets) <= %d elements (%s)", what, static_cast<ll>(K),
                    static_cast<ll>(G), bits, 128 / bits, lsq::kQChunk, other);
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_linrope_w4_abi_version(void) { return LSQ_LINROPE_W4_ABI_VERSION; }

const char* lsq_linrope_w4_last_error(void) { return g_last_error; }

int lsq_linrope_w4(int level_dtype, const void* x_levels, const void* s_x, const void* zx, const lsq_linrope_w4_proj* proj, int64_t N,
                   int64_t K, int64_t group_size, int bits, const lsq_linrope_w8_geom* geom, const lsq_rope_w8_in* qkv,
                   const lsq_rope_w8_out* rot, const void* cos, const void* sin, const void* positions, const void* block_table, void* rq,
                   void* k, void* v, void* stream) {
    const char* what = "lsq_linrope_w4";
    Dest d[3];
    lsq::R4Call c{};
    if (int rc = check_geom(what, geom, d)) return rc;
    const int64_t M = geom->B * geom->T;
    if (int rc = check_format(what, M, N, K, group_size, bits)) return rc;
    if (N != (geom->H + 2 * geom->Hkv) * geom->D)
        return fail(LSQ_EINVAL, "%s: the weight has N = %lld rows, (H + 2 Hkv) D = %lld are needed", what, static_cast<ll>(N),
                    static_cast<ll>((geom->H + 2 * geom->Hkv) * geom->D));
    if (int rc = check_levels_in(what, kCodes, level_dtype, x_levels, s_x, zx)) return rc;
    int mid = 0;
    if (int rc = check_proj(what, proj, mid, c.wt, c.qo)) return rc;
    if (!rq || !k || !v) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (int rc = check_rotation(what, geom, mid, qkv, rot, cos, sin, positions, block_table, c.ra)) return rc;
    void* const dp[3] = {rq, k, v};
    if (int rc = check_dest_overlap(what, geom, d, dp, x_levels, M * K, proj->codes, N * (K * bits / 8), cos, sin, positions, block_table))
        return rc;
    const bool aligned = aligned_to(x_levels, 16) && aligned_to(proj->codes, 16) && aligned_to(cos, 16) && aligned_to(sin, 16) &&
                         aligned_to(rq, 16) && aligned_to(k, 16) && aligned_to(v, 16);
    const lsq::R4Plan pl = lsq::plan_linrope_w4(*geom, K, group_size, bits, aligned);
    if (int rc = check_served(what, pl, *geom, K, group_size, bits, aligned, d)) return rc;
    const bool qkv_signed = std::max(proj->out->quant_max, proj->out->type_max) <= 127;
    c.act = levels_act(level_dtype, x_levels, s_x, zx);
    c.g = kernel_geom(geom, d, pl.rotate + pl.pass + pl.copy, qkv_signed);
    c.cos_t = static_cast<const float*>(cos);
    c.sin_t = static_cast<const float*>(sin);
    c.pos = static_cast<const int32_t*>(positions);
    c.bt = static_cast<const int32_t*>(block_table);
    c.dst = lsq::LrDst{{static_cast<uint8_t*>(rq), static_cast<uint8_t*>(k), static_cast<uint8_t*>(v)}};
    c.M = static_cast<int>(M);
    return hip_status(lsq::r4_launch_format(pl, bits, c, static_cast<hipStream_t>(stream)), what);
}

int lsq_linrope_w4_plan(const lsq_linrope_w8_geom* geom, int64_t K, int64_t group_size, int bits, int aligned, int32_t* out9) {
    const char* what = "lsq_linrope_w4_plan";
    Dest d[3];
    if (int rc = check_geom(what, geom, d)) return rc;
    if (int rc = check_format(what, geom->B * geom->T, (geom->H + 2 * geom->Hkv) * geom->D, K, group_size, bits)) return rc;
    if (!out9) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::R4Plan pl = lsq::plan_linrope_w4(*geom, K, group_size, bits, aligned != 0);
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
