// lsq_linmid_w4.hip -- the W4A8 / W2A8 linears with an 8-bit output for 17 to 64 rows on gfx950 (include/lsq_hip_linmid_w4.h,
// which states the contract and what is served): the kernel and the C ABI of liblsq_hip_linmid_w4.so.
//
// Nothing is defined here.  v is csrc/lindec_w4/lsq_lindec_w4.hip's: the same exact integer I per group, one conversion,
// acc + qscale * f, the same assignment of spans to wave slots, the same order of the sum over the slots, * s_x, + bias; the byte is
// lsq_lindec_w4_shared.hpp's w4q_byte / w4r_byte.  What is new is how much of x a workgroup holds against one pass over the weight.
//
// ONE KERNEL TEXT, linmid_w4_kernel<BITS, PAIR, RES, SUBS>, 512 threads = 8 waves, each owning wave slots w and w + 8 of the 16 of
// the contract with separate cursors, products and accumulators (MidSlot), a persistent grid of min(ceil(N / 16), CUs) workgroups on tiles of 16 output columns; lane (n = lane & 15, q = lane >> 4) reads row
// tile * 16 + n of the weight.  SUBS = ceil(M / 16) in {2, 3, 4} sub-tiles of 16 rows of x.
//  * WORK SPLIT.  lindec_w4's: slot w takes spans w, w + 16, ... of each chunk of 4096 k, its groups ascending, one fp32 x 4
//    accumulator PER SUB-TILE carried across the chunks.  So the order of row m's sum is lindec_w4's, whatever M is.
//  * WEIGHT STREAM.  lindec_w4's load step (4 packets of 16 bytes of each of the 16 rows, non-temporal; a group's qscale / qzero
//    once, by the lane of the place where the group ends).  TWO steps are in flight per slot, four per wave.  A chunk's first two are issued before x is staged and the NEXT
//    TILE's first two before this tile's epilogue.
//  * OPERANDS.  One B fragment (the codes of one place as unsigned nibbles / crumbs after the 4 x 4 lane transpose) feeds SUBS
//    v_mfma_i32_16x16x64_i8 on the sub-tiles' rows of x and ONE all-ones MFMA for sum c, which does not depend on the row.
//  * X IN WINDOWS.  64 rows of a chunk do not fit in LDS.  A PLACE is one MFMA's k (PER packets); a slot's places of a chunk are
//    numbered along its steps.  A WINDOW holds places [g0, g0 + wpl) of ALL 16 slots for the M rows, xs[row][slot][place][bytes],
//    each block of 16 bytes in w4_lds_pos's order: every slot meets its spans and groups in ascending order, whatever wpl is.  wpl
//    is a whole number of steps, or 1 or 2 places of one step when not even a step of every slot fits (the step's registers then
//    stay across the windows).  The host picks the largest wpl that fits 160 KB.  sum a - G z per (row, group of the chunk) is
//    set to -G z at a chunk's first window and gains each window's staged bytes, by one thread per (row, slot): a slot's groups
//    are its own.  When one window holds all of K, x and the sums stay in LDS across the workgroup's tiles.
//  * EPILOGUE.  In SUBS passes over one 16 KB buffer: the slots' fp32 tiles of one sub-tile meet in LDS, thread tid < 256 sums one
//    output in slot order, forms the byte and writes it into the [64][16] byte tile.  Then lane m < M of wave 0 stores row m as ONE
//    16-byte packet (N % 16 == 0 and y 16-byte aligned), else the tile goes out byte by byte along n.
//  * RESIDUAL (RES).  lindec_w4's scheme: lane m < M of wave 0 parks row m's 16 residual bytes in the byte tile at the top of the
//    tile; without packets the tile is filled byte by byte after the K loop.
//  * REGISTERS.  1024 threads leave 128 VGPRs, and SUBS accumulators plus SUBS product tiles do not fit there (11 to 69 spilled
//    registers in a 16-wave form): hence 8 waves with 256.  The table of sum a - G z is laid out [group][row] over whole sub-tiles
//    of rows, so a lane reads the four rows of its D registers as ONE 16-byte packet from one address per sub-tile (sixteen
//    addresses per slot spilled otherwise).  185 to 246 are used; no instantiation has scratch (profiles/r41_linmid_w4_isa.txt).
//  Rows >= M and columns >= N are never written, neither to the byte tile nor to memory (the table's rows >= M stay at -G z).
// LDS: 16 KB of partial sums, 1 KB of byte tile, M rows of x of 16 * wpl places + 16 bytes, 16 SUBS * groups-per-chunk int32: at most
// 160 KB.
//
// (load_step and the compute cursor are lindec_w4's text: they capture that kernel's locals, and moving them would change the
// three libraries that must keep their code.  A fix there belongs here too.)
#include "../lindec_w4/lsq_lindec_w4_shared.hpp"
#include "../../../include/lsq_hip_linmid_w4.h"

static_assert(LSQ_LINMID_W4_MAX_ROWS == 64 && LSQ_LINMID_W4_MIN_ROWS == 17, "2 to 4 sub-tiles of the 16 rows of one MFMA tile");
static_assert(LSQ_A8_U8 == LSQ_REQUANT_W8_U8 && LSQ_A8_I8 == LSQ_REQUANT_W8_I8, "one pair of level codes");

namespace lsq {

constexpr int kMidWaves = 8;                        // waves of a workgroup: each owns wave slots w and w + 8 of the 16
constexpr int kMidBlock = kMidWaves * 64;
constexpr int kMidMaxLds = 160 * 1024;
constexpr int kMidTileBytes = LSQ_LINMID_W4_MAX_ROWS * kQTile;     // one [64][16] byte tile
constexpr int kMidFixedLds = kQRedBytes + kMidTileBytes;

struct MidWin {             // kernel argument: the windows of x (host: plan_linmid_w4)
    int wpl;                // places of one wave slot per window
    int row_stride;         // bytes between rows of x in LDS: 16 slots * wpl places + kQRowPad
    int resident;           // one window holds all of K
};

// the first element, counted from the chunk's first, of place gp of wave slot w: step gp / NS of the slot, place gp % NS of the step
template <int BE, int PER, int NS>
__device__ __forceinline__ int mid_place_elem(const W4Geom& geo, int w, int gp) {
    const int t = gp / NS, j = gp - t * NS;
    const int round = t / geo.steps_per_span, l = t - round * geo.steps_per_span;
    return ((w + kQWaves * round) * geo.span_p + l * 4 + j * PER) * BE;
}

// One window of x into LDS, by the whole workgroup (the caller's barrier precedes): places [g0, g0 + win.wpl) of every slot, ^ flip,
// each block of 16 bytes in w4_lds_pos's order; then the window's part of sum a - G z.  Ends with a barrier.
template <int BITS, bool PAIR>
__device__ __forceinline__ void mid_stage_window(const W8Act& act, const W8Const& ac, int M, const W4Geom& geo, const MidWin& win,
                                                 int64_t kc0, int np, int g0, unsigned char* xs, int32_t* aeff, int ms, int tid) {
    constexpr int BE = 128 / BITS, PER = PAIR ? 2 : 1, NS = 4 / PER, PB = PER * BE, BP = PB / 16;
    const int held = np * BE;                       // elements of this chunk
    const int per_row = kQWaves * win.wpl * BP;     // blocks of 16 bytes of one row
    for (int it = tid; it < M * per_row; it += kMidBlock) {
        const int m = it / per_row, rem = it - m * per_row;
        const int sp = rem / BP, blk = rem - sp * BP;           // sp: slot * wpl + place of the window
        const int w = sp / win.wpl, pi = sp - w * win.wpl;
        const int e = mid_place_elem<BE, PER, NS>(geo, w, g0 + pi);
        if (e >= held) continue;                    // past the chunk: no MFMA reads it
        const u32x4 v = *reinterpret_cast<const u32x4*>(act.a + static_cast<int64_t>(m) * geo.K + kc0 + e + blk * 16) ^ ac.flip;
        *reinterpret_cast<u32x4*>(xs + m * win.row_stride + sp * PB + blk * 16) = w4_deinterleave<BITS>(v);
    }
    if (g0 == 0)
        for (int it = tid; it < ms * geo.gstride; it += kMidBlock) aeff[it] = -geo.G * ac.z;
    __syncthreads();
    for (int it = tid; it < M * kQWaves; it += kMidBlock) {       // a slot's groups are touched by this thread alone
        const int m = it >> 4, w = it & 15;
        for (int pi = 0; pi < win.wpl; ++pi) {
            const int e = mid_place_elem<BE, PER, NS>(geo, w, g0 + pi);
            if (e >= held) continue;
            const unsigned char* src = xs + m * win.row_stride + (w * win.wpl + pi) * PB;
            int sum = 0;
#pragma unroll
            for (int b = 0; b < PB; b += 16) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(src + b);
                sum += w8_sum_bytes(v.x) + w8_sum_bytes(v.y) + w8_sum_bytes(v.z) + w8_sum_bytes(v.w);
            }
            aeff[(e / geo.G) * ms + m] += sum;                  // a place lies in one group
        }
    }
    __syncthreads();
}

template <int SUBS>
struct MidSlot {            // what a wave keeps per wave slot it owns
    W4Step s0, s1;          // the slot's even and odd steps of the chunk, in flight
    W4Cursor ld;            // the load side's cursor
    i32x4 P[SUBS], C;       // the current group's products per sub-tile, and sum c
    f32x4 acc[SUBS];
    int pig, g_local, sl;   // the compute side's cursor: as ld's, two steps behind
};

template <int BITS, bool PAIR, bool RES, int SUBS>
__global__ __launch_bounds__(kMidBlock) void linmid_w4_kernel(W8Act act, int M, W4Weight wt, W4Geom geo, MidWin win, W8OutArg out,
                                                             W8ResArg res, W8PreArg pre, uint8_t* __restrict__ y) {
    constexpr int D = 32 / BITS;                    // elements per dword
    constexpr int BE = 4 * D;                       // elements per 16-byte packet
    constexpr int PER = PAIR ? 2 : 1;               // packets per MFMA
    constexpr int NS = 4 / PER;                     // MFMAs, and so places where a group can end, per step
    constexpr int PB = PER * BE;                    // bytes of x per place and row
    static_assert(!PAIR || BITS == 4, "two packets per MFMA only at 4 bits: a 2-bit packet is 64 elements already");
    static_assert(SUBS >= 2 && SUBS <= 4, "17 to 64 rows");
    typedef W4Step Step;
    typedef MidSlot<SUBS> Slot;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);            // [slot][lane][register], one sub-tile at a time
    unsigned char* tileb = smem + kQRedBytes;               // [64][16]
    unsigned char* xs = tileb + kMidTileBytes;
    constexpr int MS = SUBS * 16;                   // rows of the table of sum a - G z: whole sub-tiles, so a lane reads its four rows as one packet
    int32_t* aeff = reinterpret_cast<int32_t*>(xs + M * win.row_stride);       // [gstride][MS]: sum a - G z; rows >= M stay at -G z

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
        if (++cur.l == geo.steps_per_span) {                // the slot's next span: 16 spans on; a span starts a group and ends one
            cur.l = 0;
            cur.p += span_jump;
            cur.g += group_jump;
        }
    };

    // packets of chunk c
    auto packets_of = [&](int c) { return static_cast<int>(std::min<int64_t>(chunk_p, geo.n_packets - static_cast<int64_t>(c) * chunk_p)); };

    Slot st[2];                                             // wave slots wave and wave + 8
    auto prime = [&](int c) {                               // a chunk's first two steps of both slots
        const int np = packets_of(c);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int slot = wave + kMidWaves * h;
            st[h].ld = W4Cursor{slot * geo.span_p, 0, 0, slot * geo.groups_per_span};
            load_step(st[h].s0, st[h].ld, c, np);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) load_step(st[h].s1, st[h].ld, c, np);
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
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int sb = 0; sb < SUBS; ++sb) st[h].acc[sb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = 0; c < n_chunks; ++c) {
            const int64_t kc0 = static_cast<int64_t>(c) * geo.chunk_k;
            const int np = packets_of(c);
            if (c > 0) prime(c);                            // (chunk 0: before the loop or before the previous tile's epilogue)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int sb = 0; sb < SUBS; ++sb) st[h].P[sb] = i32x4{0, 0, 0, 0};
                st[h].C = i32x4{0, 0, 0, 0};
                st[h].pig = 0;
                st[h].g_local = (wave + kMidWaves * h) * geo.groups_per_span;
                st[h].sl = 0;
            }
            // places [j0, j1) of step s of slot S; xw: the slot's place j0 in the window, row nl
            auto compute_step = [&](Slot& S, const Step& s, int j0, int j1, const unsigned char* xw) {
                uint32_t r[4] = {s.raw.x, s.raw.y, s.raw.z, s.raw.w};
                transpose_over_rows(r);
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const int t = j * PER;
                    if (j < j0 || j >= j1 || s.p + t >= np) continue;      // the same for the whole wave
                    const unsigned char* xa = xw + (j - j0) * PB;
                    i32x4 b;
                    if constexpr (BITS == 2) {
                        const uint32_t v = r[t];
                        b = i32x4{static_cast<int>(v & 0x03030303u), static_cast<int>((v >> 2) & 0x03030303u),
                                  static_cast<int>((v >> 4) & 0x03030303u), static_cast<int>((v >> 6) & 0x03030303u)};
                    } else {
                        const uint32_t v = r[t], v2 = PAIR ? r[t + PER - 1] : 0u;
                        b = i32x4{static_cast<int>(v & 0x0F0F0F0Fu), static_cast<int>((v >> 4) & 0x0F0F0F0Fu),
                                  static_cast<int>(v2 & 0x0F0F0F0Fu), static_cast<int>((v2 >> 4) & 0x0F0F0F0Fu)};
                    }
#pragma unroll
                    for (int sb = 0; sb < SUBS; ++sb) {     // one B fragment, SUBS sub-tiles of rows
                        const unsigned char* xr = xa + sb * 16 * win.row_stride;
                        i32x4 a = {0, 0, 0, 0};
                        if (sb * 16 + nl < M) {
                            if constexpr (BITS == 2) {
                                a = *reinterpret_cast<const i32x4*>(xr + q * 16);
                            } else {
                                const u32x2 lo = *reinterpret_cast<const u32x2*>(xr + q * 8);
                                a.x = static_cast<int>(lo.x);
                                a.y = static_cast<int>(lo.y);
                                if constexpr (PAIR) {
                                    const u32x2 hi = *reinterpret_cast<const u32x2*>(xr + BE + q * 8);
                                    a.z = static_cast<int>(hi.x);
                                    a.w = static_cast<int>(hi.y);
                                }
                            }
                        }
                        S.P[sb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, S.P[sb], 0, 0, 0);
                    }
                    S.C = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b, S.C, 0, 0, 0);
                    S.pig += PER;
                    if (S.pig == geo.ppg) {                 // the group is complete: the same for the whole wave
                        const int32_t qz = w4_from_place(s.qz, lane, j);
                        const float qs = w4_from_place(s.qs, lane, j);
                        const bool far = qz < -kW4FastZero || qz > kW4FastZero;
                        const bool any_far = __ballot(far) != 0;
#pragma unroll
                        for (int sb = 0; sb < SUBS; ++sb) {
                            // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register: the lane's four rows are one packet
                            const i32x4 ae4 = *reinterpret_cast<const i32x4*>(aeff + S.g_local * MS + sb * 16 + q * 4);
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const int ae = ae4[i];
                                float f;
                                if (!any_far) {
                                    f = static_cast<float>(S.P[sb][i] - ac.z * S.C[i] - qz * ae);
                                } else {
                                    f = static_cast<float>(static_cast<int64_t>(S.P[sb][i]) - static_cast<int64_t>(ac.z) * S.C[i] -
                                                           static_cast<int64_t>(qz) * ae);
                                }
                                S.acc[sb][i] = __fadd_rn(S.acc[sb][i], __fmul_rn(qs, f));
                            }
                            S.P[sb] = i32x4{0, 0, 0, 0};
                            __builtin_amdgcn_sched_barrier(0);      // one sub-tile's table entries at a time
                        }
                        S.C = i32x4{0, 0, 0, 0};
                        S.pig = 0;
                        ++S.g_local;
                    }
                    __builtin_amdgcn_sched_barrier(0);      // one place's operands at a time: the registers go to the accumulators
                }
                if (j1 == NS && ++S.sl == geo.steps_per_span) {
                    S.sl = 0;
                    S.g_local += group_jump;
                }
            };

            // the windows of this chunk: slot 0 has the most places of any slot
            const int spans = (np + geo.span_p - 1) / geo.span_p;
            const int places = ((spans + kQWaves - 1) / kQWaves) * geo.steps_per_span * NS;
            for (int g0 = 0; g0 < places; g0 += win.wpl) {
                if (!win.resident || tile == first_tile) {  // x stays in LDS across tiles when one window holds it
                    __syncthreads();
                    mid_stage_window<BITS, PAIR>(act, ac, M, geo, win, kc0, np, g0, xs, aeff, MS, tid);
                }
                const int g1 = std::min(g0 + win.wpl, places);
                auto run_slot = [&](Slot& S, int slot) {    // the slot's places of this window
                    const unsigned char* xw = xs + slot * win.wpl * PB + nl * win.row_stride;
                    for (int gp = g0; gp < g1;) {           // the same for the whole wave; a step is reissued behind its last MFMA
                        const int t = gp / NS, j0 = gp - t * NS, j1 = std::min(NS, j0 + g1 - gp);
                        if (t & 1) {
                            if (S.s1.p >= 0) {
                                compute_step(S, S.s1, j0, j1, xw + (gp - g0) * PB);
                                if (j1 == NS) load_step(S.s1, S.ld, c, np);
                            }
                        } else {
                            if (S.s0.p >= 0) {
                                compute_step(S, S.s0, j0, j1, xw + (gp - g0) * PB);
                                if (j1 == NS) load_step(S.s0, S.ld, c, np);
                            }
                        }
                        gp += j1 - j0;
                    }
                };
                run_slot(st[0], wave);
                run_slot(st[1], wave + kMidWaves);
            }
        }
        // the next tile's first steps, in flight across this tile's epilogue
        const int next_tile = tile + static_cast<int>(gridDim.x);
        if (next_tile < tiles) {
            rows_of(next_tile);
            prime(0);
        }

        if constexpr (RES) {                                // without packets: the residual tile into the byte tile byte by byte along n
            if (!res.packets) {                             // (consecutive lanes on consecutive bytes)
                for (int i = tid; i < kMidTileBytes; i += kMidBlock) {
                    const int m = i >> 4;
                    const int64_t n = n0 + (i & 15);
                    if (m < M && n < N) tileb[i] = res.l[static_cast<int64_t>(m) * N + n];
                }
            }
        }
        // the slots' tiles, summed in slot order, one sub-tile per pass
#pragma unroll
        for (int sb = 0; sb < SUBS; ++sb) {
#pragma unroll
            for (int h = 0; h < 2; ++h) *reinterpret_cast<f32x4*>(red + ((wave + kMidWaves * h) * 64 + lane) * 4) = st[h].acc[sb];
            __syncthreads();
            if (tid < 256) {                                // one thread per output
                const int l = tid & 63, reg = tid >> 6;
                const int col = l & 15, m = sb * 16 + (l >> 4) * 4 + reg;
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
            __syncthreads();                                // the sums are free for the next sub-tile
        }
        if (out.packets) {                                  // N % 16 == 0: the tile's 16 columns lie inside N
            if (row_lane) *reinterpret_cast<u32x4*>(y + static_cast<int64_t>(lane) * N + n0) = *reinterpret_cast<const u32x4*>(tileb + lane * kQTile);
        } else {
            for (int i = tid; i < kMidTileBytes; i += kMidBlock) {
                const int m = i >> 4;
                const int64_t n = n0 + (i & 15);
                if (m < M && n < N) y[static_cast<int64_t>(m) * N + n] = tileb[i];
            }
        }
        __syncthreads();                                    // the byte tile is free for the next tile
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launcher
// ------------------------------------------------------------------------------------------------
struct MidPlan {
    int served, block, lds, subs, stages, store, res_load;
    bool pair;
    int64_t grid;
    W4Geom geo;
    MidWin win;
};

// the cut of K is lindec_w4's (w4_cut); the window is the largest whole number of steps of every slot whose rows fit next to the
// sums, the byte tile and the table of sum a - G z -- or 2 or 1 places of one step
inline MidPlan plan_linmid_w4(int64_t M, int64_t N, int64_t K, int64_t G, int bits, bool aligned, bool y_aligned, bool res_aligned) {
    MidPlan pl{};
    if (M < LSQ_LINMID_W4_MIN_ROWS || !w4_cut(M, N, K, G, bits, aligned, LSQ_LINMID_W4_MAX_ROWS, pl.geo, pl.pair)) return pl;
    const W4Geom& g = pl.geo;
    const int m = static_cast<int>(M), BE = 128 / bits, per = pl.pair ? 2 : 1, ns = 4 / per, pb = per * BE;
    const int np = static_cast<int>(std::min<int64_t>(static_cast<int64_t>(g.chunk_spans) * g.span_p, g.n_packets));   // of chunk 0
    const int spans = (np + g.span_p - 1) / g.span_p;
    const int places = ((spans + kQWaves - 1) / kQWaves) * g.steps_per_span * ns;
    const int table = (m + 15) / 16 * 16 * g.gstride * 4;  // sum a - G z: whole sub-tiles of rows
    const int per_row = (kMidMaxLds - kMidFixedLds - table) / m - kQRowPad;
    int wpl = per_row / (kQWaves * pb);
    if (wpl < 1) return pl;                                 // (not reached by a served format: 64 rows of one place are 64 KB)
    if (wpl >= ns) wpl = std::min(places, wpl / ns * ns);
    else if (wpl == 3) wpl = 2;
    pl.win.wpl = wpl;
    pl.win.row_stride = kQWaves * wpl * pb + kQRowPad;
    pl.stages = (places + wpl - 1) / wpl;
    pl.win.resident = (g.n_chunks == 1 && pl.stages == 1) ? 1 : 0;
    pl.served = 1;
    pl.block = kMidBlock;
    pl.subs = (m + 15) / 16;
    pl.lds = kMidFixedLds + m * pl.win.row_stride + table;
    pl.grid = mfma_grid(N, device_info().cu_count);
    pl.store = (N % 16 == 0 && y_aligned) ? LSQ_LINMID_W4_PACKETS : LSQ_LINMID_W4_BYTES;
    pl.res_load = (N % 16 == 0 && res_aligned) ? LSQ_LINMID_W4_PACKETS : LSQ_LINMID_W4_BYTES;
    return pl;
}

struct MidCall {            // what every instantiation's launcher takes
    W8Act act;
    W4Weight wt;
    W8OutArg out;
    W8ResArg res;
    W8PreArg pre;
    uint8_t* y;
    int M;
};

template <int BITS, bool PAIR, bool RES, int SUBS>
static hipError_t mid_launch(const MidPlan& pl, const MidCall& c, hipStream_t stream) {
    static LdsOnce once;
    if (const hipError_t e = allow_lds(once, reinterpret_cast<const void*>(&linmid_w4_kernel<BITS, PAIR, RES, SUBS>), kMidMaxLds)) return e;
    hipLaunchKernelGGL((linmid_w4_kernel<BITS, PAIR, RES, SUBS>), dim3(static_cast<unsigned>(pl.grid)), dim3(kMidBlock), pl.lds, stream,
                       c.act, c.M, c.wt, pl.geo, pl.win, c.out, c.res, c.pre, c.y);
    return hipGetLastError();
}

template <int BITS, bool PAIR, bool RES>
static hipError_t mid_launch_subs(const MidPlan& pl, const MidCall& c, hipStream_t stream) {
    if (pl.subs == 2) return mid_launch<BITS, PAIR, RES, 2>(pl, c, stream);
    return pl.subs == 3 ? mid_launch<BITS, PAIR, RES, 3>(pl, c, stream) : mid_launch<BITS, PAIR, RES, 4>(pl, c, stream);
}

template <bool RES>
static hipError_t mid_launch_format(const MidPlan& pl, int bits, const MidCall& c, hipStream_t stream) {
    if (bits == 2) return mid_launch_subs<2, false, RES>(pl, c, stream);
    return pl.pair ? mid_launch_subs<4, true, RES>(pl, c, stream) : mid_launch_subs<4, false, RES>(pl, c, stream);
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_linmid_w4.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// what this form serves; everything else that is legal belongs to lsq_hip_lindec_w4.h, lsq_hip_qlinear_a8.h and the ops after it
int check_served(const char* what, const lsq::MidPlan& pl, int64_t M, int64_t K, int64_t G, int bits, bool aligned) {
    const char* other = "lsq_hip_lindec_w4.h up to 16 rows, else compose lsq_hip_qlinear_a8.h / lsq_hip_qgemm_a8.h with the per-tensor levels forward";
    if (M < LSQ_LINMID_W4_MIN_ROWS || M > LSQ_LINMID_W4_MAX_ROWS)
        return fail(LSQ_EINVAL, "%s: M = %lld rows of x, this kernel serves %d to %d (%s)", what, static_cast<ll>(M), LSQ_LINMID_W4_MIN_ROWS,
                    LSQ_LINMID_W4_MAX_ROWS, other);
    if (!aligned) return fail(LSQ_EINVAL, "%s: codes and x_levels must be 16-byte aligned (otherwise: %s)", what, other);
    if (!pl.served)
        return fail(LSQ_EINVAL, "%s: K = %lld, group_size %lld at %d bits: this kernel serves K > 0 and groups of whole 16-byte code "
                    "packets (%d elements) with lcm(group_size, 4 packets) <= %d elements (otherwise: %s)", what, static_cast<ll>(K),
                    static_cast<ll>(G), bits, 128 / bits, lsq::kQChunk, other);
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_linmid_w4_abi_version(void) { return LSQ_LINMID_W4_ABI_VERSION; }

const char* lsq_linmid_w4_last_error(void) { return g_last_error; }

int lsq_linmid_w4_linear_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, const void* codes,
                                int64_t N, int64_t K, int64_t group_size, int bits, const void* qscale, const void* qzero,
                                const void* bias, int bias_dtype, const lsq_requant_w8_out* out, const lsq_resadd_w8_res* res,
                                const lsq_resadd_w8_pre* pre, void* y, void* stream) {
    const char* what = "lsq_linmid_w4_linear_levels";
    int mid = 0;
    lsq::MidCall c{};
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
    const lsq::MidPlan pl = lsq::plan_linmid_w4(M, N, K, group_size, bits, aligned, aligned_to(y, 16), res && aligned_to(res->levels, 16));
    if (int rc = check_served(what, pl, M, K, group_size, bits, aligned)) return rc;
    if (N == 0) return LSQ_OK;
    c.act = levels_act(level_dtype, x_levels, s_x, zx);
    c.wt = lsq::W4Weight{static_cast<const uint8_t*>(codes), static_cast<const float*>(qscale), static_cast<const int32_t*>(qzero), bias,
                         bias_dtype};
    c.out.packets = pl.store == LSQ_LINMID_W4_PACKETS ? 1 : 0;
    c.res.packets = pl.res_load == LSQ_LINMID_W4_PACKETS ? 1 : 0;
    c.y = static_cast<uint8_t*>(y);
    c.M = static_cast<int>(M);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return hip_status(res ? lsq::mid_launch_format<true>(pl, bits, c, st) : lsq::mid_launch_format<false>(pl, bits, c, st), what);
}

int lsq_linmid_w4_plan(int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int aligned, int y_aligned, int res_aligned,
                       int32_t* out8) {
    const char* what = "lsq_linmid_w4_plan";
    if (int rc = check_format(what, M, N, K, group_size, bits)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::MidPlan pl = lsq::plan_linmid_w4(M, N, K, group_size, bits, aligned != 0, y_aligned != 0, res_aligned != 0);
    out8[0] = pl.served;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.block;
    out8[3] = pl.lds;
    out8[4] = pl.subs;
    out8[5] = pl.stages;
    out8[6] = pl.store;
    out8[7] = pl.res_load;
    return LSQ_OK;
}

}  // extern "C"
