// lsq_attn_paged_w8.hip -- a paged KV cache on 8-bit levels on gfx950 (include/lsq_hip_attn_paged_w8.h, which states the contract): the
// append kernel, the three decode kernels and the C ABI of liblsq_hip_attn_paged_w8.so.
//
// The decode is ../attn_decode_split_w8/lsq_attn_decode_split_w8.hip's, kernel for kernel -- the row tile, the chunks, the workspace, the
// arithmetic and every byte --, with ONE difference: a key's row is not K + j k_ld but lies in the page the block table names,
//     row(b, hkv, j) = pool + clamp(block_table[b, j >> log2 ps], 0, Np - 1) * page stride + hkv * head stride + (j & (ps - 1)) * slot stride.
// ps is a power of two >= 16, so the 16 keys of a sub-tile of launch 1 (and the clamped last key c1 - 1, which lies in the sub-tile
// that holds 16 j < c1) and the 4 keys of a v group of launch 2 share one entry.  The entry loads are kept off the packet loads'
// critical path:
//  1 paged_scores   a wave holds the entries of its four sub-tiles of the round in registers BEFORE the round's k packets are
//                   issued; the next round's four are issued behind those packets and are first used after this round's MFMAs.
//  2 paged_context  a thread's two (four keys, a word) items of a step take their entries from registers that were loaded one step
//                   earlier: the v rows are loaded one step ahead, their entries two steps ahead and issued in front of those rows'
//                   loads, so that they complete under the first row's wait.
//  3 paged_reduce   the split library's reduce.
// The entry loads carry no branch (a guarded load is waited for at once): an index at or beyond the chunk's end is clamped to the
// chunk's last sub-tile or key, so only entries of keys below c1 <= nmax are read -- table entries at logical pages
// >= ceil(nmax / ps) and pool bytes at keys >= nmax are never read.  No atomics, no flags: the stream orders the three launches.
//
// kv_append_paged: one lane per 16-byte packet (or per byte) of k and of v; a token whose position or entry is out of range is
// skipped as a whole.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../qlinear_w8/lsq_w8_shared.hpp"
#include "../attn_w8/lsq_attn_w8_dev.hpp"
#include "../attn_w8/lsq_attn_w8_checks.hpp"
#include "../../../include/lsq_hip_attn_paged_w8.h"

namespace lsq {

typedef __attribute__((ext_vector_type(2))) unsigned short pg_u16x2;

constexpr int kPgRows = LSQ_ATTN_PAGED_W8_MAX_ROWS;             // the row tile of the matrix core
constexpr int kPgThreads = LSQ_ATTN_PAGED_W8_THREADS;
constexpr int kPgWaves = kPgThreads / 64;
constexpr int kPgStep = 64;                                     // keys per step of launch 2, and what a chunk is a multiple of
constexpr int kPgTStride = kPgStep + 16;                        // bytes between the rows of a p tile or a transposed v tile in LDS
constexpr int kPgInFlight = 4;                                  // 16-key sub-tiles of k a wave loads before it multiplies
constexpr int kPgRound = 16 * kPgInFlight * kPgWaves;           // keys a workgroup scores between two barriers: 256
constexpr int kPgScoreLd = kPgRound + 16;                       // bytes between the score rows of a round in LDS
constexpr int kPgSubsPerWave = 2;                               // D / 16 <= 8 accumulator sub-tiles over four waves
constexpr int kPgTable = 1024;
constexpr int kPgRowInfo = 256;                                 // m, 1 / S and n of the 16 rows
constexpr int kPgScoreLds = kPgRows * kPgScoreLd;
constexpr int pg_context_lds(int D) { return kPgTable + kPgRowInfo + 2 * kPgRows * kPgTStride + 2 * kPgTStride * D; }
static_assert(kPgSubsPerWave * kPgWaves * 16 >= LSQ_ATTN_PAGED_W8_MAX_D, "four waves cover every sub-tile of D");
static_assert(kPgRows * 16 == kPgThreads, "one thread per (row, word) of a p tile and per (row, packet) of a round");
static_assert(pg_context_lds(LSQ_ATTN_PAGED_W8_MAX_D) <= 65536 && kPgScoreLds <= 65536, "no launch asks for more LDS than a kernel gets unasked");
static_assert(LSQ_ATTN_PAGED_W8_MIN_PAGE % 16 == 0, "a sub-tile of launch 1 lies in one page");

struct PgGeom {             // kernel argument
    int64_t q_s0, q_s1, q_ld, k_sp, k_sh, k_ss, v_sp, v_sh, v_ss, y_s0, y_s1, y_ld;
    int64_t ldw;            // bytes between the score rows in the workspace: Tk (a multiple of 16)
    int64_t bt_ld;          // elements between the rows of the block table
    int Hkv, G, Tq, Tk, D;
    int R;                  // G Tq
    int causal, off;        // row t sees t + 1 + off keys (off clamped to Tk on the host)
    int chunk, S;           // keys of a chunk (a multiple of 64); ceil(Tk / chunk)
    int Np, lps, psm;       // pages of a pool; log2 ps; ps - 1
};

struct PgArg {              // kernel argument
    const float* s_q;
    const int32_t* z_q;
    const float* s_k;
    const int32_t* z_k;
    const float* s_v;
    const int32_t* z_v;
    const float* s_p;
    const int32_t* z_p;
    int off_q, off_k, off_v, off_s, off_p;      // 128: uint8 levels; 0: int8 (s: the scores, p: the probabilities)
    int y_packets;                              // y's base and strides are multiples of 16
};

// n(b, t) of the contract; len: max(key_lengths[b], 0), or Tk without lengths
__device__ __forceinline__ int pg_count(const PgGeom& g, int len, int t) {
    int n = min(g.Tk, len);
    if (g.causal) n = min(n, t + 1 + g.off);           // t < 16 and off <= Tk <= 65536
    return n;
}

// the page of key j of the batch entry whose table row is `row`: READS CLAMP (j < Tk = Mp ps, so j >> lps < Mp)
__device__ __forceinline__ int pg_entry(const PgGeom& g, const int32_t* __restrict__ row, int j) {
    return min(max(row[j >> g.lps], 0), g.Np - 1);
}

// ------------------------------------------------------------------------------------------------ launch 1: the scores of a chunk
__global__ __launch_bounds__(kPgThreads) void attn_paged_scores_kernel(PgGeom g, PgArg a, AttnOut so, const int32_t* __restrict__ lens,
                                                                       const int32_t* __restrict__ bt, const uint8_t* __restrict__ Q,
                                                                       const uint8_t* __restrict__ K, uint8_t* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) unsigned char sc[kPgScoreLds];       // [16][272]: the score bytes of a round
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const int64_t bh = static_cast<int64_t>(blockIdx.x) / g.S;
    const int s = static_cast<int>(static_cast<int64_t>(blockIdx.x) - bh * g.S);
    const int64_t b0 = bh / g.Hkv, b1 = bh - b0 * g.Hkv;
    const int len = lens ? max(lens[b0], 0) : g.Tk;
    const int nmax = pg_count(g, len, g.Tq - 1);                        // 0 .. Tk, the same for the S workgroups of the head
    const int c0 = s * g.chunk;                                         // s chunk < Tk + chunk: no overflow
    if (c0 >= nmax) return;                                             // the same for the whole workgroup, before any barrier
    const int c1 = min(c0 + g.chunk, nmax);
    const int jend = (c1 + 15) >> 4;                                    // 16-key sub-tiles below c1
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const uint32_t flip_q = a.off_q ? 0x80808080u : 0u, flip_k = a.off_k ? 0x80808080u : 0u;
    const int r = min(nl, g.R - 1);                                     // a clamped row computes values nobody stores
    const int rg = r / g.Tq, rt = r - rg * g.Tq;
    const uint8_t* __restrict__ qrow = Q + b0 * g.q_s0 + (b1 * g.G + rg) * g.q_s1 + static_cast<int64_t>(rt) * g.q_ld;
    const uint8_t* __restrict__ Kh = K + b1 * g.k_sh;                   // the kv head's slots of page 0
    const int32_t* __restrict__ btrow = bt + b0 * g.bt_ld;
    i32x4 qi[2], Rs = {0, 0, 0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int kk = 64 * h + 16 * q;
        u32x4 v = {0u, 0u, 0u, 0u};                                     // a packet beyond D: the operand's zero
        if (kk < g.D) v = *reinterpret_cast<const u32x4*>(qrow + kk) ^ flip_q;
        qi[h] = w8_as_i32(v);
        Rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(qi[h], ones, Rs, 0, 0, 0);         // sum_k q of row 4 q + i in register i
    }
    const AttnQ sq = attn_constants(so);
    const BmmInt ex = bmm_int_constants(static_cast<int64_t>(a.z_q[0]) - a.off_q, static_cast<int64_t>(a.z_k[0]) - a.off_k, g.D);
    const float s_q = a.s_q[0], s_k = a.s_k[0];
    const bool two = g.D > 64;                                          // the same for the whole grid
    uint8_t* __restrict__ wrow = ws + (bh * g.R + (tid >> 4)) * g.ldw;  // the row this thread copies out (used where tid / 16 < R)
    // the pages of this wave's sub-tiles of the round.  The loads carry no branch, so that all four are in flight at once: a sub-tile
    // at or beyond jend takes the entry of the chunk's last one (16 (jend - 1) < c1 <= nmax: a live logical page) and is never used
    int ent[kPgInFlight];
#pragma unroll
    for (int u = 0; u < kPgInFlight; ++u) ent[u] = pg_entry(g, btrow, 16 * min((c0 >> 4) + wave * kPgInFlight + u, jend - 1));
    for (int jb = c0 >> 4; jb < jend; jb += kPgRound / 16) {            // the same for the whole workgroup
        const int j0 = jb + wave * kPgInFlight;
        u32x4 kv[kPgInFlight][2];
#pragma unroll
        for (int u = 0; u < kPgInFlight; ++u) {
            kv[u][0] = u32x4{0u, 0u, 0u, 0u};
            kv[u][1] = u32x4{0u, 0u, 0u, 0u};
            if (j0 + u < jend) {
                // 16 (j0 + u) < c1: the clamped key is a key of the chunk, in this sub-tile and so in this page
                const int key = min(16 * (j0 + u) + nl, c1 - 1);
                const uint8_t* __restrict__ kr = Kh + static_cast<int64_t>(ent[u]) * g.k_sp + static_cast<int64_t>(key & g.psm) * g.k_ss;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int kk = 64 * h + 16 * q;
                    if (kk < g.D) kv[u][h] = *reinterpret_cast<const u32x4*>(kr + kk) ^ flip_k;        // a packet beyond D: the operand's zero
                }
            }
        }
        int nxt[kPgInFlight];                                           // the next round's pages, in flight behind the packets
#pragma unroll
        for (int u = 0; u < kPgInFlight; ++u) nxt[u] = pg_entry(g, btrow, 16 * min(j0 + kPgRound / 16 + u, jend - 1));
#pragma unroll
        for (int u = 0; u < kPgInFlight; ++u) {
            asm volatile("" : "+v"(kv[u][0]));                          // all in flight at once
            asm volatile("" : "+v"(kv[u][1]));
        }
#pragma unroll
        for (int u = 0; u < kPgInFlight; ++u) {
            const int j = j0 + u;
            if (j >= jend) continue;
            i32x4 P = {0, 0, 0, 0}, Cs = {0, 0, 0, 0};
            const i32x4 k0 = w8_as_i32(kv[u][0]);
            P = __builtin_amdgcn_mfma_i32_16x16x64_i8(qi[0], k0, P, 0, 0, 0);
            Cs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, k0, Cs, 0, 0, 0);       // sum_k k of the lane's key, in every register
            if (two) {
                const i32x4 k1 = w8_as_i32(kv[u][1]);
                P = __builtin_amdgcn_mfma_i32_16x16x64_i8(qi[1], k1, P, 0, 0, 0);
                Cs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, k1, Cs, 0, 0, 0);
            }
            // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register; 16 (j - jb) + nl < 256
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float uu = bmm_value(bmm_int_float(ex, P[i], Cs[i], Rs[i]), s_q, s_k, sq.mid);
                sc[(4 * q + i) * kPgScoreLd + 16 * (j - jb) + nl] = static_cast<unsigned char>(w8o_byte(uu, sq));
            }
        }
#pragma unroll
        for (int u = 0; u < kPgInFlight; ++u) ent[u] = nxt[u];
        __syncthreads();                                                // the round's scores are in LDS
        {
            const int pr = tid >> 4, pk = tid & 15;                     // (row, packet of the round)
            // 16 (jb + pk) + 16 <= 16 jend <= Tk = ldw
            if (pr < g.R && jb + pk < jend)
                *reinterpret_cast<u32x4*>(wrow + 16 * static_cast<int64_t>(jb + pk)) = *reinterpret_cast<const u32x4*>(sc + pr * kPgScoreLd + 16 * pk);
        }
        __syncthreads();                                                // before the next round overwrites them
    }
}

// ------------------------------------------------------------------------------------------------ launch 2: the chunk's context integer
__global__ __launch_bounds__(kPgThreads) void attn_paged_context_kernel(PgGeom g, PgArg a, AttnOut po, const int32_t* __restrict__ table,
                                                                        const int32_t* __restrict__ lens, const int32_t* __restrict__ bt,
                                                                        const uint8_t* __restrict__ V, const uint8_t* __restrict__ ws,
                                                                        int64_t* __restrict__ wi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int32_t* tab = reinterpret_cast<int32_t*>(lds);                                 // [256]
    int* row_m = reinterpret_cast<int*>(lds + kPgTable);                            // [16] the biased byte maximum
    float* row_r = reinterpret_cast<float*>(lds + kPgTable + 64);                   // [16] 1 / float(S), 0 where n = 0
    int* row_n = reinterpret_cast<int*>(lds + kPgTable + 128);                      // [16] n_r, 0 in rows >= R
    unsigned char* ptile = lds + kPgTable + kPgRowInfo;                             // 2 x [16][80]: p bytes, the operand's sign flip applied
    unsigned char* stage = ptile + 2 * kPgRows * kPgTStride;                        // 2 x [D][80]: v transposed
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const int64_t bh = static_cast<int64_t>(blockIdx.x) / g.S;
    const int s = static_cast<int>(static_cast<int64_t>(blockIdx.x) - bh * g.S);
    const int64_t b0 = bh / g.Hkv, b1 = bh - b0 * g.Hkv;
    const int len = lens ? max(lens[b0], 0) : g.Tk;
    const int nmax = pg_count(g, len, g.Tq - 1);
    const int c0 = s * g.chunk;
    if (c0 >= nmax) return;                                             // the same for the whole workgroup, before any barrier
    const int c1 = min(c0 + g.chunk, nmax);
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const uint32_t flip_s = a.off_s ? 0u : 0x80808080u;                 // int8 levels are biased by 128 on load
    const uint8_t* __restrict__ wsb = ws + bh * g.R * g.ldw;            // the head's score rows [R][ldw]

    tab[tid] = table[tid];                                              // 256 threads
    __syncthreads();

    // ---- the rows' maximum and sum over their WHOLE prefix: packets below 16 ceil(n_r / 16) <= 16 ceil(nmax / 16), all written
    for (int r = wave; r < kPgRows; r += kPgWaves) {                    // the same for the whole wave
        int n = 0, m = 0;
        float rcp = 0.0f;
        if (r < g.R) {
            const uint8_t* __restrict__ row = wsb + r * g.ldw;
            n = pg_count(g, len, r % g.Tq);                             // n <= nmax
            const int npk = (n + 15) >> 4;
            pg_u16x2 me = {0, 0}, mo = {0, 0};
            for (int p = lane; p < npk; p += 64) {
                // bytes beyond n count as 0, the least biased byte
                const u32x4 v = attn_mask_tail(*reinterpret_cast<const u32x4*>(row + 16 * p) ^ flip_s, n - 16 * p);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    me = __builtin_elementwise_max(me, __builtin_bit_cast(pg_u16x2, v[i] & 0x00ff00ffu));
                    mo = __builtin_elementwise_max(mo, __builtin_bit_cast(pg_u16x2, (v[i] >> 8) & 0x00ff00ffu));
                }
            }
            me = __builtin_elementwise_max(me, mo);
            m = max(static_cast<int>(me[0]), static_cast<int>(me[1]));
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) m = max(m, __shfl_xor(m, sh));
            uint64_t S = 0;
            for (int p = lane; p < npk; p += 64) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(row + 16 * p) ^ flip_s;
                const int valid = min(n - 16 * p, 16);
                uint32_t part = 0;                                      // 16 entries of at most 2^24
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int b = static_cast<int>((v[i / 4] >> (8 * (i % 4))) & 0xffu);
                    part += i < valid ? static_cast<uint32_t>(tab[(m - b) & 0xff]) : 0u;
                }
                S += part;
            }
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) S += smx_shfl_xor_u64(S, sh);
            if (n > 0) rcp = __fdiv_rn(1.0f, static_cast<float>(S));   // n = 0: nothing is divided and no p is formed
        }
        if (lane == 0) {
            row_m[r] = m;
            row_r[r] = rcp;
            row_n[r] = n;
        }
    }
    __syncthreads();

    // ---- the chunk in 64-key steps
    const AttnQ pq = attn_constants(po);
    const uint32_t zb = static_cast<uint32_t>(a.z_p[0]) & 0xffu;        // the byte z_p
    const uint32_t fb = a.off_p ? 0x80u : 0u, flip_v = a.off_v ? 0x80808080u : 0u;
    const int pr = tid >> 4, pw = tid & 15;                             // this thread's (row, word) of a p tile
    const int my_n = row_n[pr], my_m = row_m[pr];
    const float my_r = row_r[pr];
    const uint8_t* __restrict__ srow = wsb + min(pr, g.R - 1) * g.ldw;  // read only where a key lies below my_n (0 in rows >= R)
    const uint8_t* __restrict__ Vh = V + b1 * g.v_sh;                   // the kv head's slots of page 0
    const int32_t* __restrict__ btrow = bt + b0 * g.bt_ld;
    const int subs = g.D >> 4;                                          // 16-column sub-tiles of the context, 1 .. 8
    const int wpr = g.D >> 2, items = 16 * wpr;                         // words of a v row; (four keys, a word) items of a step
    i32x4 P[kPgSubsPerWave], Cs[kPgSubsPerWave], Rs = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < kPgSubsPerWave; ++j) {
        P[j] = i32x4{0, 0, 0, 0};
        Cs[j] = i32x4{0, 0, 0, 0};
    }
    int kgs[2], ds[2];                                                  // this thread's two items: the group of four keys and the word
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = tid + it * kPgThreads;
        kgs[it] = idx / wpr;
        ds[it] = idx - kgs[it] * wpr;
    }
    uint32_t vr[2][4];                                                  // the rows of the step to be staged next
    uint32_t sw = 0u;                                                   // the score word of the step to be staged next
    int ent[2];                                                         // the pages of the items of the step to be LOADED next
    // the pages of the items' groups in the step that starts at key kb.  No branch, so that the loads stay in flight: a group at or
    // beyond c1 takes the entry of the key c1 - 1 (a key of the chunk, below nmax: a live page), from which no row is loaded
#define PG_ENTRIES(to, kb)                                                                                      \
    _Pragma("unroll") for (int it = 0; it < 2; ++it) to[it] = pg_entry(g, btrow, min((kb) + 4 * kgs[it], c1 - 1));
    // the rows of the step that starts at key kb, from the pages in `ent`: the four keys of a group share the page (ps % 16 == 0)
#define PG_ROWS(kb)                                                                                             \
    _Pragma("unroll") for (int it = 0; it < 2; ++it) {                                                          \
        const int kf = (kb) + 4 * kgs[it];                                                                      \
        const uint8_t* __restrict__ vp = Vh + static_cast<int64_t>(ent[it]) * g.v_sp +                         \
                                         static_cast<int64_t>(kf & g.psm) * g.v_ss + 4 * ds[it];                \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                         \
            vr[it][i] = 0u;                                             /* a row beyond c1: the operand's zero */ \
            if (tid + it * kPgThreads < items && kf + i < c1)                                                   \
                vr[it][i] = *reinterpret_cast<const uint32_t*>(vp + static_cast<int64_t>(i) * g.v_ss) ^ flip_v; \
        }                                                                                                       \
    }
    int nxt[2];                                                         // ... and of the step after it, issued AHEAD of the rows' loads
    PG_ENTRIES(ent, c0)
    PG_ENTRIES(nxt, c0 + kPgStep)
    PG_ROWS(c0)
    ent[0] = nxt[0];
    ent[1] = nxt[1];
    if (c0 + 4 * pw < my_n) sw = *reinterpret_cast<const uint32_t*>(srow + c0 + 4 * pw) ^ flip_s;       // my_n <= nmax: a written packet
    int buf = 0;
    for (int k0 = c0; k0 < c1; k0 += kPgStep) {                         // the same for the whole workgroup
        unsigned char* st = stage + buf * (kPgTStride * g.D);
        unsigned char* pt = ptile + buf * (kPgRows * kPgTStride);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            if (tid + it * kPgThreads < items) {
                uint32_t c[4];
                attn_transpose4(vr[it][0], vr[it][1], vr[it][2], vr[it][3], c);
#pragma unroll
                for (int i = 0; i < 4; ++i) *reinterpret_cast<uint32_t*>(st + (4 * ds[it] + i) * kPgTStride + 4 * kgs[it]) = c[i];
            }
        }
        {
            uint32_t w = 0u;                                            // from c1 on and in rows >= R: the operand's zero
            const int key = k0 + 4 * pw;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint32_t byte = 0u;
                if (key + i < my_n) {
                    const int b = static_cast<int>((sw >> (8 * i)) & 0xffu);
                    byte = w8o_byte(smx_value(tab[(my_m - b) & 0xff], my_r, pq.mid), pq) ^ fb;
                } else if (pr < g.R && key + i < c1) {
                    byte = zb ^ fb;                                     // the byte z_p in [n_r, c1): contributes (z_p - z_p) = 0
                }
                w |= (byte & 0xffu) << (8 * i);
            }
            *reinterpret_cast<uint32_t*>(pt + pr * kPgTStride + 4 * pw) = w;
        }
        if (k0 + kPgStep < c1) {                                        // the next step's rows are loaded during this one's staging,
            PG_ENTRIES(nxt, k0 + 2 * kPgStep)                           // the pages of the step after it issued ahead of them,
            PG_ROWS(k0 + kPgStep)                                       // from pages fetched a step ago
            ent[0] = nxt[0];
            ent[1] = nxt[1];
            sw = 0u;
            if (k0 + kPgStep + 4 * pw < my_n) sw = *reinterpret_cast<const uint32_t*>(srow + k0 + kPgStep + 4 * pw) ^ flip_s;
        }
        // this step's tiles are staged; the other buffers were last read before the previous step's barrier
        __syncthreads();
        const i32x4 ai = w8_as_i32(*reinterpret_cast<const u32x4*>(pt + nl * kPgTStride + q * 16));
#pragma unroll
        for (int jj = 0; jj < kPgSubsPerWave; ++jj) {
            const int j = wave + jj * kPgWaves;
            if (j < subs) {                                             // the same for the whole wave
                const i32x4 bi = w8_as_i32(*reinterpret_cast<const u32x4*>(st + (16 * j + nl) * kPgTStride + q * 16));
                P[jj] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ai, bi, P[jj], 0, 0, 0);
                Cs[jj] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bi, Cs[jj], 0, 0, 0);
            }
        }
        Rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ai, ones, Rs, 0, 0, 0);
        buf ^= 1;
    }
#undef PG_ENTRIES
#undef PG_ROWS

    // ---- the chunk's exact integer of the rows < R: |raw sums| <= 65536 * 128 * 128 = 2^30, I_c in 64 bits
    const int64_t z_p = static_cast<int64_t>(a.z_p[0]) - a.off_p, z_v = static_cast<int64_t>(a.z_v[0]) - a.off_v;
    int64_t* __restrict__ out = wi + ((bh * g.S + s) * g.R) * g.D;      // [R][D]
#pragma unroll
    for (int jj = 0; jj < kPgSubsPerWave; ++jj) {
        const int j = wave + jj * kPgWaves;
        if (j >= subs) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * q + i;                                    // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
            if (r < g.R) out[static_cast<int64_t>(r) * g.D + 16 * j + nl] = bmm_exact(P[jj][i], Cs[jj][i], Rs[i], c1 - c0, z_p, z_v);
        }
    }
}

// ------------------------------------------------------------------------------------------------ launch 3: the sum over the chunks, the levels
__global__ __launch_bounds__(kPgThreads) void attn_paged_reduce_kernel(PgGeom g, PgArg a, AttnOut co, const int32_t* __restrict__ lens,
                                                                       const int64_t* __restrict__ wi, uint8_t* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[kPgRows * LSQ_ATTN_PAGED_W8_MAX_D];      // the level tile [R][D]
    const int tid = static_cast<int>(threadIdx.x);
    const int64_t bh = static_cast<int64_t>(blockIdx.x);
    const int64_t b0 = bh / g.Hkv, b1 = bh - b0 * g.Hkv;
    const int len = lens ? max(lens[b0], 0) : g.Tk;
    const int nmax = pg_count(g, len, g.Tq - 1);
    const int live = (nmax + g.chunk - 1) / g.chunk;                    // the chunks that start below nmax: the ones launch 2 wrote; <= S
    const AttnQ oq = attn_constants(co);
    const float s_p = a.s_p[0], s_v = a.s_v[0];
    const int RD = g.R * g.D;                                           // <= 2048
    const int64_t* __restrict__ src = wi + bh * g.S * RD;               // [S][R][D]
    for (int e = tid; e < RD; e += kPgThreads) {
        int64_t I = 0;
        for (int c = 0; c < live; ++c) I += src[static_cast<int64_t>(c) * RD + e];
        const float u = bmm_value(static_cast<float>(I), s_p, s_v, oq.mid);
        tile[e] = static_cast<unsigned char>(w8o_byte(u, oq));
    }
    __syncthreads();
    uint8_t* __restrict__ yb = y + b0 * g.y_s0 + (b1 * g.G) * g.y_s1;
    const int subs = g.D >> 4, total = g.R * subs;                      // 16-byte packets of the rows that exist
    for (int idx = tid; idx < total; idx += kPgThreads) {
        const int r = idx / subs, c = (idx - r * subs) * 16;
        const int rg = r / g.Tq, rt = r - rg * g.Tq;
        uint8_t* dst = yb + rg * g.y_s1 + static_cast<int64_t>(rt) * g.y_ld + c;
        const unsigned char* from = tile + r * g.D + c;
        if (a.y_packets) {
            *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(from);
        } else {
            for (int i = 0; i < 16; ++i) dst[i] = from[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------ the append
struct ApGeom {             // kernel argument
    int64_t k_sb, k_st, k_sh, v_sb, v_st, v_sh, kp_sp, kp_sh, kp_ss, vp_sp, vp_sh, vp_ss;
    int64_t bt_ld;
    int64_t per;            // work units of one of k and v: B T Hkv units
    int64_t cap;            // Mp ps
    int T, Hkv, units, Np, ps;
};

// one lane per unit (a 16-byte packet, or a byte) of k and then of v; WRITES SKIP: a token outside the table's capacity or whose
// entry lies outside [0, Np) changes no byte
template <bool kPackets>
__global__ __launch_bounds__(kPgThreads) void kv_append_paged_kernel(ApGeom g, const int32_t* __restrict__ bt, const int32_t* __restrict__ pos,
                                                                     const uint8_t* __restrict__ k, const uint8_t* __restrict__ v,
                                                                     uint8_t* __restrict__ kp, uint8_t* __restrict__ vp) {
    int64_t i = static_cast<int64_t>(blockIdx.x) * kPgThreads + threadIdx.x;
    if (i >= 2 * g.per) return;
    const bool second = i >= g.per;
    if (second) i -= g.per;
    const int u = static_cast<int>(i % g.units);
    i /= g.units;
    const int h = static_cast<int>(i % g.Hkv);
    i /= g.Hkv;
    const int t = static_cast<int>(i % g.T);
    const int64_t b = i / g.T;
    const int64_t p = (pos ? static_cast<int64_t>(pos[b]) : 0) + t;
    if (p < 0 || p >= g.cap) return;
    const int64_t lp = p / g.ps;                                        // < Mp
    const int e = bt[b * g.bt_ld + lp];
    if (e < 0 || e >= g.Np) return;
    const int64_t slot = p - lp * g.ps;
    const int64_t o = (kPackets ? 16 : 1) * static_cast<int64_t>(u);
    const uint8_t* __restrict__ src = second ? v + b * g.v_sb + t * g.v_st + h * g.v_sh + o : k + b * g.k_sb + t * g.k_st + h * g.k_sh + o;
    uint8_t* __restrict__ dst = second ? vp + e * g.vp_sp + h * g.vp_sh + slot * g.vp_ss + o : kp + e * g.kp_sp + h * g.kp_sh + slot * g.kp_ss + o;
    if (kPackets) {
        *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
    } else {
        *dst = *src;
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plans
// ------------------------------------------------------------------------------------------------
struct PgPlan {
    int family, rows, chunk, splits, lds, store;
    int64_t grid, heads, ldw, ws_scores, ws_bytes;      // B Hkv S; B Hkv; the workspace's row stride, its score part and its size
    PgGeom g;
};

inline bool strides16(const lsq_attn_w8_strides& s) { return s.s0 % 16 == 0 && s.s1 % 16 == 0 && s.ld % 16 == 0; }

// the chunk for `splits` (0: the library's own choice; else at most that many splits), a multiple of 64: the split library's rule
inline int64_t paged_chunk(int64_t heads, int64_t Tk, int64_t splits) {
    const int64_t units = (Tk + kPgStep - 1) / kPgStep;
    if (splits > 0) return kPgStep * ((units + splits - 1) / splits);
    const int64_t want = static_cast<int64_t>(LSQ_ATTN_PAGED_W8_WG_PER_CU) * LSQ_ATTN_PAGED_W8_CUS;
    const int64_t fewest = std::min<int64_t>((want + heads - 1) / heads, LSQ_ATTN_PAGED_W8_MAX_SPLITS);
    const int64_t chunk = kPgStep * ((units + fewest - 1) / fewest);
    return std::min<int64_t>(std::max<int64_t>(chunk, LSQ_ATTN_PAGED_W8_MIN_CHUNK), LSQ_ATTN_PAGED_W8_MAX_CHUNK);
}

inline bool paged_extents_served(const lsq_attn_decode_w8_geom& ge, const lsq_attn_paged_w8_pages& pg) {
    const int64_t R = ge.H / ge.Hkv * ge.Tq;
    return ge.D % 16 == 0 && ge.D >= 16 && ge.D <= LSQ_ATTN_PAGED_W8_MAX_D && R <= LSQ_ATTN_PAGED_W8_MAX_ROWS &&
           pg.ps >= LSQ_ATTN_PAGED_W8_MIN_PAGE && (pg.ps & (pg.ps - 1)) == 0;         // (Mp ps <= 65536: the API's own limit)
}

inline PgPlan plan_paged(const lsq_attn_decode_w8_geom& ge, const lsq_attn_paged_w8_pages& pg, bool qkv_aligned, bool y_aligned, int64_t splits) {
    PgPlan pl = {};
    pl.family = LSQ_ATTN_PAGED_W8_COMPOSITION;
    if (!(qkv_aligned && strides16(ge.q) && strides16(ge.k) && strides16(ge.v) && paged_extents_served(ge, pg))) return pl;
    const int64_t G = ge.H / ge.Hkv, R = G * ge.Tq;
    const int Tk = static_cast<int>(ge.Tk), D = static_cast<int>(ge.D);
    pl.family = LSQ_ATTN_PAGED_W8_PAGED;
    pl.heads = ge.B * ge.Hkv;
    pl.chunk = static_cast<int>(paged_chunk(pl.heads, ge.Tk, splits));
    pl.splits = (Tk + pl.chunk - 1) / pl.chunk;
    pl.rows = static_cast<int>(R);
    pl.lds = pg_context_lds(D);
    pl.store = y_aligned && strides16(ge.y) ? LSQ_ATTN_W8_STORE_PACKETS : LSQ_ATTN_W8_STORE_ELEMS;
    pl.grid = pl.heads * pl.splits;
    pl.ldw = ge.Tk;                                                     // Mp ps, a multiple of 16
    pl.ws_scores = pl.heads * R * pl.ldw;                               // a multiple of 16: the integers behind it are aligned
    pl.ws_bytes = pl.ws_scores + 8 * pl.heads * pl.splits * R * ge.D;
    int lps = 0;
    while ((int64_t{1} << lps) < pg.ps) ++lps;
    pl.g = PgGeom{ge.q.s0, ge.q.s1, ge.q.ld, ge.k.s0, ge.k.s1, ge.k.ld, ge.v.s0, ge.v.s1, ge.v.ld, ge.y.s0, ge.y.s1, ge.y.ld, pl.ldw, pg.bt_ld,
                  static_cast<int>(ge.Hkv), static_cast<int>(G), static_cast<int>(ge.Tq), Tk, D, pl.rows, ge.causal ? 1 : 0,
                  ge.causal ? static_cast<int>(std::min<int64_t>(ge.causal_offset, ge.Tk)) : 0, pl.chunk, pl.splits,
                  static_cast<int>(pg.Np), lps, static_cast<int>(pg.ps - 1)};
    return pl;
}

struct ApPlan {
    int family, units;
    int64_t grid;
    ApGeom g;
};

inline ApPlan plan_append(const lsq_kv_append_paged_w8_geom& ge, bool aligned) {
    ApPlan pl = {};
    const int64_t st[12] = {ge.k_sb, ge.k_st, ge.k_sh, ge.v_sb, ge.v_st, ge.v_sh, ge.kp_sp, ge.kp_sh, ge.kp_ss, ge.vp_sp, ge.vp_sh, ge.vp_ss};
    bool packets = aligned && ge.D % 16 == 0;
    for (int64_t s : st) packets = packets && s % 16 == 0;
    pl.family = packets ? LSQ_ATTN_PAGED_W8_APPEND_PACKETS : LSQ_ATTN_PAGED_W8_APPEND_GENERIC;
    pl.units = static_cast<int>(packets ? ge.D / 16 : ge.D);
    const int64_t per = ge.B * ge.T * ge.Hkv * pl.units;                // at most 2^40: check_append_geom
    pl.grid = (2 * per + kPgThreads - 1) / kPgThreads;
    pl.g = ApGeom{ge.k_sb, ge.k_st, ge.k_sh, ge.v_sb, ge.v_st, ge.v_sh, ge.kp_sp, ge.kp_sh, ge.kp_ss, ge.vp_sp, ge.vp_sh, ge.vp_ss,
                  ge.pages.bt_ld, per, ge.pages.Mp * ge.pages.ps, static_cast<int>(ge.T), static_cast<int>(ge.Hkv), pl.units,
                  static_cast<int>(ge.pages.Np), static_cast<int>(ge.pages.ps)};
    return pl;
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_attn_paged_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int64_t kMaxPages = (int64_t{1} << 31) - 1;       // an entry is an int32

int check_pages(const char* what, const lsq_attn_paged_w8_pages* p) {
    if (!p) return fail(LSQ_EINVAL, "%s: NULL pages", what);
    if (p->ps < 1 || p->Mp < 1 || p->Np < 1)
        return fail(LSQ_EINVAL, "%s: [Np, ps, Mp] = [%lld, %lld, %lld], every extent must be at least 1", what, static_cast<ll>(p->Np),
                    static_cast<ll>(p->ps), static_cast<ll>(p->Mp));
    if (p->Np > kMaxPages) return fail(LSQ_EINVAL, "%s: Np = %lld pages are beyond 2^31 - 1", what, static_cast<ll>(p->Np));
    if (p->bt_ld < p->Mp)
        return fail(LSQ_EINVAL, "%s: the block table's row stride bt_ld = %lld is smaller than its row of Mp = %lld", what,
                    static_cast<ll>(p->bt_ld), static_cast<ll>(p->Mp));
    return LSQ_OK;
}

// (the checks of lsq_attn_decode_w8, which that library keeps in its own translation unit, with k and v read as pools)
int check_paged_geom(const char* what, const lsq_attn_decode_w8_geom* g, const lsq_attn_paged_w8_pages* p) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (int rc = check_pages(what, p)) return rc;
    if (p->ps > LSQ_ATTN_PAGED_W8_MAX_TK || p->Mp > LSQ_ATTN_PAGED_W8_MAX_TK || p->Mp * p->ps > LSQ_ATTN_PAGED_W8_MAX_TK)
        return fail(LSQ_EINVAL, "%s: Mp ps = %lld x %lld keys, at most %d are served (the raw sums stay in 32 bits)", what,
                    static_cast<ll>(p->Mp), static_cast<ll>(p->ps), LSQ_ATTN_PAGED_W8_MAX_TK);
    if (!level_dtype(g->q_dtype) || !level_dtype(g->k_dtype) || !level_dtype(g->v_dtype))
        return fail(LSQ_EINVAL, "%s: q_dtype, k_dtype and v_dtype must be LSQ_ATTN_W8_U8 (0) or LSQ_ATTN_W8_I8 (1), got %lld, %lld and %lld",
                    what, static_cast<ll>(g->q_dtype), static_cast<ll>(g->k_dtype), static_cast<ll>(g->v_dtype));
    if (g->B < 1 || g->H < 1 || g->Hkv < 1 || g->Tq < 1 || g->Tk < 1 || g->D < 1)
        return fail(LSQ_EINVAL, "%s: [B, H, Hkv, Tq, Tk, D] = [%lld, %lld, %lld, %lld, %lld, %lld], every extent must be at least 1", what,
                    static_cast<ll>(g->B), static_cast<ll>(g->H), static_cast<ll>(g->Hkv), static_cast<ll>(g->Tq), static_cast<ll>(g->Tk),
                    static_cast<ll>(g->D));
    if (g->Tk != p->Mp * p->ps)
        return fail(LSQ_EINVAL, "%s: Tk = %lld is not the table's capacity Mp ps = %lld x %lld", what, static_cast<ll>(g->Tk),
                    static_cast<ll>(p->Mp), static_cast<ll>(p->ps));
    if (g->H % g->Hkv != 0)
        return fail(LSQ_EINVAL, "%s: H = %lld query heads are not a multiple of Hkv = %lld kv heads", what, static_cast<ll>(g->H),
                    static_cast<ll>(g->Hkv));
    if (g->causal && g->causal_offset < 0)
        return fail(LSQ_EINVAL, "%s: causal_offset = %lld must be at least 0", what, static_cast<ll>(g->causal_offset));
    if (g->D > LSQ_ATTN_W8_MAX_K)
        return fail(LSQ_EINVAL, "%s: D = %lld, at most %d are served (the raw sums stay in 32 bits)", what, static_cast<ll>(g->D),
                    LSQ_ATTN_W8_MAX_K);
    const int64_t lim = int64_t{1} << 20;
    if (g->Tq > lim || g->B > lim || g->H > lim || g->B * g->H > lim)
        return fail(LSQ_EINVAL, "%s: Tq = %lld and B * H = %lld x %lld may each be 2^20 at most", what, static_cast<ll>(g->Tq),
                    static_cast<ll>(g->B), static_cast<ll>(g->H));
    if (int rc = check_strides(what, "q", g->q, g->D)) return rc;
    if (int rc = check_strides(what, "k_pool", g->k, g->D)) return rc;
    if (int rc = check_strides(what, "v_pool", g->v, g->D)) return rc;
    if (int rc = check_strides(what, "y", g->y, g->D)) return rc;
    if (self_overlap(g->k, p->Np, g->Hkv, p->ps, g->D) || self_overlap(g->v, p->Np, g->Hkv, p->ps, g->D))
        return fail(LSQ_EINVAL, "%s: pages, heads or slots of a pool overlap each other (k strides %lld, %lld, %lld; v strides %lld, %lld, "
                    "%lld for [%lld, %lld, %lld, %lld])", what, static_cast<ll>(g->k.s0), static_cast<ll>(g->k.s1), static_cast<ll>(g->k.ld),
                    static_cast<ll>(g->v.s0), static_cast<ll>(g->v.s1), static_cast<ll>(g->v.ld), static_cast<ll>(p->Np),
                    static_cast<ll>(g->Hkv), static_cast<ll>(p->ps), static_cast<ll>(g->D));
    if (self_overlap(g->y, g->B, g->H, g->Tq, g->D))
        return fail(LSQ_EINVAL, "%s: y's rows or batches overlap each other (strides %lld, %lld, %lld for [%lld, %lld, %lld, %lld])", what,
                    static_cast<ll>(g->y.s0), static_cast<ll>(g->y.s1), static_cast<ll>(g->y.ld), static_cast<ll>(g->B),
                    static_cast<ll>(g->H), static_cast<ll>(g->Tq), static_cast<ll>(g->D));
    return LSQ_OK;
}

int check_splits(const char* what, const lsq_attn_decode_w8_geom* g, int64_t splits) {
    const int64_t most = (g->Tk + lsq::kPgStep - 1) / lsq::kPgStep;
    if (splits < 0 || splits > most)
        return fail(LSQ_EINVAL, "%s: splits = %lld must be 0 (the library's choice) or 1 .. ceil(Tk / 64) = %lld", what, static_cast<ll>(splits),
                    static_cast<ll>(most));
    return LSQ_OK;
}

// a side of the op is a quantizer: levels out only
int check_side(const char* what, const char* name, const lsq_attn_w8_out* c, lsq::AttnOut& arg) {
    int64_t y_elem = 1;
    if (int rc = check_out(what, c, arg, y_elem)) return rc;
    if (!c->out_scale) return fail(LSQ_EINVAL, "%s: the %s side needs out_scale and out_shift (levels out only)", what, name);
    return LSQ_OK;
}

int side_off(const lsq_attn_w8_out* c) { return std::max(c->quant_max, c->type_max) > 127 ? 128 : 0; }

int check_append_geom(const char* what, const lsq_kv_append_paged_w8_geom* g) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (int rc = check_pages(what, &g->pages)) return rc;
    const int64_t lim = int64_t{1} << 29;
    if (g->B < 1 || g->T < 1 || g->Hkv < 1 || g->D < 1 || g->B > lim || g->T > lim || g->Hkv > lim || g->D > lim || g->pages.ps > lim ||
        g->pages.Mp > lim)
        return fail(LSQ_EINVAL, "%s: [B, T, Hkv, D] = [%lld, %lld, %lld, %lld] with ps = %lld and Mp = %lld, every extent must be 1 .. 2^29", what,
                    static_cast<ll>(g->B), static_cast<ll>(g->T), static_cast<ll>(g->Hkv), static_cast<ll>(g->D), static_cast<ll>(g->pages.ps),
                    static_cast<ll>(g->pages.Mp));
    int64_t elems = g->B;                                               // B T Hkv D without overflow: each factor is 2^29 at most
    for (int64_t n : {g->T, g->Hkv, g->D}) {
        if (elems > (int64_t{1} << 40) / n)
            return fail(LSQ_EINVAL, "%s: [B, T, Hkv, D] = [%lld, %lld, %lld, %lld] are more than 2^40 elements", what, static_cast<ll>(g->B),
                        static_cast<ll>(g->T), static_cast<ll>(g->Hkv), static_cast<ll>(g->D));
        elems *= n;
    }
    const int64_t st[12] = {g->k_sb, g->k_st, g->k_sh, g->v_sb, g->v_st, g->v_sh, g->kp_sp, g->kp_sh, g->kp_ss, g->vp_sp, g->vp_sh, g->vp_ss};
    for (int64_t s : st)
        if (s < 0 || s > (int64_t{1} << 40)) return fail(LSQ_EINVAL, "%s: a stride of %lld is negative or beyond 2^40", what, static_cast<ll>(s));
    if ((g->T > 1 && g->k_st < g->D) || (g->T > 1 && g->v_st < g->D) || (g->Hkv > 1 && (g->k_sh < g->D || g->v_sh < g->D)))
        return fail(LSQ_EINVAL, "%s: a source's token or head stride is smaller than its row of %lld", what, static_cast<ll>(g->D));
    if (g->kp_ss < g->D || g->vp_ss < g->D)
        return fail(LSQ_EINVAL, "%s: a pool's slot stride (%lld, %lld) is smaller than its row of %lld", what, static_cast<ll>(g->kp_ss),
                    static_cast<ll>(g->vp_ss), static_cast<ll>(g->D));
    const lsq_attn_w8_strides kp{g->kp_sp, g->kp_sh, g->kp_ss}, vp{g->vp_sp, g->vp_sh, g->vp_ss};
    if (self_overlap(kp, g->pages.Np, g->Hkv, g->pages.ps, g->D) || self_overlap(vp, g->pages.Np, g->Hkv, g->pages.ps, g->D))
        return fail(LSQ_EINVAL, "%s: pages, heads or slots of a pool overlap each other (k strides %lld, %lld, %lld; v strides %lld, %lld, "
                    "%lld for [%lld, %lld, %lld, %lld])", what, static_cast<ll>(g->kp_sp), static_cast<ll>(g->kp_sh), static_cast<ll>(g->kp_ss),
                    static_cast<ll>(g->vp_sp), static_cast<ll>(g->vp_sh), static_cast<ll>(g->vp_ss), static_cast<ll>(g->pages.Np),
                    static_cast<ll>(g->Hkv), static_cast<ll>(g->pages.ps), static_cast<ll>(g->D));
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_attn_paged_w8_abi_version(void) { return LSQ_ATTN_PAGED_W8_ABI_VERSION; }

const char* lsq_attn_paged_w8_last_error(void) { return g_last_error; }

int lsq_attn_paged_w8_workspace(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, int64_t splits, int64_t* bytes) {
    const char* what = "lsq_attn_paged_w8_workspace";
    if (int rc = check_paged_geom(what, geom, pages)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (!bytes) return fail(LSQ_EINVAL, "%s: NULL bytes", what);
    lsq_attn_decode_w8_geom dense = *geom;                              // the size does not depend on bases or strides
    dense.q = dense.k = dense.v = lsq_attn_w8_strides{0, 0, 16 * ((geom->D + 15) / 16)};
    const lsq::PgPlan pl = lsq::plan_paged(dense, *pages, true, true, splits);
    if (int rc = check_grid(what, pl.grid)) return rc;
    *bytes = pl.family == LSQ_ATTN_PAGED_W8_PAGED ? pl.ws_bytes : 0;
    return LSQ_OK;
}

int lsq_attn_paged_w8_decode(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, const lsq_attn_decode_w8_consts* consts,
                             const lsq_attn_w8_out* scores_out, const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out,
                             const void* table, const void* key_lengths, const void* block_table, const void* q_levels, const void* k_pool,
                             const void* v_pool, void* y, void* workspace, int64_t workspace_bytes, int64_t splits, void* stream) {
    const char* what = "lsq_attn_paged_w8_decode";
    lsq::AttnOut so{}, po{}, co{};
    if (int rc = check_paged_geom(what, geom, pages)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (!consts) return fail(LSQ_EINVAL, "%s: NULL constants", what);
    const void* cs[8] = {consts->s_q, consts->z_q, consts->s_k, consts->z_k, consts->s_v, consts->z_v, consts->s_p, consts->z_p};
    for (const void* c : cs) {
        if (!c) return fail(LSQ_EINVAL, "%s: NULL scale or zero point", what);
        if (!aligned_to(c, 4)) return fail(LSQ_EINVAL, "%s: the scales and zero points must be element-aligned", what);
    }
    if (int rc = check_side(what, "scores", scores_out, so)) return rc;
    if (int rc = check_side(what, "probabilities", probs_out, po)) return rc;
    if (int rc = check_side(what, "context", ctx_out, co)) return rc;
    if (scores_out->mid_dtype != probs_out->mid_dtype || scores_out->mid_dtype != ctx_out->mid_dtype)
        return fail(LSQ_EINVAL, "%s: the three sides carry one mid_dtype, got codes %lld, %lld and %lld", what,
                    static_cast<ll>(scores_out->mid_dtype), static_cast<ll>(probs_out->mid_dtype), static_cast<ll>(ctx_out->mid_dtype));
    if (!table || !q_levels || !k_pool || !v_pool || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(table, 4)) return fail(LSQ_EINVAL, "%s: the table must be element-aligned", what);
    if (!block_table) return fail(LSQ_EINVAL, "%s: NULL block table", what);
    if (!aligned_to(block_table, 4)) return fail(LSQ_EINVAL, "%s: the block table must be 4-byte aligned", what);
    if (geom->has_lengths && !key_lengths) return fail(LSQ_EINVAL, "%s: key_lengths is NULL but the geometry says has_lengths", what);
    if (!geom->has_lengths && key_lengths) return fail(LSQ_EINVAL, "%s: key_lengths is given but the geometry says has_lengths = 0", what);
    if (key_lengths && !aligned_to(key_lengths, 4)) return fail(LSQ_EINVAL, "%s: key_lengths must be 4-byte aligned", what);
    const int64_t q_span = span_of(geom->q, geom->B, geom->H, geom->Tq, geom->D), y_bytes = span_of(geom->y, geom->B, geom->H, geom->Tq, geom->D);
    const int64_t k_span = span_of(geom->k, pages->Np, geom->Hkv, pages->ps, geom->D), v_span = span_of(geom->v, pages->Np, geom->Hkv, pages->ps, geom->D);
    const int64_t bt_bytes = 4 * ((geom->B - 1) * pages->bt_ld + pages->Mp);
    if (overlap(y, y_bytes, q_levels, q_span) || overlap(y, y_bytes, k_pool, k_span) || overlap(y, y_bytes, v_pool, v_span) ||
        overlap(y, y_bytes, table, 1024) || overlap(y, y_bytes, block_table, bt_bytes) ||
        (key_lengths && overlap(y, y_bytes, key_lengths, 4 * geom->B)))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap q's %lld, the k pool's %lld, the v pool's %lld, the table, the block table or "
                    "key_lengths", what, static_cast<ll>(y_bytes), static_cast<ll>(q_span), static_cast<ll>(k_span), static_cast<ll>(v_span));
    const lsq::PgPlan pl = lsq::plan_paged(*geom, *pages, aligned_to(q_levels, 16) && aligned_to(k_pool, 16) && aligned_to(v_pool, 16),
                                           aligned_to(y, 16), splits);
    if (pl.family != LSQ_ATTN_PAGED_W8_PAGED)
        return fail(LSQ_EINVAL, "%s: [B, H, Hkv, Tq, D] = [%lld, %lld, %lld, %lld, %lld] on pages of %lld slots with these bases and strides is "
                    "not served by the paged kernels (G Tq <= %d, q and the pools 16-byte aligned with strides that are multiples of 16, "
                    "D %% 16 == 0, 16 <= D <= %d, ps a power of two >= %d): gather the pages and compose lsq_hip_attn_w8.h and "
                    "lsq_hip_attn_mask_w8.h", what, static_cast<ll>(geom->B), static_cast<ll>(geom->H), static_cast<ll>(geom->Hkv),
                    static_cast<ll>(geom->Tq), static_cast<ll>(geom->D), static_cast<ll>(pages->ps), LSQ_ATTN_PAGED_W8_MAX_ROWS,
                    LSQ_ATTN_PAGED_W8_MAX_D, LSQ_ATTN_PAGED_W8_MIN_PAGE);
    if (int rc = check_grid(what, pl.grid)) return rc;
    if (!workspace) return fail(LSQ_EINVAL, "%s: NULL workspace (%lld bytes are needed: lsq_attn_paged_w8_workspace)", what, static_cast<ll>(pl.ws_bytes));
    if (!aligned_to(workspace, 16)) return fail(LSQ_EINVAL, "%s: the workspace must be 16-byte aligned", what);
    if (workspace_bytes < pl.ws_bytes)
        return fail(LSQ_EINVAL, "%s: the workspace has %lld bytes, %lld are needed (lsq_attn_paged_w8_workspace)", what,
                    static_cast<ll>(workspace_bytes), static_cast<ll>(pl.ws_bytes));
    if (overlap(workspace, pl.ws_bytes, q_levels, q_span) || overlap(workspace, pl.ws_bytes, k_pool, k_span) ||
        overlap(workspace, pl.ws_bytes, v_pool, v_span) || overlap(workspace, pl.ws_bytes, y, y_bytes) ||
        overlap(workspace, pl.ws_bytes, table, 1024) || overlap(workspace, pl.ws_bytes, block_table, bt_bytes) ||
        (key_lengths && overlap(workspace, pl.ws_bytes, key_lengths, 4 * geom->B)))
        return fail(LSQ_EINVAL, "%s: the workspace's %lld bytes overlap q, a pool, y, the table, the block table or key_lengths", what,
                    static_cast<ll>(pl.ws_bytes));
    if (overlap(block_table, bt_bytes, k_pool, k_span) || overlap(block_table, bt_bytes, v_pool, v_span))
        return fail(LSQ_EINVAL, "%s: the block table's %lld bytes overlap a pool", what, static_cast<ll>(bt_bytes));
    const lsq::PgArg arg{static_cast<const float*>(consts->s_q), static_cast<const int32_t*>(consts->z_q),
                         static_cast<const float*>(consts->s_k), static_cast<const int32_t*>(consts->z_k),
                         static_cast<const float*>(consts->s_v), static_cast<const int32_t*>(consts->z_v),
                         static_cast<const float*>(consts->s_p), static_cast<const int32_t*>(consts->z_p),
                         geom->q_dtype == LSQ_ATTN_W8_U8 ? 128 : 0, geom->k_dtype == LSQ_ATTN_W8_U8 ? 128 : 0,
                         geom->v_dtype == LSQ_ATTN_W8_U8 ? 128 : 0, side_off(scores_out), side_off(probs_out),
                         pl.store == LSQ_ATTN_W8_STORE_PACKETS ? 1 : 0};
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    int64_t* wi = reinterpret_cast<int64_t*>(ws + pl.ws_scores);
    const dim3 grid(static_cast<unsigned>(pl.grid)), heads(static_cast<unsigned>(pl.heads)), block(lsq::kPgThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int32_t* lens = static_cast<const int32_t*>(key_lengths);
    const int32_t* bt = static_cast<const int32_t*>(block_table);
    hipLaunchKernelGGL(lsq::attn_paged_scores_kernel, grid, block, 0, st, pl.g, arg, so, lens, bt, static_cast<const uint8_t*>(q_levels),
                       static_cast<const uint8_t*>(k_pool), ws);
    if (int rc = hip_status(hipGetLastError(), what)) return rc;
    hipLaunchKernelGGL(lsq::attn_paged_context_kernel, grid, block, static_cast<size_t>(pl.lds), st, pl.g, arg, po,
                       static_cast<const int32_t*>(table), lens, bt, static_cast<const uint8_t*>(v_pool), static_cast<const uint8_t*>(ws), wi);
    if (int rc = hip_status(hipGetLastError(), what)) return rc;
    hipLaunchKernelGGL(lsq::attn_paged_reduce_kernel, heads, block, 0, st, pl.g, arg, co, lens, static_cast<const int64_t*>(wi),
                       static_cast<uint8_t*>(y));
    return hip_status(hipGetLastError(), what);
}

int lsq_attn_paged_w8_plan(const lsq_attn_decode_w8_geom* geom, const lsq_attn_paged_w8_pages* pages, int qkv_aligned, int y_aligned,
                           int64_t splits, int32_t* out8) {
    const char* what = "lsq_attn_paged_w8_plan";
    if (int rc = check_paged_geom(what, geom, pages)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::PgPlan pl = lsq::plan_paged(*geom, *pages, qkv_aligned != 0, y_aligned != 0, splits);
    if (int rc = check_grid(what, pl.grid)) return rc;
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.family == LSQ_ATTN_PAGED_W8_PAGED ? lsq::kPgThreads : 0;
    out8[3] = pl.rows;
    out8[4] = pl.chunk;
    out8[5] = pl.splits;
    out8[6] = pl.lds;
    out8[7] = pl.store;
    return LSQ_OK;
}

int lsq_kv_append_paged_w8(const lsq_kv_append_paged_w8_geom* geom, const void* block_table, const void* positions, const void* k_levels,
                           const void* v_levels, void* k_pool, void* v_pool, void* stream) {
    const char* what = "lsq_kv_append_paged_w8";
    if (int rc = check_append_geom(what, geom)) return rc;
    if (!k_levels || !v_levels || !k_pool || !v_pool) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!block_table) return fail(LSQ_EINVAL, "%s: NULL block table", what);
    if (!aligned_to(block_table, 4)) return fail(LSQ_EINVAL, "%s: the block table must be 4-byte aligned", what);
    if (positions && !aligned_to(positions, 4)) return fail(LSQ_EINVAL, "%s: positions must be 4-byte aligned", what);
    const lsq_attn_w8_strides ks{geom->k_sb, geom->k_st, geom->k_sh}, vs{geom->v_sb, geom->v_st, geom->v_sh};
    const lsq_attn_w8_strides kp{geom->kp_sp, geom->kp_sh, geom->kp_ss}, vp{geom->vp_sp, geom->vp_sh, geom->vp_ss};
    const int64_t k_span = span_of(ks, geom->B, geom->T, geom->Hkv, geom->D), v_span = span_of(vs, geom->B, geom->T, geom->Hkv, geom->D);
    const int64_t kp_span = span_of(kp, geom->pages.Np, geom->Hkv, geom->pages.ps, geom->D);
    const int64_t vp_span = span_of(vp, geom->pages.Np, geom->Hkv, geom->pages.ps, geom->D);
    const int64_t bt_bytes = 4 * ((geom->B - 1) * geom->pages.bt_ld + geom->pages.Mp);
    const void* pools[2] = {k_pool, v_pool};
    const int64_t spans[2] = {kp_span, vp_span};
    for (int i = 0; i < 2; ++i)
        if (overlap(pools[i], spans[i], k_levels, k_span) || overlap(pools[i], spans[i], v_levels, v_span) ||
            overlap(pools[i], spans[i], block_table, bt_bytes) || (positions && overlap(pools[i], spans[i], positions, 4 * geom->B)))
            return fail(LSQ_EINVAL, "%s: the %s pool's %lld bytes overlap a source, the block table or positions", what, i ? "v" : "k",
                        static_cast<ll>(spans[i]));
    if (overlap(k_pool, kp_span, v_pool, vp_span)) return fail(LSQ_EINVAL, "%s: the two pools overlap each other", what);
    const lsq::ApPlan pl = lsq::plan_append(*geom, aligned_to(k_levels, 16) && aligned_to(v_levels, 16) && aligned_to(k_pool, 16) && aligned_to(v_pool, 16));
    if (int rc = check_grid(what, pl.grid)) return rc;
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kPgThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int32_t* bt = static_cast<const int32_t*>(block_table);
    const int32_t* pos = static_cast<const int32_t*>(positions);
    const uint8_t* k = static_cast<const uint8_t*>(k_levels);
    const uint8_t* v = static_cast<const uint8_t*>(v_levels);
    if (pl.family == LSQ_ATTN_PAGED_W8_APPEND_PACKETS)
        hipLaunchKernelGGL(lsq::kv_append_paged_kernel<true>, grid, block, 0, st, pl.g, bt, pos, k, v, static_cast<uint8_t*>(k_pool), static_cast<uint8_t*>(v_pool));
    else
        hipLaunchKernelGGL(lsq::kv_append_paged_kernel<false>, grid, block, 0, st, pl.g, bt, pos, k, v, static_cast<uint8_t*>(k_pool), static_cast<uint8_t*>(v_pool));
    return hip_status(hipGetLastError(), what);
}

int lsq_kv_append_paged_w8_plan(const lsq_kv_append_paged_w8_geom* geom, int aligned, int32_t* out8) {
    const char* what = "lsq_kv_append_paged_w8_plan";
    if (int rc = check_append_geom(what, geom)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::ApPlan pl = lsq::plan_append(*geom, aligned != 0);
    if (int rc = check_grid(what, pl.grid)) return rc;
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = lsq::kPgThreads;
    out8[3] = pl.units;
    out8[4] = out8[5] = out8[6] = 0;
    out8[7] = pl.family;
    return LSQ_OK;
}

}  // extern "C"
