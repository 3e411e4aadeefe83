// lsq_attn_split_core.hpp -- split-key decode attention on 8-bit levels on gfx950, ONCE: the bodies of the three launches, their tile
// and LDS constants, the chunk rule, the plan and the launch sequence, for liblsq_hip_attn_decode_split_w8.so (keys in a dense
// cache) and liblsq_hip_attn_paged_w8.so (keys in the pages of a pool).  The constants are the LSQ_ATTN_DECODE_SPLIT_W8_* macros of
// include/lsq_hip_attn_decode_split_w8.h; the paged translation unit asserts that its header's twins are equal.
//
// The definition, the row tile and the arithmetic are those of ../attn_decode_w8/lsq_attn_decode_w8.hip -- the R = G Tq <= 16 query
// rows that read one kv head are ONE 16-row tile of the matrix core, row r = g Tq + t being q[b, hkv G + g, t] -- but a (b, kv head)
// is dealt to S workgroups by chunks of C keys, C a multiple of 64.  Workgroup (bh, s) of launches 1 and 2 owns the keys
// [c0, c1) = [s C, min((s + 1) C, nmax)), nmax = n(b, Tq - 1) being uniform over the S workgroups of a head; where c0 >= nmax it
// returns before its first barrier.  All three kernels run 256 threads = 4 waves.
//  1 split_scores   phase 1 of the decode kernel on the chunk, 256 keys a round: wave w takes the 16-key sub-tiles 4 w .. 4 w + 3 of
//                   the round, all four k packets in flight, k's rows the MFMA B operand straight from memory
//                   (v_mfma_i32_16x16x64_i8), sum q and sum k from the all-ones MFMAs, the decode kernel's epilogue; the score byte
//                   goes into LDS [16][272] and leaves as 16-byte packets of the rows < R for the workspace [B Hkv][R][ldw].  Keys
//                   beyond c1 are clamped to c1 - 1: their bytes fill the tail of the chunk's last packet and are never counted.
//                   A packet belongs to ONE workgroup (c0 is a multiple of 64) and packets at or beyond 16 ceil(nmax / 16) are
//                   neither written nor, in launch 2, read.
//  2 split_context  wave w takes the rows w, w + 4, .. < R: the byte maximum and S over the row's WHOLE prefix n_r, phase 2 of the
//                   decode kernel reading the workspace (cache-served; the same for every split of the head: an exact integer) ->
//                   m, 1 / float(S) and n_r of the 16 rows in LDS.  Then the chunk in 64-key steps, double buffered, one barrier a
//                   step: thread (r, w) = (tid / 16, tid % 16) turns the score word of the keys k0 + 4 w .. + 3 of row r -- loaded one
//                   step ahead -- into four probability bytes (the byte z_p from n_r on, the operand's zero from c1 on and in rows
//                   >= R) in the p tile [16][80]; v's 64 rows are staged transposed into [D][80] as in the decode kernel; the D / 16
//                   accumulator sub-tiles are dealt to the waves.  The chunk's exact integer
//                       I_c = P - z_p C - z_v S + (c1 - c0) z_p z_v        (bmm_exact: 64 bits)
//                   of the rows < R goes to the workspace [B Hkv][S][R][D] as int64.
//  3 split_reduce   one workgroup per (b, kv head): I = sum of I_c over the ceil(nmax / C) chunks that start below nmax, float(I),
//                   the decode kernel's epilogue and store.  nmax = 0: no chunk is read, I = 0.
// No atomics, no flags: the stream orders the three launches.
//
// ROW TILES (liblsq_hip_attn_chunk_w8.so: any R).  The bodies are templates over `kTiled`.  false, the default and what the two decode
// libraries instantiate, is everything above: one tile, row0 = 0, and every line below that names row0 folds to the text without
// it.  true deals the R rows of a kv head to NT = ceil(R / 16) tiles of 16 and makes the tile a grid coordinate: launches 1 and 2
// run B Hkv NT S workgroups ((b, kv head), tile, split -- the split innermost), launch 3 B Hkv NT.  Tile i holds the rows
// row0 = 16 i .. min(row0 + 15, R - 1) and may straddle two query heads (Tq % 16 != 0).  In place of nmax stands the TILE's
//     nmax_tile = the largest n of the tile's live rows = n(b, Tq - 1) where the tile straddles a head border, else n of its last row
// (n is non-decreasing in t in all three mask modes): a workgroup whose chunk starts at or beyond nmax_tile returns before its first
// barrier -- the early tiles of a causal prompt skip the late chunks --, launch 2 reads a row's prefix below 16 ceil(n_r / 16) <=
// 16 ceil(nmax_tile / 16), which the same tile's launch-1 workgroups wrote, and launch 3 sums the chunks that start below nmax_tile.
// A row with n_r below a processed chunk carries the byte z_p there and contributes exactly 0.  kTiled also knows the third mask
// mode (g.causal == 2: n(b, t) = max(0, L_b - (Tq - 1 - t)), L_b = min(Tk, max(key_lengths[b], 0))).
//
// WHERE A KEY'S ROW LIES is the one thing the two libraries do not share: launches 1 and 2 are templates over a key-addressing
// policy `Keys`, a kernel argument.  A policy provides
//     Keys::Rows keys.rows(T, s, b, hkv)       the rows of head (b, hkv) of the tensor T with the strides s = (s0, s1, ld), with
//     Rows::Entry                              what a lane keeps of the table entry that serves some keys (DenseKeys: nothing),
//     Entry rows.entry(j)                      the entry of key j: a load WITHOUT a branch (a guarded load is waited for at once),
//     const uint8_t* rows.row(e, j)            the row of key j, which e serves, and
//     int64_t rows.ld                          the bytes from that row to the next one e serves.
// The bodies ask for entries early and keep them in registers, so that no packet load waits for a table: launch 1 holds the
// entries of a wave's four sub-tiles BEFORE the round's k packets are issued and issues the next round's four behind those packets
// (first used after this round's MFMAs); launch 2 loads v's rows one step ahead and their entries two steps ahead, in front of
// those rows' loads, so that they complete under the first row's wait.  An index at or beyond the chunk's end is clamped to the
// chunk's last sub-tile or key, so only entries of keys below c1 <= nmax are asked for.  The 16 keys of a sub-tile (and the clamped
// last key c1 - 1, which lies in the sub-tile that holds 16 j < c1) and the 4 keys of a v group share one entry: a policy's entry
// serves aligned runs of at least 16 keys.  With DenseKeys all of this folds away: its kernels are the ones written without it.
//
// Include after lsq_companion_abi.hpp and ../attn_w8/lsq_attn_decode_checks.hpp (the host half uses their fail and strides16).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../qlinear_w8/lsq_w8_shared.hpp"
#include "../attn_w8/lsq_attn_w8_dev.hpp"
#include "../attn_w8/lsq_attn_decode_checks.hpp"
#include "../../../include/lsq_hip_attn_decode_split_w8.h"

namespace lsq {

typedef __attribute__((ext_vector_type(2))) unsigned short spl_u16x2;

constexpr int kSplRows = LSQ_ATTN_DECODE_SPLIT_W8_MAX_ROWS;     // the row tile of the matrix core
constexpr int kSplThreads = LSQ_ATTN_DECODE_SPLIT_W8_THREADS;
constexpr int kSplWaves = kSplThreads / 64;
constexpr int kSplStep = 64;                                    // keys per step of launch 2, and what a chunk is a multiple of
constexpr int kSplTStride = kSplStep + 16;                      // bytes between the rows of a p tile or a transposed v tile in LDS
constexpr int kSplInFlight = 4;                                 // 16-key sub-tiles of k a wave loads before it multiplies
constexpr int kSplRound = 16 * kSplInFlight * kSplWaves;        // keys a workgroup scores between two barriers: 256
constexpr int kSplScoreLd = kSplRound + 16;                     // bytes between the score rows of a round in LDS
constexpr int kSplSubsPerWave = 2;                              // D / 16 <= 8 accumulator sub-tiles over four waves
constexpr int kSplTable = 1024;
constexpr int kSplRowInfo = 256;                                // m, 1 / S and n of the 16 rows
constexpr int kSplScoreLds = kSplRows * kSplScoreLd;
constexpr int spl_context_lds(int D) { return kSplTable + kSplRowInfo + 2 * kSplRows * kSplTStride + 2 * kSplTStride * D; }
static_assert(kSplSubsPerWave * kSplWaves * 16 >= LSQ_ATTN_DECODE_SPLIT_W8_MAX_D, "four waves cover every sub-tile of D");
static_assert(kSplRows * 16 == kSplThreads, "one thread per (row, word) of a p tile and per (row, packet) of a round");
static_assert(spl_context_lds(LSQ_ATTN_DECODE_SPLIT_W8_MAX_D) <= 65536 && kSplScoreLds <= 65536, "no launch asks for more LDS than a kernel gets unasked");

struct SplGeom {            // kernel argument
    int64_t q_s0, q_s1, q_ld;
    lsq_attn_w8_strides k, v;   // as the policy reads them
    int64_t y_s0, y_s1, y_ld;
    int64_t ldw;            // bytes between the score rows in the workspace, a multiple of 16 that is at least Tk
    int Hkv, G, Tq, Tk, D;
    int R;                  // G Tq
    int causal, off;        // 1: row t sees t + 1 + off keys (off clamped to Tk on the host); 2 (kTiled only): counted back from the length
    int chunk, S;           // keys of a chunk (a multiple of 64); ceil(Tk / chunk)
};

struct SplArg {             // kernel argument
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

// keys in a dense cache: row(b, hkv, j) = T + b s0 + hkv s1 + j ld.  No table, no per-lane state
struct DenseKeys {          // kernel argument
    struct Rows {
        struct Entry {};
        const uint8_t* __restrict__ base;
        int64_t ld;
        __device__ __forceinline__ Entry entry(int) const { return Entry{}; }
        __device__ __forceinline__ const uint8_t* row(Entry, int j) const { return base + static_cast<int64_t>(j) * ld; }
    };
    __device__ __forceinline__ Rows rows(const uint8_t* __restrict__ T, const lsq_attn_w8_strides& s, int64_t b, int64_t hkv) const {
        return Rows{T + b * s.s0 + hkv * s.s1, s.ld};
    }
};

// n(b, t) of the contract; len: max(key_lengths[b], 0), or Tk without lengths
template <bool kTiled = false>
__device__ __forceinline__ int spl_count(const SplGeom& g, int len, int t) {
    int n = min(g.Tk, len);
    if (kTiled && g.causal == 2) return max(n - (g.Tq - 1 - t), 0);    // the last row sees L_b keys, the row before it one fewer
    if (g.causal) n = min(n, t + 1 + g.off);           // t < Tq <= 2^20 and off <= Tk <= 65536
    return n;
}

// the row tile of a workgroup.  `bh` comes in as the workgroup's index without its split, ((b, kv head), tile), and leaves as
// (b, kv head); the tile's first row is returned.  !kTiled: one tile, nothing is touched
template <bool kTiled>
__device__ __forceinline__ int spl_tile(const SplGeom& g, int64_t& bh) {
    if constexpr (kTiled) {
        const int NT = (g.R + kSplRows - 1) / kSplRows;
        const int64_t bt = bh;
        bh = bt / NT;
        return kSplRows * static_cast<int>(bt - bh * NT);
    } else {
        return 0;
    }
}

// R D, the integers of one chunk of a kv head: at most 2048 with one tile, beyond an int with row tiles
template <bool kTiled>
__device__ __forceinline__ auto spl_chunk_stride(const SplGeom& g) {
    if constexpr (kTiled) {
        return static_cast<int64_t>(g.R) * g.D;
    } else {
        return g.R * g.D;
    }
}

// the largest n among the rows of the tile that starts at row0: where the workgroup's key loops end
template <bool kTiled>
__device__ __forceinline__ int spl_nmax(const SplGeom& g, int len, int row0) {
    if constexpr (kTiled) {
        const int last = min(row0 + kSplRows, g.R) - 1;                 // the tile's last live row
        const int h0 = row0 / g.Tq, h1 = last / g.Tq;
        return spl_count<true>(g, len, h0 != h1 ? g.Tq - 1 : last - h1 * g.Tq);    // a straddled border: the row t = Tq - 1 is in the tile
    } else {
        return spl_count(g, len, g.Tq - 1);
    }
}

// ------------------------------------------------------------------------------------------------ launch 1: the scores of a chunk
template <class Keys, bool kTiled = false>
__device__ __forceinline__ void attn_split_scores(const SplGeom& g, const SplArg& a, const AttnOut& so, const int32_t* __restrict__ lens,
                                                  const uint8_t* __restrict__ Q, const uint8_t* __restrict__ K, uint8_t* __restrict__ ws,
                                                  const Keys& keys) {
    __shared__ __attribute__((aligned(16))) unsigned char sc[kSplScoreLds];      // [16][272]: the score bytes of a round
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    int64_t bh = static_cast<int64_t>(blockIdx.x) / g.S;
    const int s = static_cast<int>(static_cast<int64_t>(blockIdx.x) - bh * g.S);
    const int row0 = spl_tile<kTiled>(g, bh);
    const int64_t b0 = bh / g.Hkv, b1 = bh - b0 * g.Hkv;
    const int len = lens ? max(lens[b0], 0) : g.Tk;
    const int nmax = spl_nmax<kTiled>(g, len, row0);                    // 0 .. Tk, the same for the S workgroups of the head (kTiled: of the tile)
    const int c0 = s * g.chunk;                                         // s chunk < Tk + chunk: no overflow
    if (c0 >= nmax) return;                                             // the same for the whole workgroup, before any barrier
    const int c1 = min(c0 + g.chunk, nmax);
    const int jend = (c1 + 15) >> 4;                                    // 16-key sub-tiles below c1
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const uint32_t flip_q = a.off_q ? 0x80808080u : 0u, flip_k = a.off_k ? 0x80808080u : 0u;
    const int r = min(row0 + nl, g.R - 1);                              // a clamped row computes values nobody stores
    const int rg = r / g.Tq, rt = r - rg * g.Tq;
    const uint8_t* __restrict__ qrow = Q + b0 * g.q_s0 + (b1 * g.G + rg) * g.q_s1 + static_cast<int64_t>(rt) * g.q_ld;
    const typename Keys::Rows krows = keys.rows(K, g.k, b0, b1);
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
    uint8_t* __restrict__ wrow = ws + (bh * g.R + row0 + (tid >> 4)) * g.ldw;       // the row this thread copies out (used where it is < R)
    // the entries of this wave's sub-tiles of the round, all four in flight at once: a sub-tile at or beyond jend takes the entry of
    // the chunk's last one (16 (jend - 1) < c1 <= nmax: a live key) and is never used
    typename Keys::Rows::Entry ent[kSplInFlight];
#pragma unroll
    for (int u = 0; u < kSplInFlight; ++u) ent[u] = krows.entry(16 * min((c0 >> 4) + wave * kSplInFlight + u, jend - 1));
    for (int jb = c0 >> 4; jb < jend; jb += kSplRound / 16) {           // the same for the whole workgroup
        const int j0 = jb + wave * kSplInFlight;
        u32x4 kv[kSplInFlight][2];
#pragma unroll
        for (int u = 0; u < kSplInFlight; ++u) {
            kv[u][0] = u32x4{0u, 0u, 0u, 0u};
            kv[u][1] = u32x4{0u, 0u, 0u, 0u};
            if (j0 + u < jend) {
                // 16 (j0 + u) < c1: the clamped key is a key of the chunk, in this sub-tile and so served by its entry
                const uint8_t* __restrict__ kr = krows.row(ent[u], min(16 * (j0 + u) + nl, c1 - 1));
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int kk = 64 * h + 16 * q;
                    if (kk < g.D) kv[u][h] = *reinterpret_cast<const u32x4*>(kr + kk) ^ flip_k;        // a packet beyond D: the operand's zero
                }
            }
        }
        typename Keys::Rows::Entry nxt[kSplInFlight];                         // the next round's entries, in flight behind the packets
#pragma unroll
        for (int u = 0; u < kSplInFlight; ++u) nxt[u] = krows.entry(16 * min(j0 + kSplRound / 16 + u, jend - 1));
#pragma unroll
        for (int u = 0; u < kSplInFlight; ++u) {
            asm volatile("" : "+v"(kv[u][0]));                          // all in flight at once
            asm volatile("" : "+v"(kv[u][1]));
        }
#pragma unroll
        for (int u = 0; u < kSplInFlight; ++u) {
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
                sc[(4 * q + i) * kSplScoreLd + 16 * (j - jb) + nl] = static_cast<unsigned char>(w8o_byte(uu, sq));
            }
        }
#pragma unroll
        for (int u = 0; u < kSplInFlight; ++u) ent[u] = nxt[u];
        __syncthreads();                                                // the round's scores are in LDS
        {
            const int pr = tid >> 4, pk = tid & 15;                     // (row, packet of the round)
            // 16 (jb + pk) + 16 <= 16 jend <= 16 ceil(Tk / 16) <= ldw
            if (row0 + pr < g.R && jb + pk < jend)
                *reinterpret_cast<u32x4*>(wrow + 16 * static_cast<int64_t>(jb + pk)) = *reinterpret_cast<const u32x4*>(sc + pr * kSplScoreLd + 16 * pk);
        }
        __syncthreads();                                                // before the next round overwrites them
    }
}

// ------------------------------------------------------------------------------------------------ launch 2: the chunk's context integer
template <class Keys, bool kTiled = false>
__device__ __forceinline__ void attn_split_context(const SplGeom& g, const SplArg& a, const AttnOut& po, const int32_t* __restrict__ table,
                                                   const int32_t* __restrict__ lens, const uint8_t* __restrict__ V,
                                                   const uint8_t* __restrict__ ws, int64_t* __restrict__ wi, const Keys& keys) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int32_t* tab = reinterpret_cast<int32_t*>(lds);                                 // [256]
    int* row_m = reinterpret_cast<int*>(lds + kSplTable);                           // [16] the biased byte maximum
    float* row_r = reinterpret_cast<float*>(lds + kSplTable + 64);                  // [16] 1 / float(S), 0 where n = 0
    int* row_n = reinterpret_cast<int*>(lds + kSplTable + 128);                     // [16] n_r, 0 in rows >= R
    unsigned char* ptile = lds + kSplTable + kSplRowInfo;                           // 2 x [16][80]: p bytes, the operand's sign flip applied
    unsigned char* stage = ptile + 2 * kSplRows * kSplTStride;                      // 2 x [D][80]: v transposed
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    int64_t bh = static_cast<int64_t>(blockIdx.x) / g.S;
    const int s = static_cast<int>(static_cast<int64_t>(blockIdx.x) - bh * g.S);
    const int row0 = spl_tile<kTiled>(g, bh);
    const int64_t b0 = bh / g.Hkv, b1 = bh - b0 * g.Hkv;
    const int len = lens ? max(lens[b0], 0) : g.Tk;
    const int nmax = spl_nmax<kTiled>(g, len, row0);
    const int c0 = s * g.chunk;
    if (c0 >= nmax) return;                                             // the same for the whole workgroup, before any barrier
    const int c1 = min(c0 + g.chunk, nmax);
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const uint32_t flip_s = a.off_s ? 0u : 0x80808080u;                 // int8 levels are biased by 128 on load
    const uint8_t* __restrict__ wsb = ws + bh * g.R * g.ldw;            // the head's score rows [R][ldw]

    tab[tid] = table[tid];                                              // 256 threads
    __syncthreads();

    // ---- the tile's rows' maximum and sum over their WHOLE prefix: packets below 16 ceil(n_r / 16) <= 16 ceil(nmax / 16), all written
    for (int r = wave; r < kSplRows; r += kSplWaves) {                  // the same for the whole wave
        int n = 0, m = 0;
        float rcp = 0.0f;
        if (row0 + r < g.R) {
            const uint8_t* __restrict__ row = wsb + (row0 + r) * g.ldw;
            n = spl_count<kTiled>(g, len, (row0 + r) % g.Tq);           // n <= nmax
            const int npk = (n + 15) >> 4;
            spl_u16x2 me = {0, 0}, mo = {0, 0};
            for (int p = lane; p < npk; p += 64) {
                // bytes beyond n count as 0, the least biased byte
                const u32x4 v = attn_mask_tail(*reinterpret_cast<const u32x4*>(row + 16 * p) ^ flip_s, n - 16 * p);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    me = __builtin_elementwise_max(me, __builtin_bit_cast(spl_u16x2, v[i] & 0x00ff00ffu));
                    mo = __builtin_elementwise_max(mo, __builtin_bit_cast(spl_u16x2, (v[i] >> 8) & 0x00ff00ffu));
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
    const uint8_t* __restrict__ srow = wsb + min(row0 + pr, g.R - 1) * g.ldw;       // read only where a key lies below my_n (0 in rows >= R)
    const typename Keys::Rows vrows = keys.rows(V, g.v, b0, b1);
    const int subs = g.D >> 4;                                          // 16-column sub-tiles of the context, 1 .. 8
    const int wpr = g.D >> 2, items = 16 * wpr;                         // words of a v row; (four keys, a word) items of a step
    i32x4 P[kSplSubsPerWave], Cs[kSplSubsPerWave], Rs = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < kSplSubsPerWave; ++j) {
        P[j] = i32x4{0, 0, 0, 0};
        Cs[j] = i32x4{0, 0, 0, 0};
    }
    int kgs[2], ds[2];                                                  // this thread's two items: the group of four keys and the word
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = tid + it * kSplThreads;
        kgs[it] = idx / wpr;
        ds[it] = idx - kgs[it] * wpr;
    }
    uint32_t vr[2][4];                                                  // the rows of the step to be staged next
    uint32_t sw = 0u;                                                   // the score word of the step to be staged next
    typename Keys::Rows::Entry ent[2];                                        // the entries of the items of the step to be LOADED next
    typename Keys::Rows::Entry nxt[2];                                        // ... and of the step after it, issued AHEAD of the rows' loads
    // the entries of the items' groups in the step that starts at key kb: a group at or beyond c1 takes the entry of the key c1 - 1
    // (a key of the chunk, below nmax: a live key), from which no row is loaded
    auto entries = [&](typename Keys::Rows::Entry (&to)[2], int kb) {
#pragma unroll
        for (int it = 0; it < 2; ++it) to[it] = vrows.entry(min(kb + 4 * kgs[it], c1 - 1));
    };
    // the rows of the step that starts at key kb, served by `ent`: the four keys of a group share the entry
    auto rows = [&](int kb) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int kf = kb + 4 * kgs[it];
            const uint8_t* __restrict__ vp = vrows.row(ent[it], kf) + 4 * ds[it];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                vr[it][i] = 0u;                                         // a row beyond c1: the operand's zero
                if (tid + it * kSplThreads < items && kf + i < c1)
                    vr[it][i] = *reinterpret_cast<const uint32_t*>(vp + static_cast<int64_t>(i) * vrows.ld) ^ flip_v;
            }
        }
    };
    entries(ent, c0);
    entries(nxt, c0 + kSplStep);
    rows(c0);
    ent[0] = nxt[0];
    ent[1] = nxt[1];
    if (c0 + 4 * pw < my_n) sw = *reinterpret_cast<const uint32_t*>(srow + c0 + 4 * pw) ^ flip_s;       // my_n <= nmax: a written packet
    int buf = 0;
    for (int k0 = c0; k0 < c1; k0 += kSplStep) {                        // the same for the whole workgroup
        unsigned char* st = stage + buf * (kSplTStride * g.D);
        unsigned char* pt = ptile + buf * (kSplRows * kSplTStride);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            if (tid + it * kSplThreads < items) {
                uint32_t c[4];
                attn_transpose4(vr[it][0], vr[it][1], vr[it][2], vr[it][3], c);
#pragma unroll
                for (int i = 0; i < 4; ++i) *reinterpret_cast<uint32_t*>(st + (4 * ds[it] + i) * kSplTStride + 4 * kgs[it]) = c[i];
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
                } else if (row0 + pr < g.R && key + i < c1) {
                    byte = zb ^ fb;                                     // the byte z_p in [n_r, c1): contributes (z_p - z_p) = 0
                }
                w |= (byte & 0xffu) << (8 * i);
            }
            *reinterpret_cast<uint32_t*>(pt + pr * kSplTStride + 4 * pw) = w;
        }
        if (k0 + kSplStep < c1) {                                       // the next step's rows are loaded during this one's staging,
            entries(nxt, k0 + 2 * kSplStep);                            // the entries of the step after it issued ahead of them,
            rows(k0 + kSplStep);                                        // from entries fetched a step ago
            ent[0] = nxt[0];
            ent[1] = nxt[1];
            sw = 0u;
            if (k0 + kSplStep + 4 * pw < my_n) sw = *reinterpret_cast<const uint32_t*>(srow + k0 + kSplStep + 4 * pw) ^ flip_s;
        }
        // this step's tiles are staged; the other buffers were last read before the previous step's barrier
        __syncthreads();
        const i32x4 ai = w8_as_i32(*reinterpret_cast<const u32x4*>(pt + nl * kSplTStride + q * 16));
#pragma unroll
        for (int jj = 0; jj < kSplSubsPerWave; ++jj) {
            const int j = wave + jj * kSplWaves;
            if (j < subs) {                                             // the same for the whole wave
                const i32x4 bi = w8_as_i32(*reinterpret_cast<const u32x4*>(st + (16 * j + nl) * kSplTStride + q * 16));
                P[jj] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ai, bi, P[jj], 0, 0, 0);
                Cs[jj] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bi, Cs[jj], 0, 0, 0);
            }
        }
        Rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ai, ones, Rs, 0, 0, 0);
        buf ^= 1;
    }

    // ---- the chunk's exact integer of the rows < R: |raw sums| <= 65536 * 128 * 128 = 2^30, I_c in 64 bits
    const int64_t z_p = static_cast<int64_t>(a.z_p[0]) - a.off_p, z_v = static_cast<int64_t>(a.z_v[0]) - a.off_v;
    int64_t* __restrict__ out = wi + ((bh * g.S + s) * g.R) * g.D;      // [R][D]
#pragma unroll
    for (int jj = 0; jj < kSplSubsPerWave; ++jj) {
        const int j = wave + jj * kSplWaves;
        if (j >= subs) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * q + i;                                    // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
            if (row0 + r < g.R) out[static_cast<int64_t>(row0 + r) * g.D + 16 * j + nl] = bmm_exact(P[jj][i], Cs[jj][i], Rs[i], c1 - c0, z_p, z_v);
        }
    }
}

// ------------------------------------------------------------------------------------------------ launch 3: the sum over the chunks, the levels
template <bool kTiled = false>
__device__ __forceinline__ void attn_split_reduce(const SplGeom& g, const SplArg& a, const AttnOut& co, const int32_t* __restrict__ lens,
                                                  const int64_t* __restrict__ wi, uint8_t* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[kSplRows * LSQ_ATTN_DECODE_SPLIT_W8_MAX_D];      // the level tile [R][D]
    const int tid = static_cast<int>(threadIdx.x);
    int64_t bh = static_cast<int64_t>(blockIdx.x);
    const int row0 = spl_tile<kTiled>(g, bh);
    const int64_t b0 = bh / g.Hkv, b1 = bh - b0 * g.Hkv;
    const int len = lens ? max(lens[b0], 0) : g.Tk;
    const int nmax = spl_nmax<kTiled>(g, len, row0);
    const int live = (nmax + g.chunk - 1) / g.chunk;                    // the chunks that start below nmax: the ones launch 2 wrote; <= S
    const AttnQ oq = attn_constants(co);
    const float s_p = a.s_p[0], s_v = a.s_v[0];
    const auto RD = spl_chunk_stride<kTiled>(g);                        // the integers between two chunks
    int rows, TD;                                                       // the tile's live rows and their integers, <= 2048
    if constexpr (kTiled) {
        rows = min(kSplRows, g.R - row0);
        TD = rows * g.D;
    } else {
        rows = g.R;
        TD = RD;
    }
    const int64_t* __restrict__ src = wi + bh * g.S * RD + static_cast<int64_t>(row0) * g.D;    // [S][R][D], from the tile's first row
    for (int e = tid; e < TD; e += kSplThreads) {
        int64_t I = 0;
        for (int c = 0; c < live; ++c) I += src[static_cast<int64_t>(c) * RD + e];
        const float u = bmm_value(static_cast<float>(I), s_p, s_v, oq.mid);
        tile[e] = static_cast<unsigned char>(w8o_byte(u, oq));
    }
    __syncthreads();
    uint8_t* __restrict__ yb = y + b0 * g.y_s0 + (b1 * g.G) * g.y_s1;
    // 16-byte packets of the rows that exist (one tile: g.R by its name, which keeps the decode libraries' code objects the bytes they were)
    const int subs = g.D >> 4, total = (kTiled ? rows : g.R) * subs;
    for (int idx = tid; idx < total; idx += kSplThreads) {
        const int lr = idx / subs, c = (idx - lr * subs) * 16, r = row0 + lr;
        const int rg = r / g.Tq, rt = r - rg * g.Tq;
        uint8_t* dst = yb + rg * g.y_s1 + static_cast<int64_t>(rt) * g.y_ld + c;
        const unsigned char* from = tile + lr * g.D + c;
        if (a.y_packets) {
            *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(from);
        } else {
            for (int i = 0; i < 16; ++i) dst[i] = from[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launches
// ------------------------------------------------------------------------------------------------
struct SplPlan {
    bool served;
    int rows, tiles, chunk, splits, lds, store;
    // B Hkv NT S; B Hkv NT (launch 3's grid); the workspace's row stride, its score part and its size
    int64_t grid, heads, ldw, ws_scores, ws_bytes;
    SplGeom g;
};

// what differs between the libraries' plans: whether the rows are dealt to tiles (else R <= 16 is asked for), and the constants of
// the library's own choice of the chunk (splits = 0); max_chunk 0: no upper bound
struct SplRule {
    bool tiled;
    int64_t want, max_splits, min_chunk, max_chunk;
};
constexpr SplRule kSplDecodeRule = {false, static_cast<int64_t>(LSQ_ATTN_DECODE_SPLIT_W8_WG_PER_CU) * LSQ_ATTN_DECODE_SPLIT_W8_CUS,
                                    LSQ_ATTN_DECODE_SPLIT_W8_MAX_SPLITS, LSQ_ATTN_DECODE_SPLIT_W8_MIN_CHUNK, LSQ_ATTN_DECODE_SPLIT_W8_MAX_CHUNK};

// the chunk for `splits` (0: the library's own choice; else at most that many splits), a multiple of 64; `heads`: the workgroups
// of a launch before the keys are split, B Hkv NT
inline int64_t split_chunk(int64_t heads, int64_t Tk, int64_t splits, const SplRule& rule) {
    const int64_t units = (Tk + kSplStep - 1) / kSplStep;
    if (splits > 0) return kSplStep * ((units + splits - 1) / splits);
    // the fewest splits with which the grid fills the part, dealt evenly; the chunk taken into its range
    const int64_t fewest = std::min<int64_t>((rule.want + heads - 1) / heads, rule.max_splits);
    const int64_t chunk = std::max<int64_t>(kSplStep * ((units + fewest - 1) / fewest), rule.min_chunk);
    return rule.max_chunk ? std::min<int64_t>(chunk, rule.max_chunk) : chunk;
}

// what the libraries ask of a geometry (each adds its own limit: Tk there, the page size here) and plan the same way; `ldw` is
// the library's: a multiple of 16 that is at least Tk
inline SplPlan plan_split_core(const lsq_attn_decode_w8_geom& ge, bool qkv_aligned, bool y_aligned, int64_t splits, int64_t ldw,
                               const SplRule& rule = kSplDecodeRule) {
    SplPlan pl = {};
    const int64_t G = ge.H / ge.Hkv, R = G * ge.Tq;                     // R <= 2^40: check_decode_geom
    pl.served = qkv_aligned && strides16(ge.q) && strides16(ge.k) && strides16(ge.v) && ge.D % 16 == 0 && ge.D >= 16 &&
                ge.D <= LSQ_ATTN_DECODE_SPLIT_W8_MAX_D && ge.Tk <= LSQ_ATTN_DECODE_SPLIT_W8_MAX_TK &&
                (rule.tiled || R <= LSQ_ATTN_DECODE_SPLIT_W8_MAX_ROWS);
    if (!pl.served) return pl;
    const int Tk = static_cast<int>(ge.Tk), D = static_cast<int>(ge.D);
    const int64_t tiles = (R + kSplRows - 1) / kSplRows;
    pl.heads = ge.B * ge.Hkv * tiles;                                   // <= 2^40
    pl.chunk = static_cast<int>(split_chunk(pl.heads, ge.Tk, splits, rule));
    pl.splits = (Tk + pl.chunk - 1) / pl.chunk;                         // <= 1024
    // (a grid beyond 2^24 - 1 workgroups is refused by every entry before these two are used: R < 2^28 where a plan is launched)
    pl.rows = static_cast<int>(std::min<int64_t>(R, INT32_MAX));
    pl.tiles = static_cast<int>(std::min<int64_t>(tiles, INT32_MAX));
    pl.lds = spl_context_lds(D);
    pl.store = y_aligned && strides16(ge.y) ? LSQ_ATTN_W8_STORE_PACKETS : LSQ_ATTN_W8_STORE_ELEMS;
    pl.grid = pl.heads * pl.splits;
    pl.ldw = ldw;
    pl.ws_scores = ge.B * ge.Hkv * R * pl.ldw;                          // a multiple of 16: the integers behind it are aligned; <= 2^56
    pl.ws_bytes = pl.ws_scores + 8 * ge.B * ge.Hkv * pl.splits * R * ge.D;
    const int mode = !ge.causal ? 0 : rule.tiled && ge.causal == 2 ? 2 : 1;
    pl.g = SplGeom{ge.q.s0, ge.q.s1, ge.q.ld, ge.k, ge.v, ge.y.s0, ge.y.s1, ge.y.ld, pl.ldw,
                   static_cast<int>(ge.Hkv), static_cast<int>(G), static_cast<int>(ge.Tq), Tk, D, pl.rows, mode,
                   mode == 1 ? static_cast<int>(std::min<int64_t>(ge.causal_offset, ge.Tk)) : 0, pl.chunk, pl.splits};
    return pl;
}

// what a `*_plan` entry of the two decode libraries reports of a plan; `family`: the library's code for it (its composition code where !pl.served: all else 0)
inline void split_plan_out(const SplPlan& pl, int family, int32_t* out8) {
    out8[0] = family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.served ? kSplThreads : 0;
    out8[3] = pl.rows;
    out8[4] = pl.chunk;
    out8[5] = pl.splits;
    out8[6] = pl.lds;
    out8[7] = pl.store;
}

}  // namespace lsq

namespace {

int check_splits(const char* what, const lsq_attn_decode_w8_geom* g, int64_t splits) {
    const int64_t most = (g->Tk + lsq::kSplStep - 1) / lsq::kSplStep;
    if (splits < 0 || splits > most)
        return fail(LSQ_EINVAL, "%s: splits = %lld must be 0 (the library's choice) or 1 .. ceil(Tk / 64) = %lld", what, static_cast<ll>(splits),
                    static_cast<ll>(most));
    return LSQ_OK;
}

// the three launches of a served plan on `stream`; the kernels are the library's own instantiations of the bodies above
template <auto scores, auto context, auto reduce, class Keys>
int split_launch(const char* what, const lsq::SplPlan& pl, const lsq_attn_decode_w8_geom* geom, const lsq_attn_decode_w8_consts* consts,
                 const lsq_attn_w8_out* scores_out, const lsq_attn_w8_out* probs_out, const lsq::AttnOut& so, const lsq::AttnOut& po,
                 const lsq::AttnOut& co, const void* table, const void* key_lengths, const void* q_levels, const void* k_levels,
                 const void* v_levels, void* y, void* workspace, void* stream, const Keys& keys) {
    const lsq::SplArg arg{static_cast<const float*>(consts->s_q), static_cast<const int32_t*>(consts->z_q),
                          static_cast<const float*>(consts->s_k), static_cast<const int32_t*>(consts->z_k),
                          static_cast<const float*>(consts->s_v), static_cast<const int32_t*>(consts->z_v),
                          static_cast<const float*>(consts->s_p), static_cast<const int32_t*>(consts->z_p),
                          geom->q_dtype == LSQ_ATTN_W8_U8 ? 128 : 0, geom->k_dtype == LSQ_ATTN_W8_U8 ? 128 : 0,
                          geom->v_dtype == LSQ_ATTN_W8_U8 ? 128 : 0, side_off(scores_out), side_off(probs_out),
                          pl.store == LSQ_ATTN_W8_STORE_PACKETS ? 1 : 0};
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    int64_t* wi = reinterpret_cast<int64_t*>(ws + pl.ws_scores);
    const dim3 grid(static_cast<unsigned>(pl.grid)), heads(static_cast<unsigned>(pl.heads)), block(lsq::kSplThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int32_t* lens = static_cast<const int32_t*>(key_lengths);
    hipLaunchKernelGGL(scores, grid, block, 0, st, pl.g, arg, so, lens, static_cast<const uint8_t*>(q_levels),
                       static_cast<const uint8_t*>(k_levels), ws, keys);
    if (int rc = hip_status(hipGetLastError(), what)) return rc;
    hipLaunchKernelGGL(context, grid, block, static_cast<size_t>(pl.lds), st, pl.g, arg, po, static_cast<const int32_t*>(table), lens,
                       static_cast<const uint8_t*>(v_levels), static_cast<const uint8_t*>(ws), wi, keys);
    if (int rc = hip_status(hipGetLastError(), what)) return rc;
    hipLaunchKernelGGL(reduce, heads, block, 0, st, pl.g, arg, co, lens, static_cast<const int64_t*>(wi), static_cast<uint8_t*>(y));
    return hip_status(hipGetLastError(), what);
}

}  // namespace
