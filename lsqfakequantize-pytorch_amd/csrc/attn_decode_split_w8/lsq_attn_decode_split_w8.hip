// lsq_attn_decode_split_w8.hip -- split-key decode attention on 8-bit levels on gfx950 (include/lsq_hip_attn_decode_split_w8.h, which
// states the contract): the three kernels and the C ABI of liblsq_hip_attn_decode_split_w8.so.
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
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../qlinear_w8/lsq_w8_shared.hpp"
#include "../attn_w8/lsq_attn_w8_dev.hpp"
#include "../attn_w8/lsq_attn_w8_checks.hpp"
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
    int64_t q_s0, q_s1, q_ld, k_s0, k_s1, k_ld, v_s0, v_s1, v_ld, y_s0, y_s1, y_ld;
    int64_t ldw;            // bytes between the score rows in the workspace: 16 ceil(Tk / 16)
    int Hkv, G, Tq, Tk, D;
    int R;                  // G Tq
    int causal, off;        // row t sees t + 1 + off keys (off clamped to Tk on the host)
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

// n(b, t) of the contract; len: max(key_lengths[b], 0), or Tk without lengths
__device__ __forceinline__ int spl_count(const SplGeom& g, int len, int t) {
    int n = min(g.Tk, len);
    if (g.causal) n = min(n, t + 1 + g.off);           // t < 16 and off <= Tk <= 65536
    return n;
}

// ------------------------------------------------------------------------------------------------ launch 1: the scores of a chunk
__global__ __launch_bounds__(kSplThreads) void attn_split_scores_kernel(SplGeom g, SplArg a, AttnOut so, const int32_t* __restrict__ lens,
                                                                        const uint8_t* __restrict__ Q, const uint8_t* __restrict__ K,
                                                                        uint8_t* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) unsigned char sc[kSplScoreLds];      // [16][272]: the score bytes of a round
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const int64_t bh = static_cast<int64_t>(blockIdx.x) / g.S;
    const int s = static_cast<int>(static_cast<int64_t>(blockIdx.x) - bh * g.S);
    const int64_t b0 = bh / g.Hkv, b1 = bh - b0 * g.Hkv;
    const int len = lens ? max(lens[b0], 0) : g.Tk;
    const int nmax = spl_count(g, len, g.Tq - 1);                       // 0 .. Tk, the same for the S workgroups of the head
    const int c0 = s * g.chunk;                                         // s chunk < Tk + chunk: no overflow
    if (c0 >= nmax) return;                                             // the same for the whole workgroup, before any barrier
    const int c1 = min(c0 + g.chunk, nmax);
    const int jend = (c1 + 15) >> 4;                                    // 16-key sub-tiles below c1
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const uint32_t flip_q = a.off_q ? 0x80808080u : 0u, flip_k = a.off_k ? 0x80808080u : 0u;
    const int r = min(nl, g.R - 1);                                     // a clamped row computes values nobody stores
    const int rg = r / g.Tq, rt = r - rg * g.Tq;
    const uint8_t* __restrict__ qrow = Q + b0 * g.q_s0 + (b1 * g.G + rg) * g.q_s1 + static_cast<int64_t>(rt) * g.q_ld;
    const uint8_t* __restrict__ Kb = K + b0 * g.k_s0 + b1 * g.k_s1;
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
    for (int jb = c0 >> 4; jb < jend; jb += kSplRound / 16) {           // the same for the whole workgroup
        const int j0 = jb + wave * kSplInFlight;
        u32x4 kv[kSplInFlight][2];
#pragma unroll
        for (int u = 0; u < kSplInFlight; ++u) {
            kv[u][0] = u32x4{0u, 0u, 0u, 0u};
            kv[u][1] = u32x4{0u, 0u, 0u, 0u};
            if (j0 + u < jend) {
                // 16 (j0 + u) < c1: the clamped key is a key of the chunk
                const uint8_t* __restrict__ kr = Kb + static_cast<int64_t>(min(16 * (j0 + u) + nl, c1 - 1)) * g.k_ld;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int kk = 64 * h + 16 * q;
                    if (kk < g.D) kv[u][h] = *reinterpret_cast<const u32x4*>(kr + kk) ^ flip_k;        // a packet beyond D: the operand's zero
                }
            }
        }
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
        __syncthreads();                                                // the round's scores are in LDS
        {
            const int pr = tid >> 4, pk = tid & 15;                     // (row, packet of the round)
            // 16 (jb + pk) + 16 <= 16 jend <= 16 ceil(Tk / 16) = ldw
            if (pr < g.R && jb + pk < jend)
                *reinterpret_cast<u32x4*>(wrow + 16 * static_cast<int64_t>(jb + pk)) = *reinterpret_cast<const u32x4*>(sc + pr * kSplScoreLd + 16 * pk);
        }
        __syncthreads();                                                // before the next round overwrites them
    }
}

// ------------------------------------------------------------------------------------------------ launch 2: the chunk's context integer
__global__ __launch_bounds__(kSplThreads) void attn_split_context_kernel(SplGeom g, SplArg a, AttnOut po, const int32_t* __restrict__ table,
                                                                         const int32_t* __restrict__ lens, const uint8_t* __restrict__ V,
                                                                         const uint8_t* __restrict__ ws, int64_t* __restrict__ wi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int32_t* tab = reinterpret_cast<int32_t*>(lds);                                 // [256]
    int* row_m = reinterpret_cast<int*>(lds + kSplTable);                           // [16] the biased byte maximum
    float* row_r = reinterpret_cast<float*>(lds + kSplTable + 64);                  // [16] 1 / float(S), 0 where n = 0
    int* row_n = reinterpret_cast<int*>(lds + kSplTable + 128);                     // [16] n_r, 0 in rows >= R
    unsigned char* ptile = lds + kSplTable + kSplRowInfo;                           // 2 x [16][80]: p bytes, the operand's sign flip applied
    unsigned char* stage = ptile + 2 * kSplRows * kSplTStride;                      // 2 x [D][80]: v transposed
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const int64_t bh = static_cast<int64_t>(blockIdx.x) / g.S;
    const int s = static_cast<int>(static_cast<int64_t>(blockIdx.x) - bh * g.S);
    const int64_t b0 = bh / g.Hkv, b1 = bh - b0 * g.Hkv;
    const int len = lens ? max(lens[b0], 0) : g.Tk;
    const int nmax = spl_count(g, len, g.Tq - 1);
    const int c0 = s * g.chunk;
    if (c0 >= nmax) return;                                             // the same for the whole workgroup, before any barrier
    const int c1 = min(c0 + g.chunk, nmax);
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const uint32_t flip_s = a.off_s ? 0u : 0x80808080u;                 // int8 levels are biased by 128 on load
    const uint8_t* __restrict__ wsb = ws + bh * g.R * g.ldw;            // the head's score rows [R][ldw]

    tab[tid] = table[tid];                                              // 256 threads
    __syncthreads();

    // ---- the rows' maximum and sum over their WHOLE prefix: packets below 16 ceil(n_r / 16) <= 16 ceil(nmax / 16), all written
    for (int r = wave; r < kSplRows; r += kSplWaves) {                  // the same for the whole wave
        int n = 0, m = 0;
        float rcp = 0.0f;
        if (r < g.R) {
            const uint8_t* __restrict__ row = wsb + r * g.ldw;
            n = spl_count(g, len, r % g.Tq);                            // n <= nmax
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
    const uint8_t* __restrict__ srow = wsb + min(pr, g.R - 1) * g.ldw;  // read only where a key lies below my_n (0 in rows >= R)
    const uint8_t* __restrict__ Vb = V + b0 * g.v_s0 + b1 * g.v_s1;
    const int subs = g.D >> 4;                                          // 16-column sub-tiles of the context, 1 .. 8
    const int wpr = g.D >> 2, items = 16 * wpr;                         // words of a v row; (four keys, a word) items of a step
    i32x4 P[kSplSubsPerWave], Cs[kSplSubsPerWave], Rs = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < kSplSubsPerWave; ++j) {
        P[j] = i32x4{0, 0, 0, 0};
        Cs[j] = i32x4{0, 0, 0, 0};
    }
    uint32_t vr[2][4];                                                  // the rows of the step to be staged next
    uint32_t sw = 0u;                                                   // the score word of the step to be staged next
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = tid + it * kSplThreads, kg = idx / wpr, d = idx - kg * wpr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = c0 + 4 * kg + i;
            vr[it][i] = 0u;                                             // a row beyond c1: the operand's zero
            if (idx < items && k < c1) vr[it][i] = *reinterpret_cast<const uint32_t*>(Vb + static_cast<int64_t>(k) * g.v_ld + 4 * d) ^ flip_v;
        }
    }
    if (c0 + 4 * pw < my_n) sw = *reinterpret_cast<const uint32_t*>(srow + c0 + 4 * pw) ^ flip_s;       // my_n <= nmax: a written packet
    int buf = 0;
    for (int k0 = c0; k0 < c1; k0 += kSplStep) {                        // the same for the whole workgroup
        unsigned char* st = stage + buf * (kSplTStride * g.D);
        unsigned char* pt = ptile + buf * (kSplRows * kSplTStride);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = tid + it * kSplThreads, kg = idx / wpr, d = idx - kg * wpr;
            if (idx < items) {
                uint32_t c[4];
                attn_transpose4(vr[it][0], vr[it][1], vr[it][2], vr[it][3], c);
#pragma unroll
                for (int i = 0; i < 4; ++i) *reinterpret_cast<uint32_t*>(st + (4 * d + i) * kSplTStride + 4 * kg) = c[i];
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
            *reinterpret_cast<uint32_t*>(pt + pr * kSplTStride + 4 * pw) = w;
        }
        if (k0 + kSplStep < c1) {                                       // the next step's rows are in flight during this one's MFMAs
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int idx = tid + it * kSplThreads, kg = idx / wpr, d = idx - kg * wpr;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + kSplStep + 4 * kg + i;
                    vr[it][i] = 0u;
                    if (idx < items && k < c1) vr[it][i] = *reinterpret_cast<const uint32_t*>(Vb + static_cast<int64_t>(k) * g.v_ld + 4 * d) ^ flip_v;
                }
            }
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
            if (r < g.R) out[static_cast<int64_t>(r) * g.D + 16 * j + nl] = bmm_exact(P[jj][i], Cs[jj][i], Rs[i], c1 - c0, z_p, z_v);
        }
    }
}

// ------------------------------------------------------------------------------------------------ launch 3: the sum over the chunks, the levels
__global__ __launch_bounds__(kSplThreads) void attn_split_reduce_kernel(SplGeom g, SplArg a, AttnOut co, const int32_t* __restrict__ lens,
                                                                        const int64_t* __restrict__ wi, uint8_t* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[kSplRows * LSQ_ATTN_DECODE_SPLIT_W8_MAX_D];      // the level tile [R][D]
    const int tid = static_cast<int>(threadIdx.x);
    const int64_t bh = static_cast<int64_t>(blockIdx.x);
    const int64_t b0 = bh / g.Hkv, b1 = bh - b0 * g.Hkv;
    const int len = lens ? max(lens[b0], 0) : g.Tk;
    const int nmax = spl_count(g, len, g.Tq - 1);
    const int live = (nmax + g.chunk - 1) / g.chunk;                    // the chunks that start below nmax: the ones launch 2 wrote; <= S
    const AttnQ oq = attn_constants(co);
    const float s_p = a.s_p[0], s_v = a.s_v[0];
    const int RD = g.R * g.D;                                           // <= 2048
    const int64_t* __restrict__ src = wi + bh * g.S * RD;               // [S][R][D]
    for (int e = tid; e < RD; e += kSplThreads) {
        int64_t I = 0;
        for (int c = 0; c < live; ++c) I += src[static_cast<int64_t>(c) * RD + e];
        const float u = bmm_value(static_cast<float>(I), s_p, s_v, oq.mid);
        tile[e] = static_cast<unsigned char>(w8o_byte(u, oq));
    }
    __syncthreads();
    uint8_t* __restrict__ yb = y + b0 * g.y_s0 + (b1 * g.G) * g.y_s1;
    const int subs = g.D >> 4, total = g.R * subs;                      // 16-byte packets of the rows that exist
    for (int idx = tid; idx < total; idx += kSplThreads) {
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

// ------------------------------------------------------------------------------------------------
// host side: the plan
// ------------------------------------------------------------------------------------------------
struct SplPlan {
    int family, rows, chunk, splits, lds, store;
    int64_t grid, heads, ldw, ws_scores, ws_bytes;      // B Hkv S; B Hkv; the workspace's row stride, its score part and its size
    SplGeom g;
};

inline bool strides16(const lsq_attn_w8_strides& s) { return s.s0 % 16 == 0 && s.s1 % 16 == 0 && s.ld % 16 == 0; }

// the chunk for `splits` (0: the library's own choice; else at most that many splits), a multiple of 64
inline int64_t split_chunk(int64_t heads, int64_t Tk, int64_t splits) {
    const int64_t units = (Tk + kSplStep - 1) / kSplStep;
    if (splits > 0) return kSplStep * ((units + splits - 1) / splits);
    // the fewest splits with which the grid fills the part, dealt evenly; the chunk taken into its range
    const int64_t want = static_cast<int64_t>(LSQ_ATTN_DECODE_SPLIT_W8_WG_PER_CU) * LSQ_ATTN_DECODE_SPLIT_W8_CUS;
    const int64_t fewest = std::min<int64_t>((want + heads - 1) / heads, LSQ_ATTN_DECODE_SPLIT_W8_MAX_SPLITS);
    const int64_t chunk = kSplStep * ((units + fewest - 1) / fewest);
    return std::min<int64_t>(std::max<int64_t>(chunk, LSQ_ATTN_DECODE_SPLIT_W8_MIN_CHUNK), LSQ_ATTN_DECODE_SPLIT_W8_MAX_CHUNK);
}

inline bool split_extents_served(const lsq_attn_decode_w8_geom& ge) {
    const int64_t R = ge.H / ge.Hkv * ge.Tq;
    return ge.D % 16 == 0 && ge.D >= 16 && ge.D <= LSQ_ATTN_DECODE_SPLIT_W8_MAX_D && ge.Tk <= LSQ_ATTN_DECODE_SPLIT_W8_MAX_TK &&
           R <= LSQ_ATTN_DECODE_SPLIT_W8_MAX_ROWS;
}

inline SplPlan plan_split(const lsq_attn_decode_w8_geom& ge, bool qkv_aligned, bool y_aligned, int64_t splits) {
    SplPlan pl = {};
    pl.family = LSQ_ATTN_DECODE_SPLIT_W8_COMPOSITION;
    if (!(qkv_aligned && strides16(ge.q) && strides16(ge.k) && strides16(ge.v) && split_extents_served(ge))) return pl;
    const int64_t G = ge.H / ge.Hkv, R = G * ge.Tq;
    const int Tk = static_cast<int>(ge.Tk), D = static_cast<int>(ge.D);
    pl.family = LSQ_ATTN_DECODE_SPLIT_W8_SPLIT;
    pl.heads = ge.B * ge.Hkv;
    pl.chunk = static_cast<int>(split_chunk(pl.heads, ge.Tk, splits));
    pl.splits = (Tk + pl.chunk - 1) / pl.chunk;
    pl.rows = static_cast<int>(R);
    pl.lds = spl_context_lds(D);
    pl.store = y_aligned && strides16(ge.y) ? LSQ_ATTN_W8_STORE_PACKETS : LSQ_ATTN_W8_STORE_ELEMS;
    pl.grid = pl.heads * pl.splits;
    pl.ldw = 16 * ((ge.Tk + 15) / 16);
    pl.ws_scores = pl.heads * R * pl.ldw;                               // a multiple of 16: the integers behind it are aligned
    pl.ws_bytes = pl.ws_scores + 8 * pl.heads * pl.splits * R * ge.D;
    pl.g = SplGeom{ge.q.s0, ge.q.s1, ge.q.ld, ge.k.s0, ge.k.s1, ge.k.ld, ge.v.s0, ge.v.s1, ge.v.ld, ge.y.s0, ge.y.s1, ge.y.ld, pl.ldw,
                   static_cast<int>(ge.Hkv), static_cast<int>(G), static_cast<int>(ge.Tq), Tk, D, pl.rows, ge.causal ? 1 : 0,
                   ge.causal ? static_cast<int>(std::min<int64_t>(ge.causal_offset, ge.Tk)) : 0, pl.chunk, pl.splits};
    return pl;
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_attn_decode_split_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// (the checks of lsq_attn_decode_w8, which that library keeps in its own translation unit)
int check_split_geom(const char* what, const lsq_attn_decode_w8_geom* g) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (!level_dtype(g->q_dtype) || !level_dtype(g->k_dtype) || !level_dtype(g->v_dtype))
        return fail(LSQ_EINVAL, "%s: q_dtype, k_dtype and v_dtype must be LSQ_ATTN_W8_U8 (0) or LSQ_ATTN_W8_I8 (1), got %lld, %lld and %lld",
                    what, static_cast<ll>(g->q_dtype), static_cast<ll>(g->k_dtype), static_cast<ll>(g->v_dtype));
    if (g->B < 1 || g->H < 1 || g->Hkv < 1 || g->Tq < 1 || g->Tk < 1 || g->D < 1)
        return fail(LSQ_EINVAL, "%s: [B, H, Hkv, Tq, Tk, D] = [%lld, %lld, %lld, %lld, %lld, %lld], every extent must be at least 1", what,
                    static_cast<ll>(g->B), static_cast<ll>(g->H), static_cast<ll>(g->Hkv), static_cast<ll>(g->Tq), static_cast<ll>(g->Tk),
                    static_cast<ll>(g->D));
    if (g->H % g->Hkv != 0)
        return fail(LSQ_EINVAL, "%s: H = %lld query heads are not a multiple of Hkv = %lld kv heads", what, static_cast<ll>(g->H),
                    static_cast<ll>(g->Hkv));
    if (g->causal && g->causal_offset < 0)
        return fail(LSQ_EINVAL, "%s: causal_offset = %lld must be at least 0", what, static_cast<ll>(g->causal_offset));
    if (g->D > LSQ_ATTN_W8_MAX_K || g->Tk > LSQ_ATTN_W8_MAX_K)
        return fail(LSQ_EINVAL, "%s: D = %lld and Tk = %lld, at most %d are served (the raw sums stay in 32 bits)", what, static_cast<ll>(g->D),
                    static_cast<ll>(g->Tk), LSQ_ATTN_W8_MAX_K);
    const int64_t lim = int64_t{1} << 20;
    if (g->Tq > lim || g->B > lim || g->H > lim || g->B * g->H > lim)
        return fail(LSQ_EINVAL, "%s: Tq = %lld and B * H = %lld x %lld may each be 2^20 at most", what, static_cast<ll>(g->Tq),
                    static_cast<ll>(g->B), static_cast<ll>(g->H));
    if (int rc = check_strides(what, "q", g->q, g->D)) return rc;
    if (int rc = check_strides(what, "k", g->k, g->D)) return rc;
    if (int rc = check_strides(what, "v", g->v, g->D)) return rc;
    if (int rc = check_strides(what, "y", g->y, g->D)) return rc;
    if (self_overlap(g->y, g->B, g->H, g->Tq, g->D))
        return fail(LSQ_EINVAL, "%s: y's rows or batches overlap each other (strides %lld, %lld, %lld for [%lld, %lld, %lld, %lld])", what,
                    static_cast<ll>(g->y.s0), static_cast<ll>(g->y.s1), static_cast<ll>(g->y.ld), static_cast<ll>(g->B),
                    static_cast<ll>(g->H), static_cast<ll>(g->Tq), static_cast<ll>(g->D));
    return LSQ_OK;
}

int check_splits(const char* what, const lsq_attn_decode_w8_geom* g, int64_t splits) {
    const int64_t most = (g->Tk + lsq::kSplStep - 1) / lsq::kSplStep;
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

}  // namespace

extern "C" {

int lsq_attn_decode_split_w8_abi_version(void) { return LSQ_ATTN_DECODE_SPLIT_W8_ABI_VERSION; }

const char* lsq_attn_decode_split_w8_last_error(void) { return g_last_error; }

int lsq_attn_decode_split_w8_workspace(const lsq_attn_decode_w8_geom* geom, int64_t splits, int64_t* bytes) {
    const char* what = "lsq_attn_decode_split_w8_workspace";
    if (int rc = check_split_geom(what, geom)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (!bytes) return fail(LSQ_EINVAL, "%s: NULL bytes", what);
    lsq_attn_decode_w8_geom dense = *geom;                              // the size does not depend on bases or strides
    dense.q = dense.k = dense.v = lsq_attn_w8_strides{0, 0, 16 * ((geom->D + 15) / 16)};
    const lsq::SplPlan pl = lsq::plan_split(dense, true, true, splits);
    if (int rc = check_grid(what, pl.grid)) return rc;
    *bytes = pl.family == LSQ_ATTN_DECODE_SPLIT_W8_SPLIT ? pl.ws_bytes : 0;
    return LSQ_OK;
}

int lsq_attn_decode_split_w8(const lsq_attn_decode_w8_geom* geom, const lsq_attn_decode_w8_consts* consts, const lsq_attn_w8_out* scores_out,
                             const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out, const void* table, const void* key_lengths,
                             const void* q_levels, const void* k_levels, const void* v_levels, void* y, void* workspace,
                             int64_t workspace_bytes, int64_t splits, void* stream) {
    const char* what = "lsq_attn_decode_split_w8";
    lsq::AttnOut so{}, po{}, co{};
    if (int rc = check_split_geom(what, geom)) return rc;
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
    if (!table || !q_levels || !k_levels || !v_levels || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(table, 4)) return fail(LSQ_EINVAL, "%s: the table must be element-aligned", what);
    if (geom->has_lengths && !key_lengths) return fail(LSQ_EINVAL, "%s: key_lengths is NULL but the geometry says has_lengths", what);
    if (!geom->has_lengths && key_lengths) return fail(LSQ_EINVAL, "%s: key_lengths is given but the geometry says has_lengths = 0", what);
    if (key_lengths && !aligned_to(key_lengths, 4)) return fail(LSQ_EINVAL, "%s: key_lengths must be 4-byte aligned", what);
    const int64_t q_span = span_of(geom->q, geom->B, geom->H, geom->Tq, geom->D), k_span = span_of(geom->k, geom->B, geom->Hkv, geom->Tk, geom->D);
    const int64_t v_span = span_of(geom->v, geom->B, geom->Hkv, geom->Tk, geom->D), y_bytes = span_of(geom->y, geom->B, geom->H, geom->Tq, geom->D);
    if (overlap(y, y_bytes, q_levels, q_span) || overlap(y, y_bytes, k_levels, k_span) || overlap(y, y_bytes, v_levels, v_span) ||
        overlap(y, y_bytes, table, 1024) || (key_lengths && overlap(y, y_bytes, key_lengths, 4 * geom->B)))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap q's %lld, k's %lld, v's %lld, the table or key_lengths", what,
                    static_cast<ll>(y_bytes), static_cast<ll>(q_span), static_cast<ll>(k_span), static_cast<ll>(v_span));
    const lsq::SplPlan pl = lsq::plan_split(*geom, aligned_to(q_levels, 16) && aligned_to(k_levels, 16) && aligned_to(v_levels, 16),
                                            aligned_to(y, 16), splits);
    if (pl.family != LSQ_ATTN_DECODE_SPLIT_W8_SPLIT)
        return fail(LSQ_EINVAL, "%s: [B, H, Hkv, Tq, Tk, D] = [%lld, %lld, %lld, %lld, %lld, %lld] with these bases and strides is not served "
                    "by the split kernels (G Tq <= %d, q, k, v 16-byte aligned with strides that are multiples of 16, D %% 16 == 0, "
                    "16 <= D <= %d, Tk <= %d): compose lsq_hip_attn_w8.h and lsq_hip_attn_mask_w8.h", what, static_cast<ll>(geom->B),
                    static_cast<ll>(geom->H), static_cast<ll>(geom->Hkv), static_cast<ll>(geom->Tq), static_cast<ll>(geom->Tk),
                    static_cast<ll>(geom->D), LSQ_ATTN_DECODE_SPLIT_W8_MAX_ROWS, LSQ_ATTN_DECODE_SPLIT_W8_MAX_D, LSQ_ATTN_DECODE_SPLIT_W8_MAX_TK);
    if (int rc = check_grid(what, pl.grid)) return rc;
    if (!workspace) return fail(LSQ_EINVAL, "%s: NULL workspace (%lld bytes are needed: lsq_attn_decode_split_w8_workspace)", what, static_cast<ll>(pl.ws_bytes));
    if (!aligned_to(workspace, 16)) return fail(LSQ_EINVAL, "%s: the workspace must be 16-byte aligned", what);
    if (workspace_bytes < pl.ws_bytes)
        return fail(LSQ_EINVAL, "%s: the workspace has %lld bytes, %lld are needed (lsq_attn_decode_split_w8_workspace)", what,
                    static_cast<ll>(workspace_bytes), static_cast<ll>(pl.ws_bytes));
    if (overlap(workspace, pl.ws_bytes, q_levels, q_span) || overlap(workspace, pl.ws_bytes, k_levels, k_span) ||
        overlap(workspace, pl.ws_bytes, v_levels, v_span) || overlap(workspace, pl.ws_bytes, y, y_bytes) ||
        overlap(workspace, pl.ws_bytes, table, 1024) || (key_lengths && overlap(workspace, pl.ws_bytes, key_lengths, 4 * geom->B)))
        return fail(LSQ_EINVAL, "%s: the workspace's %lld bytes overlap q, k, v, y, the table or key_lengths", what, static_cast<ll>(pl.ws_bytes));
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
    hipLaunchKernelGGL(lsq::attn_split_scores_kernel, grid, block, 0, st, pl.g, arg, so, lens, static_cast<const uint8_t*>(q_levels),
                       static_cast<const uint8_t*>(k_levels), ws);
    if (int rc = hip_status(hipGetLastError(), what)) return rc;
    hipLaunchKernelGGL(lsq::attn_split_context_kernel, grid, block, static_cast<size_t>(pl.lds), st, pl.g, arg, po,
                       static_cast<const int32_t*>(table), lens, static_cast<const uint8_t*>(v_levels), static_cast<const uint8_t*>(ws), wi);
    if (int rc = hip_status(hipGetLastError(), what)) return rc;
    hipLaunchKernelGGL(lsq::attn_split_reduce_kernel, heads, block, 0, st, pl.g, arg, co, lens, static_cast<const int64_t*>(wi),
                       static_cast<uint8_t*>(y));
    return hip_status(hipGetLastError(), what);
}

int lsq_attn_decode_split_w8_plan(const lsq_attn_decode_w8_geom* geom, int qkv_aligned, int y_aligned, int64_t splits, int32_t* out8) {
    const char* what = "lsq_attn_decode_split_w8_plan";
    if (int rc = check_split_geom(what, geom)) return rc;
    if (int rc = check_splits(what, geom, splits)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::SplPlan pl = lsq::plan_split(*geom, qkv_aligned != 0, y_aligned != 0, splits);
    if (int rc = check_grid(what, pl.grid)) return rc;
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.family == LSQ_ATTN_DECODE_SPLIT_W8_SPLIT ? lsq::kSplThreads : 0;
    out8[3] = pl.rows;
    out8[4] = pl.chunk;
    out8[5] = pl.splits;
    out8[6] = pl.lds;
    out8[7] = pl.store;
    return LSQ_OK;
}

}  // extern "C"
