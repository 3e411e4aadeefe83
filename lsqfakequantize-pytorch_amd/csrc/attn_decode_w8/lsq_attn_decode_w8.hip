// lsq_attn_decode_w8.hip -- decode attention on 8-bit levels against a grouped-query KV cache in one launch on gfx950
// (include/lsq_hip_attn_decode_w8.h, which states the contract): the kernel and the C ABI of liblsq_hip_attn_decode_w8.so.
//
// One workgroup of nw = 4 or 8 waves takes one (b, kv head): the R = G Tq <= 16 query rows that read that head are ONE 16-row tile
// of the matrix core, row r = g Tq + t being q[b, hkv G + g, t], so k[b, hkv] and v[b, hkv] are read once for all G heads.
// nmax = max_t n(b, t) = n(b, Tq - 1) is uniform in the workgroup and every key loop ends there: Tk only sizes the LDS.
//  1 SCORES   the q packets stay in registers (every wave holds all 16 rows); wave w takes the 16-key sub-tiles 4 (w + i nw) ..
//             + 3 below nmax, FOUR sub-tiles' k packets in flight at once, k's rows the MFMA B operand straight from memory
//             (v_mfma_i32_16x16x64_i8), sum q and sum k from the all-ones MFMAs; the epilogue of the fused kernel; the score BYTE
//             goes into LDS [16][ld].  Keys beyond nmax are clamped to nmax - 1: their bytes are never counted.
//  2 SOFTMAX  after a workgroup barrier, wave w takes the rows w, w + nw, .. < R: a lane walks the packets lane, lane + 64, .. of
//             the row's prefix n_r three times (max, sum, write), in place.  A packet's 16 table entries (<= 2^28) are summed in 32
//             bits and added to the lane's 64-bit sum, which crosses lanes as 64 bits.  Bytes in [n_r, 16 ceil(nmax / 16)) become
//             the byte z_p: one K = nmax then serves the raw-sum correction of all 16 rows.
//  3 CONTEXT  after a barrier, p [16 x nmax] times v [nmax x D], K = nmax: the A packets from LDS, v staged per 64-key step
//             through LDS transposed into [D][80] (attn_transpose4) by all waves, DOUBLE BUFFERED -- the next step's rows are in
//             registers while this step's MFMAs run, one barrier per step; the D / 16 accumulator sub-tiles are dealt to the waves
//             (all sums are integers: exact for any split).  Rows of v and bytes of p beyond nmax enter as the operand's zero.
//             The epilogue of the fused kernel; the level tile leaves through LDS as 16-byte packets (byte by byte into a y that
//             is not packet-aligned).
// LDS is not zeroed between workgroups: rows >= R hold clamped copies of row R - 1 (nobody stores them), score packets at and
// beyond 16 ceil(nmax / 16) are never read, and the tail of the last packet is masked where phase 3 reads it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../qlinear_w8/lsq_w8_shared.hpp"
#include "../attn_w8/lsq_attn_w8_dev.hpp"
#include "../attn_w8/lsq_attn_decode_checks.hpp"
#include "../../../include/lsq_hip_attn_decode_w8.h"

namespace lsq {

typedef __attribute__((ext_vector_type(2))) unsigned short dec_u16x2;

constexpr int kDecRows = LSQ_ATTN_DECODE_W8_MAX_ROWS;   // the row tile of the matrix core
constexpr int kDecStep = 64;                            // keys per step of phase 3
constexpr int kDecVtStride = kDecStep + 16;             // bytes between the rows of a transposed v tile in LDS
constexpr int kDecTable = 1024;
constexpr int kDecMaxThreads = 512;
constexpr int kDecSmallTk = 256;                        // up to here four waves, above eight
constexpr int kDecInFlight = 4;                         // 16-key sub-tiles of k a wave loads before it multiplies
constexpr int kDecSubsPerWave = 2;                      // D / 16 <= 8 accumulator sub-tiles over at least four waves

constexpr int dec_ld(int Tk) {                          // 16 n, n = ceil(Tk / 16) made odd: 16 rows start on different banks
    return 16 * (((Tk + 15) / 16) | 1);
}
constexpr int dec_lds(int Tk, int D) { return kDecRows * dec_ld(Tk) + kDecTable + 2 * kDecVtStride * D; }
constexpr int kDecMaxLds = dec_lds(LSQ_ATTN_DECODE_W8_MAX_TK, LSQ_ATTN_DECODE_W8_MAX_D);
static_assert(kDecMaxLds <= LSQ_ATTN_DECODE_W8_MAX_LDS, "the largest served geometry fits the CU's LDS");
static_assert(kDecRows * LSQ_ATTN_DECODE_W8_MAX_D <= 2 * kDecVtStride * LSQ_ATTN_DECODE_W8_MAX_D, "the level tile fits the staging area");
static_assert(kDecSubsPerWave * 4 * 16 >= LSQ_ATTN_DECODE_W8_MAX_D, "four waves cover every sub-tile of D");

struct DecGeom {            // kernel argument
    int64_t q_s0, q_s1, q_ld, k_s0, k_s1, k_ld, v_s0, v_s1, v_ld, y_s0, y_s1, y_ld;
    int Hkv, G, Tq, Tk, D;
    int R, ld;              // G Tq; bytes between score rows in LDS
    int causal, off;        // row t sees t + 1 + off keys (off clamped to Tk on the host)
};

struct DecArg {             // kernel argument
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
__device__ __forceinline__ int dec_count(const DecGeom& g, int len, int t) {
    int n = min(g.Tk, len);
    if (g.causal) n = min(n, t + 1 + g.off);           // t < 16 and off <= Tk <= 8192
    return n;
}

__global__ __launch_bounds__(kDecMaxThreads) void attn_decode_w8_kernel(DecGeom g, DecArg a, AttnOut so, AttnOut po, AttnOut co,
                                                                        const int32_t* __restrict__ table,
                                                                        const int32_t* __restrict__ lens, const uint8_t* __restrict__ Q,
                                                                        const uint8_t* __restrict__ K, const uint8_t* __restrict__ V,
                                                                        uint8_t* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* sc = lds;                                            // [16][ld]: score bytes, then probability bytes
    int32_t* tab = reinterpret_cast<int32_t*>(lds + kDecRows * g.ld);   // [256]
    unsigned char* stage = lds + kDecRows * g.ld + kDecTable;           // v transposed 2 x [D][80]; then the level tile [16][D]
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nthr = static_cast<int>(blockDim.x), nw = nthr >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) / g.Hkv, b1 = static_cast<int64_t>(blockIdx.x) - b0 * g.Hkv;
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const int len = lens ? max(lens[b0], 0) : g.Tk;
    const int nmax = dec_count(g, len, g.Tq - 1);                       // 0 .. Tk, the same for the whole workgroup
    const int nsub = (nmax + 15) >> 4;                                  // 16-key sub-tiles below nmax, and the packets of a row that count
    unsigned char* myrow = sc + nl * g.ld;                              // the row this lane reads as the A operand in phase 3

    if (tid < 256) tab[tid] = table[tid];

    // -------------------------------------------------------------------------------------------- phase 1: the scores
    if (nsub > 0) {
        const uint32_t flip_q = a.off_q ? 0x80808080u : 0u, flip_k = a.off_k ? 0x80808080u : 0u;
        const int r = min(nl, g.R - 1);                                 // a clamped row computes values nobody stores
        const int rg = r / g.Tq, rt = r - rg * g.Tq;
        const uint8_t* __restrict__ qrow = Q + b0 * g.q_s0 + (b1 * g.G + rg) * g.q_s1 + static_cast<int64_t>(rt) * g.q_ld;
        const uint8_t* __restrict__ Kb = K + b0 * g.k_s0 + b1 * g.k_s1;
        i32x4 qi[2], Rs = {0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int kk = 64 * s + 16 * q;
            u32x4 v = {0u, 0u, 0u, 0u};                                 // a packet beyond D: the operand's zero
            if (kk < g.D) v = *reinterpret_cast<const u32x4*>(qrow + kk) ^ flip_q;
            qi[s] = w8_as_i32(v);
            Rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(qi[s], ones, Rs, 0, 0, 0);     // sum_k q of row 4 q + i in register i
        }
        const AttnQ sq = attn_constants(so);
        const BmmInt ex = bmm_int_constants(static_cast<int64_t>(a.z_q[0]) - a.off_q, static_cast<int64_t>(a.z_k[0]) - a.off_k, g.D);
        const float s_q = a.s_q[0], s_k = a.s_k[0];
        const bool two = g.D > 64;                                      // the same for the whole grid
        for (int j0 = wave * kDecInFlight; j0 < nsub; j0 += nw * kDecInFlight) {      // the same for the whole wave
            u32x4 kv[kDecInFlight][2];
#pragma unroll
            for (int u = 0; u < kDecInFlight; ++u) {
                kv[u][0] = u32x4{0u, 0u, 0u, 0u};
                kv[u][1] = u32x4{0u, 0u, 0u, 0u};
                if (j0 + u < nsub) {
                    // 16 (j0 + u) < nmax: the clamped key is a key below nmax
                    const uint8_t* __restrict__ kr = Kb + static_cast<int64_t>(min(16 * (j0 + u) + nl, nmax - 1)) * g.k_ld;
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int kk = 64 * s + 16 * q;
                        if (kk < g.D) kv[u][s] = *reinterpret_cast<const u32x4*>(kr + kk) ^ flip_k;      // a packet beyond D: the operand's zero
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kDecInFlight; ++u) {
                asm volatile("" : "+v"(kv[u][0]));                      // all in flight at once
                asm volatile("" : "+v"(kv[u][1]));
            }
#pragma unroll
            for (int u = 0; u < kDecInFlight; ++u) {
                const int j = j0 + u;
                if (j >= nsub) continue;
                i32x4 P = {0, 0, 0, 0}, Cs = {0, 0, 0, 0};
                const i32x4 k0 = w8_as_i32(kv[u][0]);
                P = __builtin_amdgcn_mfma_i32_16x16x64_i8(qi[0], k0, P, 0, 0, 0);
                Cs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, k0, Cs, 0, 0, 0);   // sum_k k of the lane's key, in every register
                if (two) {
                    const i32x4 k1 = w8_as_i32(kv[u][1]);
                    P = __builtin_amdgcn_mfma_i32_16x16x64_i8(qi[1], k1, P, 0, 0, 0);
                    Cs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, k1, Cs, 0, 0, 0);
                }
                // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register; 16 j + nl < 16 nsub <= ld
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float uu = bmm_value(bmm_int_float(ex, P[i], Cs[i], Rs[i]), s_q, s_k, sq.mid);
                    sc[(4 * q + i) * g.ld + 16 * j + nl] = static_cast<unsigned char>(w8o_byte(uu, sq));
                }
            }
        }
    }
    __syncthreads();                                                    // the scores and the table are in LDS

    // -------------------------------------------------------------------------------------------- phase 2: the softmax, in place
    if (nsub > 0) {
        const uint32_t flip_s = a.off_s ? 0u : 0x80808080u;             // int8 levels are biased by 128 on load
        const AttnQ pq = attn_constants(po);
        const uint32_t zb = static_cast<uint32_t>(a.z_p[0]) & 0xffu, zw = zb * 0x01010101u;       // the byte z_p
        for (int r = wave; r < g.R; r += nw) {                          // the same for the whole wave
            unsigned char* row = sc + r * g.ld;
            const int n = dec_count(g, len, r % g.Tq);                  // n <= nmax
            const int npk = (n + 15) >> 4;
            dec_u16x2 me = {0, 0}, mo = {0, 0};
            for (int p = lane; p < npk; p += 64) {
                // bytes beyond n count as 0, the least biased byte
                const u32x4 v = attn_mask_tail(*reinterpret_cast<const u32x4*>(row + 16 * p) ^ flip_s, n - 16 * p);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    me = __builtin_elementwise_max(me, __builtin_bit_cast(dec_u16x2, v[i] & 0x00ff00ffu));
                    mo = __builtin_elementwise_max(mo, __builtin_bit_cast(dec_u16x2, (v[i] >> 8) & 0x00ff00ffu));
                }
            }
            me = __builtin_elementwise_max(me, mo);
            int m = max(static_cast<int>(me[0]), static_cast<int>(me[1]));
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) m = max(m, __shfl_xor(m, s));
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
            for (int s = 32; s >= 1; s >>= 1) S += smx_shfl_xor_u64(S, s);
            float rcp = 0.0f;
            if (n > 0) rcp = __fdiv_rn(1.0f, static_cast<float>(S));   // n = 0: nothing is divided and no p is formed
            for (int p = lane; p < nsub; p += 64) {
                const int valid = min(max(n - 16 * p, 0), 16);
                uint32_t w[4] = {zw, zw, zw, zw};                       // the byte z_p from n on
                if (valid > 0) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(row + 16 * p) ^ flip_s;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int b = static_cast<int>((v[i / 4] >> (8 * (i % 4))) & 0xffu);
                        const uint32_t pb = w8o_byte(smx_value(tab[(m - b) & 0xff], rcp, pq.mid), pq);
                        const uint32_t sel = i < valid ? pb : zb;
                        w[i / 4] = (w[i / 4] & ~(0xffu << (8 * (i % 4)))) | (sel << (8 * (i % 4)));
                    }
                }
                *reinterpret_cast<u32x4*>(row + 16 * p) = u32x4{w[0], w[1], w[2], w[3]};
            }
        }
    }
    __syncthreads();                                                    // the probabilities are in LDS

    // -------------------------------------------------------------------------------------------- phase 3: the context
    const uint32_t flip_p = a.off_p ? 0x80808080u : 0u, flip_v = a.off_v ? 0x80808080u : 0u;
    const uint8_t* __restrict__ Vb = V + b0 * g.v_s0 + b1 * g.v_s1;
    const int subs = g.D >> 4;                                          // 16-column sub-tiles of the context, 1 .. 8
    const int wpr = g.D >> 2, items = 16 * wpr;                         // words of a v row; (four keys, a word) items of a step
    i32x4 P[kDecSubsPerWave], Cs[kDecSubsPerWave], Rs = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < kDecSubsPerWave; ++j) {
        P[j] = i32x4{0, 0, 0, 0};
        Cs[j] = i32x4{0, 0, 0, 0};
    }
    uint32_t vr[2][4];                                                  // the rows of the step to be staged next
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = tid + it * nthr, kg = idx / wpr, d = idx - kg * wpr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 4 * kg + i;
            vr[it][i] = 0u;                                             // a row beyond nmax: the operand's zero
            if (idx < items && k < nmax) vr[it][i] = *reinterpret_cast<const uint32_t*>(Vb + static_cast<int64_t>(k) * g.v_ld + 4 * d) ^ flip_v;
        }
    }
    int buf = 0;
    for (int k0 = 0; k0 < nmax; k0 += kDecStep) {                       // the same for the whole workgroup
        unsigned char* st = stage + buf * (kDecVtStride * g.D);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = tid + it * nthr, kg = idx / wpr, d = idx - kg * wpr;
            if (idx < items) {
                uint32_t c[4];
                attn_transpose4(vr[it][0], vr[it][1], vr[it][2], vr[it][3], c);
#pragma unroll
                for (int i = 0; i < 4; ++i) *reinterpret_cast<uint32_t*>(st + (4 * d + i) * kDecVtStride + 4 * kg) = c[i];
            }
        }
        if (k0 + kDecStep < nmax) {                                     // the next step's rows are in flight during this one's MFMAs
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int idx = tid + it * nthr, kg = idx / wpr, d = idx - kg * wpr;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + kDecStep + 4 * kg + i;
                    vr[it][i] = 0u;
                    if (idx < items && k < nmax) vr[it][i] = *reinterpret_cast<const uint32_t*>(Vb + static_cast<int64_t>(k) * g.v_ld + 4 * d) ^ flip_v;
                }
            }
        }
        const int kk = k0 + q * 16;
        u32x4 av = {0u, 0u, 0u, 0u};                                    // kk < nmax: a packet below 16 nsub, its tail beyond nmax masked
        if (kk < nmax) av = attn_mask_tail(*reinterpret_cast<const u32x4*>(myrow + kk) ^ flip_p, nmax - kk);
        // this step's tile is staged; the other buffer was last read before the previous step's barrier
        __syncthreads();
        const i32x4 ai = w8_as_i32(av);
#pragma unroll
        for (int jj = 0; jj < kDecSubsPerWave; ++jj) {
            const int j = wave + jj * nw;
            if (j < subs) {                                             // the same for the whole wave
                const i32x4 bi = w8_as_i32(*reinterpret_cast<const u32x4*>(st + (16 * j + nl) * kDecVtStride + q * 16));
                P[jj] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ai, bi, P[jj], 0, 0, 0);
                Cs[jj] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bi, Cs[jj], 0, 0, 0);
            }
        }
        Rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ai, ones, Rs, 0, 0, 0);
        buf ^= 1;
    }

    const AttnQ oq = attn_constants(co);
    const BmmInt ex = bmm_int_constants(static_cast<int64_t>(a.z_p[0]) - a.off_p, static_cast<int64_t>(a.z_v[0]) - a.off_v, nmax);
    const float s_p = a.s_p[0], s_v = a.s_v[0];
    __syncthreads();                                                    // the last step's reads of the staging area are done
#pragma unroll
    for (int jj = 0; jj < kDecSubsPerWave; ++jj) {
        const int j = wave + jj * nw;
        if (j >= subs) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float u = bmm_value(bmm_int_float(ex, P[jj][i], Cs[jj][i], Rs[i]), s_p, s_v, oq.mid);
            stage[(4 * q + i) * g.D + 16 * j + nl] = static_cast<unsigned char>(w8o_byte(u, oq));
        }
    }
    __syncthreads();
    uint8_t* __restrict__ yb = y + b0 * g.y_s0 + (b1 * g.G) * g.y_s1;
    const int total = g.R * subs;                                       // 16-byte packets of the rows that exist
    for (int idx = tid; idx < total; idx += nthr) {
        const int r = idx / subs, c = (idx - r * subs) * 16;
        const int rg = r / g.Tq, rt = r - rg * g.Tq;
        uint8_t* dst = yb + rg * g.y_s1 + static_cast<int64_t>(rt) * g.y_ld + c;
        const unsigned char* src = stage + r * g.D + c;
        if (a.y_packets) {
            *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
        } else {
            for (int i = 0; i < 16; ++i) dst[i] = src[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan
// ------------------------------------------------------------------------------------------------
struct DecPlan {
    int family, block, rows, ld, lds, dynamic, store;
    int64_t grid;
    DecGeom g;
};

inline DecPlan plan_decode(const lsq_attn_decode_w8_geom& ge, bool qkv_aligned, bool y_aligned) {
    DecPlan pl = {};
    pl.family = LSQ_ATTN_DECODE_W8_COMPOSITION;
    const int64_t G = ge.H / ge.Hkv, R = G * ge.Tq;
    if (!(qkv_aligned && strides16(ge.q) && strides16(ge.k) && strides16(ge.v) && ge.D % 16 == 0 && ge.D >= 16 &&
          ge.D <= LSQ_ATTN_DECODE_W8_MAX_D && ge.Tk <= LSQ_ATTN_DECODE_W8_MAX_TK && R <= LSQ_ATTN_DECODE_W8_MAX_ROWS))
        return pl;
    const int Tk = static_cast<int>(ge.Tk), D = static_cast<int>(ge.D);
    pl.family = LSQ_ATTN_DECODE_W8_DECODE;
    pl.block = Tk <= kDecSmallTk ? 256 : kDecMaxThreads;
    pl.rows = static_cast<int>(R);
    pl.ld = dec_ld(Tk);
    pl.lds = dec_lds(Tk, D);
    pl.dynamic = pl.lds > 65536 ? 1 : 0;
    pl.store = y_aligned && strides16(ge.y) ? LSQ_ATTN_W8_STORE_PACKETS : LSQ_ATTN_W8_STORE_ELEMS;
    pl.grid = ge.B * ge.Hkv;
    pl.g = DecGeom{ge.q.s0, ge.q.s1, ge.q.ld, ge.k.s0, ge.k.s1, ge.k.ld, ge.v.s0, ge.v.s1, ge.v.ld, ge.y.s0, ge.y.s1, ge.y.ld,
                   static_cast<int>(ge.Hkv), static_cast<int>(G), static_cast<int>(ge.Tq), Tk, D, pl.rows, pl.ld,
                   ge.causal ? 1 : 0, ge.causal ? static_cast<int>(std::min<int64_t>(ge.causal_offset, ge.Tk)) : 0};
    return pl;
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_attn_decode_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
extern "C" {

int lsq_attn_decode_w8_abi_version(void) { return LSQ_ATTN_DECODE_W8_ABI_VERSION; }

const char* lsq_attn_decode_w8_last_error(void) { return g_last_error; }

int lsq_attn_decode_w8(const lsq_attn_decode_w8_geom* geom, const lsq_attn_decode_w8_consts* consts, const lsq_attn_w8_out* scores_out,
                       const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out, const void* table, const void* key_lengths,
                       const void* q_levels, const void* k_levels, const void* v_levels, void* y, void* stream) {
    const char* what = "lsq_attn_decode_w8";
    lsq::AttnOut so{}, po{}, co{};
    if (int rc = check_decode_geom(what, geom)) return rc;
    if (int rc = check_decode_consts(what, consts)) return rc;
    if (int rc = check_decode_sides(what, scores_out, probs_out, ctx_out, so, po, co)) return rc;
    if (!table || !q_levels || !k_levels || !v_levels || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(table, 4)) return fail(LSQ_EINVAL, "%s: the table must be element-aligned", what);
    if (int rc = check_key_lengths(what, geom, key_lengths)) return rc;
    const int64_t q_span = span_of(geom->q, geom->B, geom->H, geom->Tq, geom->D), k_span = span_of(geom->k, geom->B, geom->Hkv, geom->Tk, geom->D);
    const int64_t v_span = span_of(geom->v, geom->B, geom->Hkv, geom->Tk, geom->D), y_bytes = span_of(geom->y, geom->B, geom->H, geom->Tq, geom->D);
    if (overlap(y, y_bytes, q_levels, q_span) || overlap(y, y_bytes, k_levels, k_span) || overlap(y, y_bytes, v_levels, v_span) ||
        overlap(y, y_bytes, table, 1024) || (key_lengths && overlap(y, y_bytes, key_lengths, 4 * geom->B)))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap q's %lld, k's %lld, v's %lld, the table or key_lengths", what,
                    static_cast<ll>(y_bytes), static_cast<ll>(q_span), static_cast<ll>(k_span), static_cast<ll>(v_span));
    const lsq::DecPlan pl = lsq::plan_decode(*geom, aligned_to(q_levels, 16) && aligned_to(k_levels, 16) && aligned_to(v_levels, 16),
                                             aligned_to(y, 16));
    if (pl.family != LSQ_ATTN_DECODE_W8_DECODE)
        return fail(LSQ_EINVAL, "%s: [B, H, Hkv, Tq, Tk, D] = [%lld, %lld, %lld, %lld, %lld, %lld] with these bases and strides is not served "
                    "by the decode kernel (G Tq <= %d, q, k, v 16-byte aligned with strides that are multiples of 16, D %% 16 == 0, "
                    "16 <= D <= %d, Tk <= %d): compose lsq_hip_attn_w8.h and lsq_hip_attn_mask_w8.h", what, static_cast<ll>(geom->B),
                    static_cast<ll>(geom->H), static_cast<ll>(geom->Hkv), static_cast<ll>(geom->Tq), static_cast<ll>(geom->Tk),
                    static_cast<ll>(geom->D), LSQ_ATTN_DECODE_W8_MAX_ROWS, LSQ_ATTN_DECODE_W8_MAX_D, LSQ_ATTN_DECODE_W8_MAX_TK);
    if (int rc = check_grid(what, pl.grid)) return rc;
    if (pl.dynamic) {
        static lsq::LdsOnce once;
        if (int rc = hip_status(lsq::allow_lds(once, reinterpret_cast<const void*>(lsq::attn_decode_w8_kernel), lsq::kDecMaxLds), what)) return rc;
    }
    const lsq::DecArg arg{static_cast<const float*>(consts->s_q), static_cast<const int32_t*>(consts->z_q),
                          static_cast<const float*>(consts->s_k), static_cast<const int32_t*>(consts->z_k),
                          static_cast<const float*>(consts->s_v), static_cast<const int32_t*>(consts->z_v),
                          static_cast<const float*>(consts->s_p), static_cast<const int32_t*>(consts->z_p),
                          geom->q_dtype == LSQ_ATTN_W8_U8 ? 128 : 0, geom->k_dtype == LSQ_ATTN_W8_U8 ? 128 : 0,
                          geom->v_dtype == LSQ_ATTN_W8_U8 ? 128 : 0, side_off(scores_out), side_off(probs_out),
                          pl.store == LSQ_ATTN_W8_STORE_PACKETS ? 1 : 0};
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(static_cast<unsigned>(pl.block));
    hipLaunchKernelGGL(lsq::attn_decode_w8_kernel, grid, block, static_cast<size_t>(pl.lds), static_cast<hipStream_t>(stream), pl.g, arg, so,
                       po, co, static_cast<const int32_t*>(table), static_cast<const int32_t*>(key_lengths),
                       static_cast<const uint8_t*>(q_levels), static_cast<const uint8_t*>(k_levels), static_cast<const uint8_t*>(v_levels),
                       static_cast<uint8_t*>(y));
    return hip_status(hipGetLastError(), what);
}

int lsq_attn_decode_w8_plan(const lsq_attn_decode_w8_geom* geom, int qkv_aligned, int y_aligned, int32_t* out8) {
    const char* what = "lsq_attn_decode_w8_plan";
    if (int rc = check_decode_geom(what, geom)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::DecPlan pl = lsq::plan_decode(*geom, qkv_aligned != 0, y_aligned != 0);
    if (int rc = check_grid(what, pl.grid)) return rc;
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.block;
    out8[3] = pl.rows;
    out8[4] = pl.ld;
    out8[5] = pl.lds;
    out8[6] = pl.dynamic;
    out8[7] = pl.store;
    return LSQ_OK;
}

}  // extern "C"
