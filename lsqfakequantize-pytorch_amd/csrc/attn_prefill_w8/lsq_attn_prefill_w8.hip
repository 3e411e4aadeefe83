// lsq_attn_prefill_w8.hip -- prefill attention on 8-bit levels in one launch on gfx950: causal and key-length masked, grouped-query
// (include/lsq_hip_attn_prefill_w8.h, which states the contract): the kernel and the C ABI of liblsq_hip_attn_prefill_w8.so.
//
// attn_fused_w8_kernel's frame with the decode kernel's key counts.  A workgroup of four waves takes one (b, h) and 64 query rows;
// wave w owns rows 16 w .. 16 w + 15 in ALL THREE PHASES, so the score and probability rows in LDS are wave-private.  n(b, t) is
// monotone in t: nmax_wave = n of the wave's last live row, nmax_wg = n of the workgroup's last live row, both from key_lengths[b]
// read here.  k and v are those of kv head h / G; the G heads of a kv head are G workgroups next to each other in the grid and share
// k and v through L2.
//  1 SCORES   as the fused kernel's, over the 16-key sub-tiles below 16 ceil(nmax_wave / 16): nothing above the wave's diagonal is
//             computed.  Keys beyond nmax_wave are clamped to nmax_wave - 1: their bytes are never counted.
//  2 SOFTMAX  in place, a row in the registers of a group of L lanes as in the fused kernel; each row takes max, sum and
//             probabilities over its own prefix n_r.  Bytes in [n_r, 16 ceil(nmax_wave / 16)) become the byte z_p (as in the decode
//             kernel): one K = nmax_wave then serves the raw-sum correction of all 16 rows.
//  3 CONTEXT  v[b, h / G] staged per 64-key step through LDS transposed into [D][80] for the whole workgroup, so the loop has
//             workgroup barriers and its bound is workgroup-uniform: nmax_wg.  A wave skips only its own MFMAs for steps at or
//             beyond its nmax_wave; it still stages and meets every barrier.  Rows of v beyond nmax_wg are not read; within a
//             wave's last step, bytes of p and the ones of the column sums from nmax_wave on are the operand's zero.
//             The epilogue of the fused kernel with K = nmax_wave; the level tile leaves through LDS over the staging area as
//             16-byte packets (byte by byte into a y that is not packet-aligned).
// A workgroup with nmax_wg = 0 runs no key loop: P = C = S = 0 with K = 0 is I = 0, the level of 0.0.
// LDS is not zeroed between workgroups: score packets at and beyond 16 ceil(nmax_wave / 16) are never read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../qlinear_w8/lsq_w8_shared.hpp"
#include "../attn_w8/lsq_attn_w8_dev.hpp"
#include "../attn_w8/lsq_attn_decode_checks.hpp"
#include "../../../include/lsq_hip_attn_prefill_w8.h"

namespace lsq {

typedef __attribute__((ext_vector_type(2))) unsigned short pre_u16x2;

constexpr int kPreRows = LSQ_ATTN_PREFILL_W8_ROWS;  // query rows of a workgroup: four waves of 16
constexpr int kPreStep = 64;                        // keys per step of phase 3
constexpr int kPreVtStride = kPreStep + 16;         // bytes between the rows of the transposed v tile in LDS
constexpr int kPreTable = 1024;
constexpr int kPreMaxSubs = LSQ_ATTN_PREFILL_W8_MAX_D / 16;
static_assert(kBlock == 256, "four waves per workgroup");

constexpr int pre_ld(int Tk_eff) {                  // 16 n, n = ceil(Tk_eff / 16) made odd
    return 16 * (((Tk_eff + 15) / 16) | 1);
}
constexpr int pre_lds(int Tk_eff, int D) { return kPreRows * pre_ld(Tk_eff) + kPreTable + kPreVtStride * D; }
constexpr int kPreMaxLds = pre_lds(LSQ_ATTN_PREFILL_W8_MAX_TK_EFF, LSQ_ATTN_PREFILL_W8_MAX_D);
static_assert(kPreMaxLds <= LSQ_ATTN_PREFILL_W8_MAX_LDS, "the largest served geometry fits the CU's LDS");
static_assert(kPreRows * LSQ_ATTN_PREFILL_W8_MAX_D <= kPreVtStride * LSQ_ATTN_PREFILL_W8_MAX_D, "the level tile fits the staging area");
static_assert(LSQ_ATTN_PREFILL_W8_MAX_TK_EFF <= 2 * 64 * 16, "a row fits two packets per lane of a wave");

struct PreGeom {            // kernel argument
    int64_t q_s0, q_s1, q_ld, k_s0, k_s1, k_ld, v_s0, v_s1, v_ld, y_s0, y_s1, y_ld;
    int H, G, Tq, Tk, D;
    int row_tiles, ld;      // ceil(Tq / 64); bytes between score rows in LDS
    int causal, off;        // row t sees t + 1 + off keys (off clamped to Tk on the host)
};

struct PreArg {             // kernel argument
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
__device__ __forceinline__ int pre_count(const PreGeom& g, int len, int t) {
    int n = min(g.Tk, len);
    if (g.causal) n = min(n, t + 1 + g.off);           // t < 2^20 and off <= Tk <= 65536
    return n;
}

// what one wave writes to LDS its other lanes read next: LDS serves a wave's accesses in order; the compiler must keep it
__device__ __forceinline__ void pre_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(kBlock) void attn_prefill_w8_kernel(PreGeom g, PreArg a, AttnOut so, AttnOut po, AttnOut co,
                                                                 const int32_t* __restrict__ table, const int32_t* __restrict__ lens,
                                                                 const uint8_t* __restrict__ Q, const uint8_t* __restrict__ K,
                                                                 const uint8_t* __restrict__ V, uint8_t* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* sc = lds;                                            // [64][ld]: score bytes, then probability bytes
    int32_t* tab = reinterpret_cast<int32_t*>(lds + kPreRows * g.ld);   // [256]
    unsigned char* stage = lds + kPreRows * g.ld + kPreTable;           // v transposed [D][80]; then the level tile [64][D]
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    const int rt = static_cast<int>(blockIdx.x % g.row_tiles);
    const int64_t batch = static_cast<int64_t>(blockIdx.x / g.row_tiles);
    const int64_t b0 = batch / g.H, b1 = batch - b0 * g.H, bkv = b1 / g.G;
    const int m0 = rt * kPreRows;
    const bool wave_live = m0 + wave * 16 < g.Tq;                       // the same for the whole wave
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const int len = lens ? max(lens[b0], 0) : g.Tk;
    // n is monotone in t: the last live row of the workgroup and of the wave have the largest
    const int nmax_wg = pre_count(g, len, min(m0 + kPreRows, g.Tq) - 1);                  // the same for the whole workgroup
    const int nmax_wave = wave_live ? pre_count(g, len, min(m0 + wave * 16 + 16, g.Tq) - 1) : 0;    // the same for the whole wave, <= nmax_wg
    const int nsub = (nmax_wave + 15) >> 4;                             // 16-key sub-tiles below nmax_wave, and the packets of a row that count
    unsigned char* myrow = sc + (wave * 16 + nl) * g.ld;                // the row this lane reads as the A operand in phase 3

    tab[tid] = table[tid];
    __syncthreads();

    if (nsub > 0) {                                                     // the same for the whole wave; no workgroup barrier inside
        // ---------------------------------------------------------------------------------------- phase 1: the scores
        const uint32_t flip_q = a.off_q ? 0x80808080u : 0u, flip_k = a.off_k ? 0x80808080u : 0u;
        // a clamped row computes values nobody stores
        const uint8_t* __restrict__ qrow = Q + b0 * g.q_s0 + b1 * g.q_s1 + static_cast<int64_t>(min(m0 + wave * 16 + nl, g.Tq - 1)) * g.q_ld;
        const uint8_t* __restrict__ Kb = K + b0 * g.k_s0 + bkv * g.k_s1;
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
        u32x4 cur[2], nxt[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int kk = 64 * s + 16 * q;
            cur[s] = u32x4{0u, 0u, 0u, 0u};
            // nmax_wave >= 1 here: the clamped key is a key below nmax_wave
            if (kk < g.D) cur[s] = *reinterpret_cast<const u32x4*>(Kb + static_cast<int64_t>(min(nl, nmax_wave - 1)) * g.k_ld + kk) ^ flip_k;
            nxt[s] = cur[s];
        }
        for (int j = 0; j < nsub; ++j) {
            if (j + 1 < nsub) {                                         // the next sub-tile's rows are in flight during this one's epilogue
                const uint8_t* __restrict__ kr = Kb + static_cast<int64_t>(min(16 * (j + 1) + nl, nmax_wave - 1)) * g.k_ld;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int kk = 64 * s + 16 * q;
                    if (kk < g.D) nxt[s] = *reinterpret_cast<const u32x4*>(kr + kk) ^ flip_k;
                }
            }
            i32x4 P = {0, 0, 0, 0}, Cs = {0, 0, 0, 0};
            const i32x4 k0 = w8_as_i32(cur[0]);
            P = __builtin_amdgcn_mfma_i32_16x16x64_i8(qi[0], k0, P, 0, 0, 0);
            Cs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, k0, Cs, 0, 0, 0);       // sum_k k of the lane's key, in every register
            if (two) {
                const i32x4 k1 = w8_as_i32(cur[1]);
                P = __builtin_amdgcn_mfma_i32_16x16x64_i8(qi[1], k1, P, 0, 0, 0);
                Cs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, k1, Cs, 0, 0, 0);
            }
            // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register; 16 j + nl < 16 nsub <= ld
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float u = bmm_value(bmm_int_float(ex, P[i], Cs[i], Rs[i]), s_q, s_k, sq.mid);
                sc[(wave * 16 + 4 * q + i) * g.ld + 16 * j + nl] = static_cast<unsigned char>(w8o_byte(u, sq));
            }
            cur[0] = nxt[0];
            cur[1] = nxt[1];
        }
        pre_wave_sync();

        // ---------------------------------------------------------------------------------------- phase 2: the softmax, in place
        const uint32_t flip_s = a.off_s ? 0u : 0x80808080u;             // int8 levels are biased by 128 on load
        const AttnQ pq = attn_constants(po);
        const uint32_t zb = static_cast<uint32_t>(a.z_p[0]) & 0xffu;    // the byte z_p
        int L = 4, lsh = 2;                                             // the lanes of a row's group
        while (L < nsub && L < 64) {
            L <<= 1;
            ++lsh;
        }
        const int RG = 64 >> lsh, lg = lane & (L - 1), grp = lane >> lsh;      // RG rows at a time
        const bool second = nsub > L;                                   // a second packet per lane: above 1024 keys only; the same for the whole wave
        for (int r0 = 0; r0 < 16; r0 += RG) {                           // the same for the whole wave
            unsigned char* row = sc + (wave * 16 + r0 + grp) * g.ld;
            // this row's prefix; a row beyond Tq takes the last row's (nobody stores it); 1 <= n <= nmax_wave
            const int n = pre_count(g, len, min(m0 + wave * 16 + r0 + grp, g.Tq - 1));
            u32x4 v[2];
            pre_u16x2 me = {0, 0}, mo = {0, 0};
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int p = lg + jj * L;
                v[jj] = u32x4{0u, 0u, 0u, 0u};
                if (jj && !second) continue;
                // clamped: always a packet phase 1 wrote; bytes from n on (and whole packets beyond) count as 0, the least biased byte
                v[jj] = attn_mask_tail(*reinterpret_cast<const u32x4*>(row + 16 * min(p, nsub - 1)) ^ flip_s, p < nsub ? n - 16 * p : 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    me = __builtin_elementwise_max(me, __builtin_bit_cast(pre_u16x2, v[jj][i] & 0x00ff00ffu));
                    mo = __builtin_elementwise_max(mo, __builtin_bit_cast(pre_u16x2, (v[jj][i] >> 8) & 0x00ff00ffu));
                }
            }
            me = __builtin_elementwise_max(me, mo);
            int m = max(static_cast<int>(me[0]), static_cast<int>(me[1]));
            for (int s = L >> 1; s >= 1; s >>= 1) m = max(m, __shfl_xor(m, s));
            // the sum: at most 32 entries of at most 2^24 per lane fit 32 bits; 64 across lanes
            uint32_t part = 0;
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                if (jj && !second) continue;
                const int valid = min(max(n - 16 * (lg + jj * L), 0), 16);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int b = static_cast<int>((v[jj][i / 4] >> (8 * (i % 4))) & 0xffu);
                    part += i < valid ? static_cast<uint32_t>(tab[(m - b) & 0xff]) : 0u;
                }
            }
            uint64_t S = part;
            for (int s = L >> 1; s >= 1; s >>= 1) S += smx_shfl_xor_u64(S, s);
            float r = 0.0f;
            if (n > 0) r = __fdiv_rn(1.0f, static_cast<float>(S));     // n = 0: nothing is divided and no p is formed
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                if (jj && !second) continue;
                const int p = lg + jj * L;
                const int valid = min(max(n - 16 * p, 0), 16);
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int b = static_cast<int>((v[jj][i / 4] >> (8 * (i % 4))) & 0xffu);
                    const uint32_t pb = w8o_byte(smx_value(tab[(m - b) & 0xff], r, pq.mid), pq);
                    w[i / 4] |= (i < valid ? pb : zb) << (8 * (i % 4));         // the byte z_p from n on
                }
                if (p < nsub) *reinterpret_cast<u32x4*>(row + 16 * p) = u32x4{w[0], w[1], w[2], w[3]};
            }
        }
        pre_wave_sync();
    }

    // -------------------------------------------------------------------------------------------- phase 3: the context
    const uint32_t flip_p = a.off_p ? 0x80808080u : 0u, flip_v = a.off_v ? 0x80808080u : 0u;
    const uint8_t* __restrict__ Vb = V + b0 * g.v_s0 + bkv * g.v_s1;
    const int subs = g.D >> 4;                                          // 16-column sub-tiles of the context, 1 .. 8
    i32x4 P[kPreMaxSubs], Cs[kPreMaxSubs], Rs = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < kPreMaxSubs; ++j) {
        P[j] = i32x4{0, 0, 0, 0};
        Cs[j] = i32x4{0, 0, 0, 0};
    }
    // THE BOUND IS nmax_wg, the same for every thread of the workgroup: both barriers of a step are met by all four waves
    for (int k0 = 0; k0 < nmax_wg; k0 += kPreStep) {
        const int kk = k0 + q * 16;
        const bool mine = k0 < nmax_wave;                               // the same for the whole wave; false for a wave beyond Tq
        u32x4 av = {0u, 0u, 0u, 0u}, on = {0u, 0u, 0u, 0u};
        if (kk < nmax_wave) {                                           // a packet below 16 nsub, its tail beyond nmax_wave the operand's zero
            av = attn_mask_tail(*reinterpret_cast<const u32x4*>(myrow + kk) ^ flip_p, nmax_wave - kk);
            on = attn_mask_tail(u32x4{0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u}, nmax_wave - kk);
        }
        __syncthreads();                                                // the previous step's reads of the staging area are done
        const int kg = tid >> 4, d = tid & 15;                          // four k rows 4 kg .., the word of columns 4 d .. (+ 64)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = 64 * h + 4 * d;
            if (n < g.D) {
                uint32_t r[4], c[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + 4 * kg + i;
                    r[i] = 0u;                                          // a row at or beyond nmax_wg is not read: the operand's zero
                    if (k < nmax_wg) r[i] = *reinterpret_cast<const uint32_t*>(Vb + static_cast<int64_t>(k) * g.v_ld + n) ^ flip_v;
                }
                attn_transpose4(r[0], r[1], r[2], r[3], c);
#pragma unroll
                for (int i = 0; i < 4; ++i) *reinterpret_cast<uint32_t*>(stage + (n + i) * kPreVtStride + 4 * kg) = c[i];
            }
        }
        __syncthreads();
        if (mine) {                                                     // only MFMAs inside: no barrier is skipped
            const i32x4 ai = w8_as_i32(av), oi = w8_as_i32(on);
#pragma unroll
            for (int j = 0; j < kPreMaxSubs; ++j) {
                if (j < subs) {                                         // the same for the whole grid
                    const i32x4 bi = w8_as_i32(*reinterpret_cast<const u32x4*>(stage + (16 * j + nl) * kPreVtStride + q * 16));
                    P[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ai, bi, P[j], 0, 0, 0);
                    Cs[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(oi, bi, Cs[j], 0, 0, 0);  // sum of v over the keys below nmax_wave
                }
            }
            Rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ai, ones, Rs, 0, 0, 0);
        }
    }

    const AttnQ oq = attn_constants(co);
    const BmmInt ex = bmm_int_constants(static_cast<int64_t>(a.z_p[0]) - a.off_p, static_cast<int64_t>(a.z_v[0]) - a.off_v, nmax_wave);
    const float s_p = a.s_p[0], s_v = a.s_v[0];
    __syncthreads();                                                    // the last step's reads of the staging area are done
    if (wave_live) {
#pragma unroll
        for (int j = 0; j < kPreMaxSubs; ++j) {
            if (j >= subs) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float u = bmm_value(bmm_int_float(ex, P[j][i], Cs[j][i], Rs[i]), s_p, s_v, oq.mid);
                stage[(wave * 16 + 4 * q + i) * g.D + 16 * j + nl] = static_cast<unsigned char>(w8o_byte(u, oq));
            }
        }
    }
    __syncthreads();
    uint8_t* __restrict__ yb = y + b0 * g.y_s0 + b1 * g.y_s1;
    const int per_row = subs, total = kPreRows * per_row;               // 16-byte packets of the tile
    for (int idx = tid; idx < total; idx += kBlock) {
        const int r = idx / per_row, c = (idx - r * per_row) * 16;
        if (m0 + r >= g.Tq) continue;
        uint8_t* dst = yb + static_cast<int64_t>(m0 + r) * g.y_ld + c;
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
struct PrePlan {
    int family, block, rows, ld, lds, dynamic, store;
    int64_t grid;
    PreGeom g;
};

inline PrePlan plan_prefill(const lsq_attn_decode_w8_geom& ge, bool qkv_aligned, bool y_aligned) {
    PrePlan pl = {};
    pl.family = LSQ_ATTN_PREFILL_W8_COMPOSITION;
    const int64_t off = ge.causal ? std::min<int64_t>(ge.causal_offset, ge.Tk) : 0;
    // the largest key count any row can have as the host knows it
    const int64_t tk_eff = ge.causal ? std::min<int64_t>(ge.Tk, ge.Tq + off) : ge.Tk;
    if (!(qkv_aligned && strides16(ge.q) && strides16(ge.k) && strides16(ge.v) && ge.D % 16 == 0 && ge.D >= 16 &&
          ge.D <= LSQ_ATTN_PREFILL_W8_MAX_D && tk_eff <= LSQ_ATTN_PREFILL_W8_MAX_TK_EFF))
        return pl;
    const int D = static_cast<int>(ge.D);
    pl.family = LSQ_ATTN_PREFILL_W8_PREFILL;
    pl.block = kBlock;
    pl.rows = kPreRows;
    pl.ld = pre_ld(static_cast<int>(tk_eff));
    pl.lds = pre_lds(static_cast<int>(tk_eff), D);
    pl.dynamic = pl.lds > 65536 ? 1 : 0;
    pl.store = y_aligned && strides16(ge.y) ? LSQ_ATTN_W8_STORE_PACKETS : LSQ_ATTN_W8_STORE_ELEMS;
    const int64_t row_tiles = ceil_div(ge.Tq, kPreRows);
    pl.grid = ge.B * ge.H * row_tiles;
    pl.g = PreGeom{ge.q.s0, ge.q.s1, ge.q.ld, ge.k.s0, ge.k.s1, ge.k.ld, ge.v.s0, ge.v.s1, ge.v.ld, ge.y.s0, ge.y.s1, ge.y.ld,
                   static_cast<int>(ge.H), static_cast<int>(ge.H / ge.Hkv), static_cast<int>(ge.Tq), static_cast<int>(ge.Tk), D,
                   static_cast<int>(row_tiles), pl.ld, ge.causal ? 1 : 0, static_cast<int>(off)};
    return pl;
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_attn_prefill_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
extern "C" {

int lsq_attn_prefill_w8_abi_version(void) { return LSQ_ATTN_PREFILL_W8_ABI_VERSION; }

const char* lsq_attn_prefill_w8_last_error(void) { return g_last_error; }

int lsq_attn_prefill_w8(const lsq_attn_decode_w8_geom* geom, const lsq_attn_decode_w8_consts* consts, const lsq_attn_w8_out* scores_out,
                        const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out, const void* table, const void* key_lengths,
                        const void* q_levels, const void* k_levels, const void* v_levels, void* y, void* stream) {
    const char* what = "lsq_attn_prefill_w8";
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
    const lsq::PrePlan pl = lsq::plan_prefill(*geom, aligned_to(q_levels, 16) && aligned_to(k_levels, 16) && aligned_to(v_levels, 16),
                                              aligned_to(y, 16));
    if (pl.family != LSQ_ATTN_PREFILL_W8_PREFILL)
        return fail(LSQ_EINVAL, "%s: [B, H, Hkv, Tq, Tk, D] = [%lld, %lld, %lld, %lld, %lld, %lld] with this mask, these bases and strides is "
                    "not served by the prefill kernel (q, k, v 16-byte aligned with strides that are multiples of 16, D %% 16 == 0, "
                    "16 <= D <= %d, min(Tk, Tq + causal_offset) where causal, else Tk, <= %d): compose lsq_hip_attn_w8.h and "
                    "lsq_hip_attn_mask_w8.h", what, static_cast<ll>(geom->B), static_cast<ll>(geom->H), static_cast<ll>(geom->Hkv),
                    static_cast<ll>(geom->Tq), static_cast<ll>(geom->Tk), static_cast<ll>(geom->D), LSQ_ATTN_PREFILL_W8_MAX_D,
                    LSQ_ATTN_PREFILL_W8_MAX_TK_EFF);
    if (int rc = check_grid(what, pl.grid)) return rc;
    if (pl.dynamic) {
        static lsq::LdsOnce once;
        if (int rc = hip_status(lsq::allow_lds(once, reinterpret_cast<const void*>(lsq::attn_prefill_w8_kernel), lsq::kPreMaxLds), what)) return rc;
    }
    const lsq::PreArg arg{static_cast<const float*>(consts->s_q), static_cast<const int32_t*>(consts->z_q),
                          static_cast<const float*>(consts->s_k), static_cast<const int32_t*>(consts->z_k),
                          static_cast<const float*>(consts->s_v), static_cast<const int32_t*>(consts->z_v),
                          static_cast<const float*>(consts->s_p), static_cast<const int32_t*>(consts->z_p),
                          geom->q_dtype == LSQ_ATTN_W8_U8 ? 128 : 0, geom->k_dtype == LSQ_ATTN_W8_U8 ? 128 : 0,
                          geom->v_dtype == LSQ_ATTN_W8_U8 ? 128 : 0, side_off(scores_out), side_off(probs_out),
                          pl.store == LSQ_ATTN_W8_STORE_PACKETS ? 1 : 0};
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kBlock);
    hipLaunchKernelGGL(lsq::attn_prefill_w8_kernel, grid, block, static_cast<size_t>(pl.lds), static_cast<hipStream_t>(stream), pl.g, arg, so,
                       po, co, static_cast<const int32_t*>(table), static_cast<const int32_t*>(key_lengths),
                       static_cast<const uint8_t*>(q_levels), static_cast<const uint8_t*>(k_levels), static_cast<const uint8_t*>(v_levels),
                       static_cast<uint8_t*>(y));
    return hip_status(hipGetLastError(), what);
}

int lsq_attn_prefill_w8_plan(const lsq_attn_decode_w8_geom* geom, int qkv_aligned, int y_aligned, int32_t* out8) {
    const char* what = "lsq_attn_prefill_w8_plan";
    if (int rc = check_decode_geom(what, geom)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::PrePlan pl = lsq::plan_prefill(*geom, qkv_aligned != 0, y_aligned != 0);
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
