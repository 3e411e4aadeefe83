// lsq_attn_w8.hip -- the attention core on 8-bit levels on gfx950 (include/lsq_hip_attn_w8.h, which states the contract): the
// kernels and the C ABI of liblsq_hip_attn_w8.so.
//
// BATCHED MATMUL
//  * MFMA (bases and strides of A and B multiples of 16): a workgroup of four waves takes one batch and a 64 x 64 tile of y; wave w
//    owns rows 16 w .. 16 w + 15 and all four 16-column sub-tiles, and walks K in steps of 64 with v_mfma_i32_16x16x64_i8.  A's
//    packet comes straight from memory (row lane & 15, bytes 16 (lane >> 4) ..).  NT: so do B's four.  NN: the step's [64 k, 64 n]
//    bytes of B are staged through LDS transposed -- a thread loads the same word of four consecutive k rows, transposes the
//    4 x 4 block of bytes with eight v_perm_b32 and writes four words -- and every wave reads its B packets from there.  The
//    bytes of a last partial packet are masked to the operand's zero byte in registers; rows beyond M, N (clamped) and beyond
//    NN's K (zero) cost nothing but their lanes.  sum_k a per row and sum_k b per column come from the same packets against
//    0x01010101 on the matrix core, in the accumulator's layout: no LDS, no shuffles.  Levels leave through LDS as a 64 x 64 byte
//    tile, one 16-byte packet per thread; floats leave from the accumulator's layout (16 adjacent columns per 16 lanes).
//  * GENERIC (every other legal call): a thread per output, a 64-bit sum over k.  Correct, not tuned.
// SOFTMAX
//  * PACKETS (C <= 8192, bases and ldx, ldy multiples of 16): a row lives in the registers of a group of L lanes, P packets per lane,
//    read once; the tail bytes of the last packet take no part.  The byte max goes through the packed 16-bit max (even and odd
//    bytes; int8 biased by 0x80), then __shfl_xor; E = table[m - b] from the 1 KB table in LDS; a lane's partial sum is 32 bits
//    (at most 128 entries of 2^24: 2^31), widened to 64 before it crosses lanes.  No barrier but the one after staging the table.
//  * GENERIC: one wave per row, three passes over its bytes, the table from memory.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../qlinear_w8/lsq_w8_shared.hpp"
#include "lsq_attn_w8_dev.hpp"
#include "lsq_attn_w8_checks.hpp"
#include "../../../include/lsq_hip_attn_w8.h"

namespace lsq {

typedef __attribute__((ext_vector_type(2))) unsigned short attn_u16x2;

constexpr int kAttnTile = 64;                   // rows and columns of a workgroup's tile, and the K step
constexpr int kAttnBtStride = kAttnTile + 16;   // bytes between the rows of the transposed B tile in LDS
constexpr int kAttnLds = kAttnTile * kAttnBtStride;
constexpr int kSmxMaxP = 8;
constexpr int kSmxWave = 64;
constexpr int kSmxRows = 4;                     // rows a group walks where the grid stays large
constexpr int64_t kSmxFill = 512;               // ... that is: at least this many workgroups
static_assert(kBlock == 256, "four waves per workgroup");

// ------------------------------------------------------------------------------------------------
// batched matmul
// ------------------------------------------------------------------------------------------------
struct BmmGeom {            // kernel argument
    int64_t a_s0, a_s1, a_ld, b_s0, b_s1, b_ld, y_s0, y_s1, y_ld;
    int B1, M, N, K;
    int row_tiles, col_tiles;
};

struct BmmArg {             // kernel argument
    const float* s_a;
    const int32_t* z_a;
    const float* s_b;
    const int32_t* z_b;
    int off_a, off_b;       // 128: uint8 levels (the byte ^ 0x80 read as int8 is the level - 128); 0: int8
    int y_packets;          // levels out: y's base and strides are multiples of 16
};

template <bool NN>
__global__ __launch_bounds__(kBlock) void bmm_w8_mfma_kernel(BmmGeom g, BmmArg a, AttnOut o, const uint8_t* __restrict__ A,
                                                             const uint8_t* __restrict__ B, void* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kAttnLds];   // NN: B transposed [64 n][80]; then the level tile [64][64]
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nl = lane & 15, q = lane >> 4;
    int64_t t = static_cast<int64_t>(blockIdx.x);
    const int ct = static_cast<int>(t % g.col_tiles);
    t /= g.col_tiles;
    const int rt = static_cast<int>(t % g.row_tiles);
    const int64_t batch = t / g.row_tiles;
    const int64_t b0 = batch / g.B1, b1 = batch - b0 * g.B1;
    const int m0 = rt * kAttnTile, n0 = ct * kAttnTile;
    const uint32_t flip_a = a.off_a ? 0x80808080u : 0u, flip_b = a.off_b ? 0x80808080u : 0u;
    const uint8_t* __restrict__ Bb = B + b0 * g.b_s0 + b1 * g.b_s1;
    // a clamped row computes values nobody stores
    const uint8_t* __restrict__ arow = A + b0 * g.a_s0 + b1 * g.a_s1 + static_cast<int64_t>(min(m0 + wave * 16 + nl, g.M - 1)) * g.a_ld;
    const uint8_t* brow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) brow[j] = Bb + (NN ? 0 : static_cast<int64_t>(min(n0 + 16 * j + nl, g.N - 1)) * g.b_ld);
    const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    i32x4 P[4], Cs[4], Rs = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        P[j] = i32x4{0, 0, 0, 0};
        Cs[j] = i32x4{0, 0, 0, 0};
    }

    // rows 192 .. 255 of a 197-row matrix: a wave whose 16 rows all lie beyond M, and a 16-column sub-tile beyond N, load and
    // multiply nothing (they still stage NN's B and meet the barriers)
    const bool wave_live = m0 + wave * 16 < g.M;
    for (int k0 = 0; k0 < g.K; k0 += kAttnTile) {       // the same for the whole workgroup
        const int kk = k0 + q * 16;
        u32x4 av = {0u, 0u, 0u, 0u};
        if (wave_live && kk < g.K) av = attn_mask_tail(*reinterpret_cast<const u32x4*>(arow + kk) ^ flip_a, g.K - kk);
        if constexpr (NN) {
            __syncthreads();                            // the previous step's reads of LDS are done
            const int kg = tid >> 4, d = tid & 15;      // four k rows 4 kg .., the word of columns 4 d ..
            const int n = n0 + 4 * d;
            uint32_t r[4], c[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = k0 + 4 * kg + i;
                r[i] = 0u;                              // a row beyond K and a word beyond N: the operand's zero
                if (k < g.K && n < g.N) r[i] = *reinterpret_cast<const uint32_t*>(Bb + static_cast<int64_t>(k) * g.b_ld + n) ^ flip_b;
            }
            attn_transpose4(r[0], r[1], r[2], r[3], c);
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<uint32_t*>(lds + (4 * d + i) * kAttnBtStride + 4 * kg) = c[i];
            __syncthreads();
        }
        if (wave_live) {                                // the same for the whole wave
            const i32x4 ai = w8_as_i32(av);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (n0 + 16 * j < g.N) {                // the same for the whole workgroup
                    u32x4 bv = {0u, 0u, 0u, 0u};
                    if constexpr (NN) bv = *reinterpret_cast<const u32x4*>(lds + (16 * j + nl) * kAttnBtStride + q * 16);
                    else if (kk < g.K) bv = attn_mask_tail(*reinterpret_cast<const u32x4*>(brow[j] + kk) ^ flip_b, g.K - kk);
                    const i32x4 bi = w8_as_i32(bv);
                    P[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ai, bi, P[j], 0, 0, 0);
                    Cs[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bi, Cs[j], 0, 0, 0);   // sum_k b of the lane's column, in every register
                }
            }
            Rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ai, ones, Rs, 0, 0, 0);              // sum_k a of row 4 q + i in register i
        }
    }

    // D of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
    const AttnQ oq = attn_constants(o);
    // 64 bits from the first subtraction on: no zero point, however far outside the level range, overflows a signed step
    const int64_t z_a = static_cast<int64_t>(a.z_a[0]) - a.off_a, z_b = static_cast<int64_t>(a.z_b[0]) - a.off_b;
    const float s_a = a.s_a[0], s_b = a.s_b[0];
    uint8_t* yb = static_cast<uint8_t*>(y);
    const int64_t ybase = b0 * g.y_s0 + b1 * g.y_s1;
    if constexpr (NN) __syncthreads();                  // the last step's reads of LDS are done
    // |I| <= K max|la - za| max|lb - zb|: where that stays below 2^31 (every K up to 32768 with zero points inside the level
    // ranges) the four terms are summed in 32 wrapping bits and converted with one instruction; the value is the same integer
    // (lsq_attn_w8_dev.hpp's bmm_int_constants / bmm_int_float state the same selection for the fused kernel; called from here they
    // change this kernel's register allocation and compare senses, so it keeps its own text: profiles/r24_attn_w8_shared_isa_diff.txt)
    const int64_t reach_a = max(z_a + 128, 127 - z_a), reach_b = max(z_b + 128, 127 - z_b);        // max |a - z| over a in -128..127
    const bool narrow = reach_a < 65536 && reach_b < 65536 && g.K * reach_a * reach_b < (int64_t{1} << 31);
    const uint32_t kzz = static_cast<uint32_t>(g.K) * static_cast<uint32_t>(z_a) * static_cast<uint32_t>(z_b);
    if (wave_live) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n0 + 16 * j >= g.N) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = wave * 16 + 4 * q + i, c = 16 * j + nl;
                float fI;
                if (narrow) {
                    const uint32_t I32 = static_cast<uint32_t>(P[j][i]) - static_cast<uint32_t>(z_a) * static_cast<uint32_t>(Cs[j][i]) -
                                         static_cast<uint32_t>(z_b) * static_cast<uint32_t>(Rs[i]) + kzz;
                    fI = static_cast<float>(static_cast<int32_t>(I32));
                } else {
                    fI = static_cast<float>(bmm_exact(P[j][i], Cs[j][i], Rs[i], g.K, z_a, z_b));
                }
                const float u = bmm_value(fI, s_a, s_b, oq.mid);
                if (oq.levels_out) lds[r * kAttnTile + c] = static_cast<unsigned char>(w8o_byte(u, oq));
                else if (m0 + r < g.M && n0 + c < g.N) w8o_store_float(y, ybase + static_cast<int64_t>(m0 + r) * g.y_ld + n0 + c, u, oq.mid);
            }
        }
    }
    if (!oq.levels_out) return;                         // the same for the whole grid
    __syncthreads();
    const int r = tid >> 2, c = (tid & 3) * 16;
    const int m = m0 + r, n = n0 + c;
    if (m >= g.M || n >= g.N) return;
    uint8_t* dst = yb + ybase + static_cast<int64_t>(m) * g.y_ld + n;
    if (a.y_packets && n + 16 <= g.N) {
        *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(lds + r * kAttnTile + c);
    } else {
        const int cnt = min(16, g.N - n);
        for (int i = 0; i < cnt; ++i) dst[i] = lds[r * kAttnTile + c + i];
    }
}

// a thread per output
__global__ __launch_bounds__(kBlock) void bmm_w8_generic_kernel(BmmGeom g, BmmArg a, AttnOut o, int nn, int64_t total,
                                                                const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                                void* __restrict__ y) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (idx >= total) return;
    const int n = static_cast<int>(idx % g.N);
    int64_t t = idx / g.N;
    const int m = static_cast<int>(t % g.M);
    const int64_t batch = t / g.M;
    const int64_t b0 = batch / g.B1, b1 = batch - b0 * g.B1;
    const uint8_t* __restrict__ ap = A + b0 * g.a_s0 + b1 * g.a_s1 + static_cast<int64_t>(m) * g.a_ld;
    const uint8_t* __restrict__ bp = B + b0 * g.b_s0 + b1 * g.b_s1 + (nn ? static_cast<int64_t>(n) : static_cast<int64_t>(n) * g.b_ld);
    const int64_t bstep = nn ? g.b_ld : 1;
    const int64_t z_a = a.z_a[0], z_b = a.z_b[0];
    int64_t I = 0;
    for (int k = 0; k < g.K; ++k) {
        const int la = a.off_a ? static_cast<int>(ap[k]) : static_cast<int>(static_cast<int8_t>(ap[k]));
        const uint8_t raw = bp[k * bstep];
        const int lb = a.off_b ? static_cast<int>(raw) : static_cast<int>(static_cast<int8_t>(raw));
        I = static_cast<int64_t>(static_cast<uint64_t>(I) + static_cast<uint64_t>(la - z_a) * static_cast<uint64_t>(lb - z_b));    // wraps, never overflows
    }
    const AttnQ oq = attn_constants(o);
    const float u = bmm_value(I, a.s_a[0], a.s_b[0], oq.mid);
    const int64_t at = b0 * g.y_s0 + b1 * g.y_s1 + static_cast<int64_t>(m) * g.y_ld + n;
    // w8o_store1's two lines, written out here, in smx_store16 and in softmax_w8_generic_kernel: called as one function they change
    // this kernel's branch senses and the register allocation of the softmax packet kernels (profiles/r25_w8_out_side_isa_diff.txt)
    if (oq.levels_out) static_cast<uint8_t*>(y)[at] = static_cast<uint8_t>(w8o_byte(u, oq));
    else w8o_store_float(y, at, u, oq.mid);
}

// ------------------------------------------------------------------------------------------------
// softmax
// ------------------------------------------------------------------------------------------------
struct SmxGeom {            // kernel argument
    int64_t R, ldx, ldy;
    int C, packets, K;      // elements of a row, ceil(C / 16), rows per group
    uint32_t flip;          // 0x80808080 for int8 levels (biased by 128 on load), 0 for uint8
};

// a packet of outputs, the first `cnt` of them stored: `at` in elements of y; y 16-byte aligned, at % 16 == 0
__device__ __forceinline__ void smx_store16(void* y, int64_t at, const float (&u)[16], int cnt, const AttnQ& q) {
    if (cnt >= 16 && q.levels_out) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[i] = w8o_byte(u[4 * i], q) | w8o_byte(u[4 * i + 1], q) << 8 | w8o_byte(u[4 * i + 2], q) << 16 | w8o_byte(u[4 * i + 3], q) << 24;
        *reinterpret_cast<u32x4*>(static_cast<uint8_t*>(y) + at) = u32x4{w[0], w[1], w[2], w[3]};
    } else if (cnt >= 16 && q.mid == LSQ_F32) {
        u32x4* out = reinterpret_cast<u32x4*>(static_cast<float*>(y) + at);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            out[i] = u32x4{__float_as_uint(u[4 * i]), __float_as_uint(u[4 * i + 1]), __float_as_uint(u[4 * i + 2]), __float_as_uint(u[4 * i + 3])};
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < cnt) {
                if (q.levels_out) static_cast<uint8_t*>(y)[at + i] = static_cast<uint8_t>(w8o_byte(u[i], q));
                else w8o_store_float(y, at + i, u[i], q.mid);
            }
        }
    }
}

// Workgroup b serves the rows [b G K, (b + 1) G K), G = kBlock / L groups: group g takes b G K + g + k G, k < K.  Lane l of a
// group holds the row's packets l + j L, j < P.
template <int L, int P>
__global__ __launch_bounds__(kBlock) void softmax_w8_packets_kernel(SmxGeom g, AttnOut o, const int32_t* __restrict__ table,
                                                                    const uint8_t* __restrict__ x, void* __restrict__ y) {
    constexpr int G = kBlock / L;
    __shared__ int32_t tab[256];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & (L - 1), grp = tid / L;
    tab[tid] = table[tid];
    const AttnQ q = attn_constants(o);
    __syncthreads();
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (G * g.K) + grp;
    for (int k = 0; k < g.K; ++k) {
        // a group past the last row recomputes the last row and stores nothing: every lane of the wave takes part in the exchange
        const int64_t row = first + static_cast<int64_t>(k) * G;
        const bool live = row < g.R;
        const int64_t rr = live ? row : g.R - 1;
        const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(x + rr * g.ldx);
        u32x4 v[P];
#pragma unroll
        for (int j = 0; j < P; ++j) v[j] = src[min(lane + j * L, g.packets - 1)];       // clamped: always a packet of the row
#pragma unroll
        for (int j = 0; j < P; ++j) asm volatile("" : "+v"(v[j]));                      // all in flight at once
        // the byte max: bytes beyond C (and whole packets beyond the row) count as 0, the least biased byte
        attn_u16x2 me = {0, 0}, mo = {0, 0};
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int p = lane + j * L;
            v[j] = attn_mask_tail(v[j] ^ g.flip, p < g.packets ? g.C - 16 * p : 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                me = __builtin_elementwise_max(me, __builtin_bit_cast(attn_u16x2, v[j][i] & 0x00ff00ffu));
                mo = __builtin_elementwise_max(mo, __builtin_bit_cast(attn_u16x2, (v[j][i] >> 8) & 0x00ff00ffu));
            }
        }
        me = __builtin_elementwise_max(me, mo);
        int m = max(static_cast<int>(me[0]), static_cast<int>(me[1]));
#pragma unroll
        for (int s = L / 2; s >= 1; s /= 2) m = max(m, __shfl_xor(m, s));
        // the sum: at most 128 entries of at most 2^24 per lane fit 32 bits; 64 across lanes
        uint32_t part = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int valid = min(max(g.C - 16 * (lane + j * L), 0), 16);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int b = static_cast<int>((v[j][i / 4] >> (8 * (i % 4))) & 0xffu);
                part += i < valid ? static_cast<uint32_t>(tab[(m - b) & 0xff]) : 0u;
            }
        }
        uint64_t S = part;
#pragma unroll
        for (int s = L / 2; s >= 1; s /= 2) S += smx_shfl_xor_u64(S, s);
        const float r = __fdiv_rn(1.0f, static_cast<float>(S));
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int p = lane + j * L;
            const int valid = min(max(g.C - 16 * p, 0), 16);
            float u[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int b = static_cast<int>((v[j][i / 4] >> (8 * (i % 4))) & 0xffu);
                u[i] = smx_value(tab[(m - b) & 0xff], r, q.mid);
            }
            if (live && valid > 0) smx_store16(y, rr * g.ldy + 16 * static_cast<int64_t>(p), u, valid, q);
        }
    }
}

// one wave per row: lane l takes the bytes l, l + 64, ... in all three passes
__global__ __launch_bounds__(kBlock) void softmax_w8_generic_kernel(SmxGeom g, AttnOut o, const int32_t* __restrict__ table,
                                                                    const uint8_t* __restrict__ x, void* __restrict__ y) {
    const int lane = static_cast<int>(threadIdx.x) & (kSmxWave - 1);
    const int64_t row = static_cast<int64_t>(blockIdx.x) * (kBlock / kSmxWave) + static_cast<int>(threadIdx.x) / kSmxWave;
    if (row >= g.R) return;                        // a whole wave leaves
    const AttnQ q = attn_constants(o);
    const uint8_t* __restrict__ src = x + row * g.ldx;
    const uint32_t flip = g.flip & 0xffu;
    int m = 0;
    for (int i = lane; i < g.C; i += kSmxWave) m = max(m, static_cast<int>(static_cast<uint32_t>(src[i]) ^ flip));
#pragma unroll
    for (int s = kSmxWave / 2; s >= 1; s /= 2) m = max(m, __shfl_xor(m, s));
    uint64_t S = 0;
    for (int i = lane; i < g.C; i += kSmxWave) S += static_cast<uint32_t>(table[(m - static_cast<int>(static_cast<uint32_t>(src[i]) ^ flip)) & 0xff]);
#pragma unroll
    for (int s = kSmxWave / 2; s >= 1; s /= 2) S += smx_shfl_xor_u64(S, s);
    const float r = __fdiv_rn(1.0f, static_cast<float>(S));
    for (int i = lane; i < g.C; i += kSmxWave) {
        const float u = smx_value(table[(m - static_cast<int>(static_cast<uint32_t>(src[i]) ^ flip)) & 0xff], r, q.mid);
        const int64_t at = row * g.ldy + i;
        if (q.levels_out) static_cast<uint8_t*>(y)[at] = static_cast<uint8_t>(w8o_byte(u, q));
        else w8o_store_float(y, at, u, q.mid);
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plans
// ------------------------------------------------------------------------------------------------
struct BmmPlan {
    int family, block, rows, cols, lds, store;
    int64_t grid;
    BmmGeom g;
};

inline bool strides16(const lsq_attn_w8_strides& s) { return s.s0 % 16 == 0 && s.s1 % 16 == 0 && s.ld % 16 == 0; }

inline BmmPlan plan_bmm(const lsq_bmm_w8_geom& ge, bool ab_aligned, bool y_aligned, bool levels_out) {
    BmmPlan pl = {};
    pl.block = kBlock;
    pl.g = BmmGeom{ge.a.s0, ge.a.s1, ge.a.ld, ge.b.s0, ge.b.s1, ge.b.ld, ge.y.s0, ge.y.s1, ge.y.ld, static_cast<int>(ge.B1),
                   static_cast<int>(ge.M), static_cast<int>(ge.N), static_cast<int>(ge.K), 0, 0};
    const int64_t batches = ge.B0 * ge.B1;
    if (ab_aligned && strides16(ge.a) && strides16(ge.b)) {
        pl.family = LSQ_ATTN_W8_MFMA;
        pl.rows = pl.cols = kAttnTile;
        pl.lds = kAttnLds;
        pl.g.row_tiles = static_cast<int>(ceil_div(ge.M, kAttnTile));
        pl.g.col_tiles = static_cast<int>(ceil_div(ge.N, kAttnTile));
        pl.grid = batches * pl.g.row_tiles * pl.g.col_tiles;
        pl.store = levels_out && y_aligned && strides16(ge.y) ? LSQ_ATTN_W8_STORE_PACKETS : LSQ_ATTN_W8_STORE_ELEMS;
    } else {
        pl.family = LSQ_ATTN_W8_GENERIC;
        pl.grid = ceil_div(batches * ge.M * ge.N, kBlock);
        pl.store = LSQ_ATTN_W8_STORE_ELEMS;
    }
    return pl;
}

struct SmxPlan {
    int family, block, L, P, rows, lds;
    int64_t grid;
    SmxGeom g;
};

inline SmxPlan plan_softmax(const lsq_softmax_w8_geom& ge, bool aligned) {
    SmxPlan pl = {};
    pl.block = kBlock;
    const int packets = static_cast<int>(ceil_div(ge.C, 16));
    pl.g = SmxGeom{ge.R, ge.ldx, ge.ldy, static_cast<int>(ge.C), packets, 1, ge.x_dtype == LSQ_ATTN_W8_I8 ? 0x80808080u : 0u};
    if (!(aligned && ge.ldx % 16 == 0 && ge.ldy % 16 == 0 && ge.C <= 16 * kSmxWave * kSmxMaxP)) {
        pl.family = LSQ_ATTN_W8_GENERIC;
        pl.L = kSmxWave;
        pl.rows = kBlock / kSmxWave;
        pl.grid = ceil_div(ge.R, pl.rows);
        return pl;
    }
    int P = 1;
    while (ceil_div(packets, P) > kSmxWave) P *= 2;
    int L = 4;
    while (L < ceil_div(packets, P)) L *= 2;
    const int G = kBlock / L;
    const int K = ceil_div(ge.R, static_cast<int64_t>(G) * kSmxRows) >= kSmxFill ? kSmxRows : 1;
    pl.family = LSQ_ATTN_W8_PACKETS;
    pl.L = L;
    pl.P = P;
    pl.rows = G * K;
    pl.g.K = K;
    pl.grid = ceil_div(ge.R, pl.rows);
    pl.lds = 1024;
    return pl;
}

typedef void (*SmxKernel)(SmxGeom, AttnOut, const int32_t*, const uint8_t*, void*);

inline SmxKernel packets_kernel(int L, int P) {
    switch (L) {
        case 4: return softmax_w8_packets_kernel<4, 1>;
        case 8: return softmax_w8_packets_kernel<8, 1>;
        case 16: return softmax_w8_packets_kernel<16, 1>;
        case 32: return softmax_w8_packets_kernel<32, 1>;
        default: break;
    }
    switch (P) {            // more than one packet per lane: the group is a whole wave
        case 1: return softmax_w8_packets_kernel<64, 1>;
        case 2: return softmax_w8_packets_kernel<64, 2>;
        case 4: return softmax_w8_packets_kernel<64, 4>;
        default: return softmax_w8_packets_kernel<64, 8>;
    }
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_attn_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

int check_bmm_geom(const char* what, const lsq_bmm_w8_geom* g) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (g->form != LSQ_ATTN_W8_NN && g->form != LSQ_ATTN_W8_NT)
        return fail(LSQ_EINVAL, "%s: form must be LSQ_ATTN_W8_NN (0) or LSQ_ATTN_W8_NT (1), got %lld", what, static_cast<ll>(g->form));
    if (!level_dtype(g->a_dtype) || !level_dtype(g->b_dtype))
        return fail(LSQ_EINVAL, "%s: a_dtype and b_dtype must be LSQ_ATTN_W8_U8 (0) or LSQ_ATTN_W8_I8 (1), got %lld and %lld", what,
                    static_cast<ll>(g->a_dtype), static_cast<ll>(g->b_dtype));
    if (g->B0 < 1 || g->B1 < 1 || g->M < 1 || g->N < 1 || g->K < 1)
        return fail(LSQ_EINVAL, "%s: [B0, B1, M, N, K] = [%lld, %lld, %lld, %lld, %lld], every extent must be at least 1", what,
                    static_cast<ll>(g->B0), static_cast<ll>(g->B1), static_cast<ll>(g->M), static_cast<ll>(g->N), static_cast<ll>(g->K));
    if (g->K > LSQ_ATTN_W8_MAX_K)
        return fail(LSQ_EINVAL, "%s: K = %lld, at most %d are served (the raw sum stays in 32 bits)", what, static_cast<ll>(g->K), LSQ_ATTN_W8_MAX_K);
    const int64_t lim = int64_t{1} << 20;
    if (g->M > lim || g->N > lim || g->B0 > lim || g->B1 > lim || g->B0 * g->B1 > lim)
        return fail(LSQ_EINVAL, "%s: M = %lld, N = %lld and B0 * B1 = %lld x %lld may each be 2^20 at most", what, static_cast<ll>(g->M),
                    static_cast<ll>(g->N), static_cast<ll>(g->B0), static_cast<ll>(g->B1));
    const bool nn = g->form == LSQ_ATTN_W8_NN;
    if (int rc = check_strides(what, "A", g->a, g->K)) return rc;
    if (int rc = check_strides(what, "B", g->b, nn ? g->N : g->K)) return rc;
    if (int rc = check_strides(what, "y", g->y, g->N)) return rc;
    if (self_overlap(g->y, g->B0, g->B1, g->M, g->N))
        return fail(LSQ_EINVAL, "%s: y's rows or batches overlap each other (strides %lld, %lld, %lld for [%lld, %lld, %lld, %lld])", what,
                    static_cast<ll>(g->y.s0), static_cast<ll>(g->y.s1), static_cast<ll>(g->y.ld), static_cast<ll>(g->B0),
                    static_cast<ll>(g->B1), static_cast<ll>(g->M), static_cast<ll>(g->N));
    return LSQ_OK;
}

int check_softmax_geom(const char* what, const lsq_softmax_w8_geom* g) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (!level_dtype(g->x_dtype))
        return fail(LSQ_EINVAL, "%s: x_dtype must be LSQ_ATTN_W8_U8 (0) or LSQ_ATTN_W8_I8 (1), got %lld", what, static_cast<ll>(g->x_dtype));
    if (g->R < 1 || g->C < 1)
        return fail(LSQ_EINVAL, "%s: x is [R, C] = [%lld, %lld], every extent must be at least 1", what, static_cast<ll>(g->R), static_cast<ll>(g->C));
    if (g->C > LSQ_ATTN_W8_MAX_C)
        return fail(LSQ_EINVAL, "%s: C = %lld, at most %d elements per row are served", what, static_cast<ll>(g->C), LSQ_ATTN_W8_MAX_C);
    if (g->R > INT32_MAX / 4) return fail(LSQ_EINVAL, "%s: R = %lld is beyond 29 bits", what, static_cast<ll>(g->R));
    if (g->ldx < g->C || g->ldy < g->C)
        return fail(LSQ_EINVAL, "%s: the row strides ldx = %lld and ldy = %lld must be at least C = %lld", what, static_cast<ll>(g->ldx),
                    static_cast<ll>(g->ldy), static_cast<ll>(g->C));
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_attn_w8_abi_version(void) { return LSQ_ATTN_W8_ABI_VERSION; }

const char* lsq_attn_w8_last_error(void) { return g_last_error; }

int lsq_bmm_w8(const lsq_bmm_w8_geom* geom, const lsq_bmm_w8_consts* consts, const lsq_attn_w8_out* out, const void* a_levels,
               const void* b_levels, void* y, void* stream) {
    const char* what = "lsq_bmm_w8";
    lsq::AttnOut oarg{};
    int64_t y_elem = 1;
    if (int rc = check_bmm_geom(what, geom)) return rc;
    if (!consts) return fail(LSQ_EINVAL, "%s: NULL constants", what);
    if (!consts->s_a || !consts->z_a || !consts->s_b || !consts->z_b) return fail(LSQ_EINVAL, "%s: NULL scale or zero point", what);
    if (!aligned_to(consts->s_a, 4) || !aligned_to(consts->z_a, 4) || !aligned_to(consts->s_b, 4) || !aligned_to(consts->z_b, 4))
        return fail(LSQ_EINVAL, "%s: the scales and zero points must be element-aligned", what);
    if (int rc = check_out(what, out, oarg, y_elem)) return rc;
    if (!a_levels || !b_levels || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(y, static_cast<uintptr_t>(y_elem))) return fail(LSQ_EINVAL, "%s: a floating y must be element-aligned", what);
    const bool nn = geom->form == LSQ_ATTN_W8_NN;
    const int64_t a_span = span_of(geom->a, geom->B0, geom->B1, geom->M, geom->K);
    const int64_t b_span = nn ? span_of(geom->b, geom->B0, geom->B1, geom->K, geom->N) : span_of(geom->b, geom->B0, geom->B1, geom->N, geom->K);
    const int64_t y_bytes = span_of(geom->y, geom->B0, geom->B1, geom->M, geom->N) * y_elem;
    if (overlap(y, y_bytes, a_levels, a_span) || overlap(y, y_bytes, b_levels, b_span))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap A's %lld or B's %lld", what, static_cast<ll>(y_bytes), static_cast<ll>(a_span),
                    static_cast<ll>(b_span));
    const bool levels_out = out->out_scale != nullptr;
    lsq::BmmPlan pl = lsq::plan_bmm(*geom, aligned_to(a_levels, 16) && aligned_to(b_levels, 16), aligned_to(y, 16), levels_out);
    if (int rc = check_grid(what, pl.grid)) return rc;
    const lsq::BmmArg arg{static_cast<const float*>(consts->s_a), static_cast<const int32_t*>(consts->z_a),
                          static_cast<const float*>(consts->s_b), static_cast<const int32_t*>(consts->z_b),
                          geom->a_dtype == LSQ_ATTN_W8_U8 ? 128 : 0, geom->b_dtype == LSQ_ATTN_W8_U8 ? 128 : 0,
                          pl.store == LSQ_ATTN_W8_STORE_PACKETS ? 1 : 0};
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kBlock);
    const uint8_t* A = static_cast<const uint8_t*>(a_levels);
    const uint8_t* B = static_cast<const uint8_t*>(b_levels);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pl.family == LSQ_ATTN_W8_MFMA) {
        if (nn) hipLaunchKernelGGL(lsq::bmm_w8_mfma_kernel<true>, grid, block, 0, st, pl.g, arg, oarg, A, B, y);
        else hipLaunchKernelGGL(lsq::bmm_w8_mfma_kernel<false>, grid, block, 0, st, pl.g, arg, oarg, A, B, y);
    } else {
        hipLaunchKernelGGL(lsq::bmm_w8_generic_kernel, grid, block, 0, st, pl.g, arg, oarg, nn ? 1 : 0,
                           geom->B0 * geom->B1 * geom->M * geom->N, A, B, y);
    }
    return hip_status(hipGetLastError(), what);
}

int lsq_bmm_w8_plan(const lsq_bmm_w8_geom* geom, int ab_aligned, int y_aligned, int levels_out, int32_t* out8) {
    const char* what = "lsq_bmm_w8_plan";
    if (int rc = check_bmm_geom(what, geom)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::BmmPlan pl = lsq::plan_bmm(*geom, ab_aligned != 0, y_aligned != 0, levels_out != 0);
    if (int rc = check_grid(what, pl.grid)) return rc;
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(geom->form);
    out8[2] = static_cast<int32_t>(pl.grid);
    out8[3] = pl.block;
    out8[4] = pl.rows;
    out8[5] = pl.cols;
    out8[6] = pl.lds;
    out8[7] = pl.store;
    return LSQ_OK;
}

int lsq_softmax_w8(const lsq_softmax_w8_geom* geom, const lsq_attn_w8_out* out, const void* table, const void* x_levels, void* y,
                   void* stream) {
    const char* what = "lsq_softmax_w8";
    lsq::AttnOut oarg{};
    int64_t y_elem = 1;
    if (int rc = check_softmax_geom(what, geom)) return rc;
    if (int rc = check_out(what, out, oarg, y_elem)) return rc;
    if (!table || !x_levels || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(table, 4)) return fail(LSQ_EINVAL, "%s: the table must be element-aligned", what);
    if (!aligned_to(y, static_cast<uintptr_t>(y_elem))) return fail(LSQ_EINVAL, "%s: a floating y must be element-aligned", what);
    const int64_t x_bytes = (geom->R - 1) * geom->ldx + geom->C, y_bytes = ((geom->R - 1) * geom->ldy + geom->C) * y_elem;
    if (overlap(y, y_bytes, x_levels, x_bytes) || overlap(y, y_bytes, table, 1024))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap x's %lld or the table: the softmax in place is not served", what,
                    static_cast<ll>(y_bytes), static_cast<ll>(x_bytes));
    const lsq::SmxPlan pl = lsq::plan_softmax(*geom, aligned_to(x_levels, 16) && aligned_to(y, 16));
    if (int rc = check_grid(what, pl.grid)) return rc;
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kBlock);
    const uint8_t* x = static_cast<const uint8_t*>(x_levels);
    const int32_t* tb = static_cast<const int32_t*>(table);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pl.family == LSQ_ATTN_W8_PACKETS) hipLaunchKernelGGL(lsq::packets_kernel(pl.L, pl.P), grid, block, 0, st, pl.g, oarg, tb, x, y);
    else hipLaunchKernelGGL(lsq::softmax_w8_generic_kernel, grid, block, 0, st, pl.g, oarg, tb, x, y);
    return hip_status(hipGetLastError(), what);
}

int lsq_softmax_w8_plan(const lsq_softmax_w8_geom* geom, int aligned, int32_t* out8) {
    const char* what = "lsq_softmax_w8_plan";
    if (int rc = check_softmax_geom(what, geom)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::SmxPlan pl = lsq::plan_softmax(*geom, aligned != 0);
    if (int rc = check_grid(what, pl.grid)) return rc;
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.block;
    out8[3] = pl.L;
    out8[4] = pl.P;
    out8[5] = pl.rows;
    out8[6] = pl.lds;
    out8[7] = 0;
    return LSQ_OK;
}

}  // extern "C"
