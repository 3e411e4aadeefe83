// lsq_dwconv_w8.hip -- the W8A8 depthwise conv2d on channels-last 8-bit levels on gfx950 (include/lsq_hip_dwconv_w8.h, which
// states the contract): the kernels and the C ABI of liblsq_hip_dwconv_w8.so.  There is no reduction over channels, so no
// matrix-core tile applies: these are per-channel tap kernels on 16-byte packets along C.
//
// Both byte operands are taken UNSIGNED: an int8 level is biased by 0x80 on load (a = l + off, off = 128 or 0), and so are the
// zero points (za = zx + off_x, zb[c] = zw[c] + off_w).  With T taps in a sum
//     I = sum a b - za sum b - zb sum a + T za zb.
//
//  * PACKETS, 3 x 3 without dilation at stride 1 and 2 (dwconv_w8_packets_dot_kernel<S>, the library's): a lane owns one
//    16-channel packet of one output pixel; adjacent lanes sit on adjacent packets.  The nine weight packets and the nine
//    packets of x are loaded up front, x from addresses clamped into the input, and a tap outside is replaced by the byte za
//    afterwards, so that T = 9 everywhere.  The products go through v_dot4_u32_u8: a word of a packet holds four channels of one
//    tap, so four words of four taps are transposed as a 4 x 4 block of bytes with eight v_perm_b32 (taps 0..3 and 4..7; tap 8
//    is a byte product), x and w alike; sum a and sum b come from the same transposed words against 0x01010101.
//    The experiment's variants, NOT shipped (-DLSQ_DWCONV_W8_DOT4=0, tools/exp_dwconv_w8_ab.py --build-variants):
//    dwconv_w8_packets_kernel<3, S, P>, a byte product per channel and tap as the compiler schedules it, with P = 1, 2 or 4
//    adjacent output pixels along ow per lane (-DLSQ_DWCONV_W8_PIX_S1=N / _S2=N) that share the held weights and, row by row,
//    the loaded columns.  Measured and not kept.
//  * PACKETS, every other window (dwconv_w8_packets_loop_kernel): one pixel per lane, the taps inside x in a loop with run-time
//    bounds; sum a, sum b and T over those taps.
//  * GENERIC (C % 16 != 0 or a misaligned buffer): one lane per output element, byte loads, (l - zx) (w - zw) as it stands.
// One epilogue (dw_value, w8o_byte; four channels at a time in dw_group) serves all of them; it has no branch on the bias's dtype
// or on mid_dtype: both candidates are formed and one is selected, so that nothing stands between a packet's loads and its
// arithmetic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../lsq_w8_out_side.hpp"
#include "../lsq_w8_out_side_host.hpp"
#include "../qlinear_w8/lsq_w8_shared.hpp"
#include "../../../include/lsq_hip_dwconv_w8.h"

#ifndef LSQ_DWCONV_W8_DOT4
#define LSQ_DWCONV_W8_DOT4 1         // 1: transposed bytes through v_dot4_u32_u8 (the library's); 0: a byte product per channel and tap
#endif
#ifndef LSQ_DWCONV_W8_PIX_S1
#define LSQ_DWCONV_W8_PIX_S1 1
#endif
#ifndef LSQ_DWCONV_W8_PIX_S2
#define LSQ_DWCONV_W8_PIX_S2 1
#endif

namespace lsq {

constexpr int kDwPixS1 = LSQ_DWCONV_W8_PIX_S1;
constexpr int kDwPixS2 = LSQ_DWCONV_W8_PIX_S2;
constexpr int kDwBlocksPerCU = 2;               // P is halved while the grid holds fewer workgroups per compute unit
static_assert(kDwPixS1 == 1 || kDwPixS1 == 2 || kDwPixS1 == 4, "pixels per lane: 1, 2 or 4");
static_assert(kDwPixS2 == 1 || kDwPixS2 == 2 || kDwPixS2 == 4, "pixels per lane: 1, 2 or 4");
static_assert(!LSQ_DWCONV_W8_DOT4 || (kDwPixS1 == 1 && kDwPixS2 == 1), "the dot-product kernel owns one pixel per lane");

struct DwGeom {             // kernel argument; the host has checked that the coordinates fit 32 bits
    int64_t image;          // H W C, the bytes of one image of x
    int C, CP;              // channels, 16-channel packets
    int H, W, OH, OW, kh, kw, sh, sw, ph, pw, dh, dw;
};

struct DwArg {              // kernel argument: the constants of one call
    const float* s_x;
    const int32_t* zx;
    const float* w_scale;
    const int32_t* w_zero;
    const void* bias;       // NULL: none
    const float* scale;     // the output quantizer; NULL: a floating y
    const float* shift;
    float qmin, qmax, tmin, tmax;
    int bias_dtype;
    int act;                // LSQ_DWCONV_W8_ACT_*
    int mid;                // LSQ_F32 / LSQ_BF16 / LSQ_F16
    int offx, offw;         // 128 for int8 levels (biased on load), 0 for uint8
};

struct DwQ : W8OutSide {    // the same, read once per thread
    float s_x;
    int zx;                 // as it is
    float lo, hi;           // the bounds of the selects
    // the bias, read without a branch: both pointers are always loadable for C elements (w_scale stands in where the bias is
    // absent or of the other width), and the selects below pick the value, or -0.0f, which no sum is changed by
    const float* bias32;
    const unsigned short* bias16;
    bool has_bias, bias_is16, bias_is_bf16;
};

__device__ __forceinline__ DwQ dw_constants(const DwArg& a) {
    DwQ q;
    w8o_constants(q, a);
    q.s_x = a.s_x[0];
    q.zx = a.zx[0];
    q.lo = a.act >= LSQ_DWCONV_W8_ACT_RELU ? 0.0f : -__builtin_huge_valf();
    q.hi = a.act == LSQ_DWCONV_W8_ACT_RELU6 ? 6.0f : __builtin_huge_valf();
    q.has_bias = a.bias != nullptr;
    q.bias_is16 = q.has_bias && a.bias_dtype != LSQ_F32;
    q.bias_is_bf16 = a.bias_dtype == LSQ_BF16;
    q.bias32 = (q.has_bias && !q.bias_is16) ? static_cast<const float*>(a.bias) : a.w_scale;
    q.bias16 = q.bias_is16 ? static_cast<const unsigned short*>(a.bias) : reinterpret_cast<const unsigned short*>(a.w_scale);
    return q;
}

// the selects of the contract with the bounds as data: act 0 has (-inf, +inf), which no value lies beyond, ReLU (0, +inf),
// ReLU6 (0, 6); a NaN compares false twice and stays a NaN
__device__ __forceinline__ float dw_act(float u, float lo, float hi) {
    u = (u < lo) ? lo : u;
    return (u > hi) ? hi : u;
}

// bias[c] as float32, -0.0f without a bias (v + -0.0f is v, bit for bit, a zero of either sign and a NaN included)
__device__ __forceinline__ float dw_bias(const DwQ& q, int64_t c) {
    const float b32 = q.bias32[c];
    const unsigned short raw = q.bias16[c];
    _Float16 half;
    __builtin_memcpy(&half, &raw, 2);
    const float b16 = q.bias_is_bf16 ? __uint_as_float(static_cast<uint32_t>(raw) << 16) : static_cast<float>(half);
    return q.has_bias ? (q.bias_is16 ? b16 : b32) : -0.0f;
}

// the fp32 steps of the contract on the exact integer, the rounding to mid_dtype and the selects: r of the contract
__device__ __forceinline__ float dw_value(int I, float s_w, float bias, const DwQ& q) {
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(s_w, static_cast<float>(I)), q.s_x), bias);
    return dw_act(w8o_round_mid(v, q.mid), q.lo, q.hi);
}

// four floating outputs: `at` in elements of y (a multiple of 4), y 16-byte aligned
__device__ __forceinline__ void dw_store4(void* y, int64_t at, const float (&r)[4], const DwQ& q) {
    if (q.mid == LSQ_F32) {
        *reinterpret_cast<u32x4*>(static_cast<float*>(y) + at) =
            u32x4{__float_as_uint(r[0]), __float_as_uint(r[1]), __float_as_uint(r[2]), __float_as_uint(r[3])};
        return;
    }
    uint32_t w[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        unsigned short lo, hi;
        if (q.mid == LSQ_BF16) {
            lo = static_cast<unsigned short>(__float_as_uint(r[2 * i]) >> 16);          // r is a bfloat16 value: its high half
            hi = static_cast<unsigned short>(__float_as_uint(r[2 * i + 1]) >> 16);
        } else {
            const _Float16 a = static_cast<_Float16>(r[2 * i]), b = static_cast<_Float16>(r[2 * i + 1]);
            __builtin_memcpy(&lo, &a, 2);
            __builtin_memcpy(&hi, &b, 2);
        }
        w[i] = static_cast<uint32_t>(lo) | static_cast<uint32_t>(hi) << 16;
    }
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
    *reinterpret_cast<u32x2_t*>(static_cast<uint8_t*>(y) + at * 2) = u32x2_t{w[0], w[1]};
}

// The epilogue of four adjacent channels c0 .. c0 + 3 (c0 % 4 == 0, w_scale and w_zero 16-byte aligned) from their raw sums over
// T taps: I = sum a b + za (T zb - sum b) - zb sum a, every factor within 24 bits.  The channels' constants are loaded here, where
// they are used, so that no more than a group's worth is held; the levels leave as one word, floats as one store at `at` (elements).
__device__ __forceinline__ uint32_t dw_group(const uint32_t (&ab)[4], const uint32_t (&sa)[4], const uint32_t (&sb)[4], int T, int za, int c0,
                                             const DwArg& a, const DwQ& q, void* y, int64_t at) {
    const u32x4 sw4 = *reinterpret_cast<const u32x4*>(a.w_scale + c0);
    const u32x4 zw4 = *reinterpret_cast<const u32x4*>(a.w_zero + c0);
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int zb = static_cast<int>(zw4[k]) + a.offw;
        const int I = static_cast<int>(ab[k]) + __mul24(za, __mul24(T, zb) - static_cast<int>(sb[k])) - __mul24(zb, static_cast<int>(sa[k]));
        r[k] = dw_value(I, __uint_as_float(sw4[k]), dw_bias(q, c0 + k), q);
    }
    if (q.levels_out)
        return w8o_byte(r[0], q) | w8o_byte(r[1], q) << 8 | w8o_byte(r[2], q) << 16 | w8o_byte(r[3], q) << 24;
    dw_store4(y, at, r, q);
    return 0u;
}

// acc[16] += the 16 byte products of a packet of x and a packet of w
__device__ __forceinline__ void dw_mac_packet(int (&acc)[16], u32x4 xv, u32x4 wv) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc[4 * i] += static_cast<int>((xv[i] & 0xffu) * (wv[i] & 0xffu));
        acc[4 * i + 1] += static_cast<int>(((xv[i] >> 8) & 0xffu) * ((wv[i] >> 8) & 0xffu));
        acc[4 * i + 2] += static_cast<int>(((xv[i] >> 16) & 0xffu) * ((wv[i] >> 16) & 0xffu));
        acc[4 * i + 3] += static_cast<int>((xv[i] >> 24) * (wv[i] >> 24));
    }
}

// sum[16] += the 16 bytes of a packet
__device__ __forceinline__ void dw_add_packet(uint32_t (&sum)[16], u32x4 v) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sum[4 * i] += v[i] & 0xffu;
        sum[4 * i + 1] += (v[i] >> 8) & 0xffu;
        sum[4 * i + 2] += (v[i] >> 16) & 0xffu;
        sum[4 * i + 3] += v[i] >> 24;
    }
}

// item = ((b OH + oh) OWN + ow) CN + c: 32-bit divisions while the count of items allows them (the usual case; one uniform test)
struct DwItem {
    int c, ow, oh;
    int64_t b;
};

__device__ __forceinline__ DwItem dw_decode(int64_t item, int64_t items, int CN, int OWN, int OH) {
    DwItem d;
    if (items <= 0x7fffffff) {
        const uint32_t it = static_cast<uint32_t>(item), t = it / static_cast<uint32_t>(CN);
        const uint32_t u = t / static_cast<uint32_t>(OWN), b = u / static_cast<uint32_t>(OH);
        d.c = static_cast<int>(it - t * static_cast<uint32_t>(CN));
        d.ow = static_cast<int>(t - u * static_cast<uint32_t>(OWN));
        d.oh = static_cast<int>(u - b * static_cast<uint32_t>(OH));
        d.b = b;
    } else {
        int64_t t = item / CN;
        d.c = static_cast<int>(item - t * CN);
        d.ow = static_cast<int>(t % OWN);
        t /= OWN;
        d.oh = static_cast<int>(t % OH);
        d.b = t / OH;
    }
    return d;
}

// where a tap lies: clamped into the input (a load from there is always legal), and whether it was inside
__device__ __forceinline__ int dw_clamp(int v, int n, bool& inside) {
    inside = inside && static_cast<unsigned>(v) < static_cast<unsigned>(n);
    return min(max(v, 0), n - 1);
}

// ------------------------------------------------------------------------------------------------
// packets, 3 x 3 without dilation at stride (S, S), one output pixel per lane, the products through v_dot4_u32_u8 (the
// library's form, LSQ_DWCONV_W8_DOT4 == 1).  item = ((b OH + oh) OW + ow) CP + packet.
// A word of a packet holds 4 channels of one tap; the dot product wants 4 taps of one channel.  Four words of four taps are
// transposed as a 4 x 4 block of bytes with 8 v_perm_b32, x and w alike: taps 0..3 and taps 4..7 are two blocks, tap 8 is a
// plain byte product.  sum a comes from the same transposed words against 0x01010101, sum b likewise, once per lane.
// ------------------------------------------------------------------------------------------------
struct DwT4 {
    uint32_t c[4];          // c[k]: byte k of each of the four words, in their order
};

__device__ __forceinline__ DwT4 dw_transpose(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
    // __builtin_amdgcn_perm(hi, lo, sel): selector bytes 0..3 take lo's bytes, 4..7 hi's
    const uint32_t lo01 = __builtin_amdgcn_perm(x1, x0, 0x05010400u), hi01 = __builtin_amdgcn_perm(x1, x0, 0x07030602u);
    const uint32_t lo23 = __builtin_amdgcn_perm(x3, x2, 0x05010400u), hi23 = __builtin_amdgcn_perm(x3, x2, 0x07030602u);
    DwT4 t;
    t.c[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
    t.c[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    t.c[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
    t.c[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
    return t;
}

__device__ __forceinline__ uint32_t dw_byte_of(uint32_t w, int k) { return (w >> (8 * k)) & 0xffu; }

template <int S>
__global__ __launch_bounds__(kBlock, 4) void dwconv_w8_packets_dot_kernel(DwGeom g, DwArg a, const uint8_t* __restrict__ x,
                                                                          const uint8_t* __restrict__ w, void* __restrict__ y, int64_t items) {
    constexpr uint32_t kOnes = 0x01010101u;
    const int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (item >= items) return;
    const DwQ q = dw_constants(a);
    const DwItem at = dw_decode(item, items, g.CP, g.OW, g.OH);
    const int cp = at.c, ow = at.ow, oh = at.oh;
    const int64_t b = at.b;
    const int ih0 = oh * S - g.ph, iw0 = ow * S - g.pw;
    const uint8_t* __restrict__ src = x + b * g.image + cp * 16;
    const uint32_t flipx = a.offx ? 0x80808080u : 0u, flipw = a.offw ? 0x80808080u : 0u;
    const int za = q.zx + a.offx;
    const uint32_t pad = static_cast<uint32_t>(za & 0xff) * 0x01010101u;

    // the weight packets first: they are in flight while the addresses of x are formed
    u32x4 wv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wv[k] = *reinterpret_cast<const u32x4*>(w + static_cast<int64_t>(k) * g.C + cp * 16);
    // every load of x from an address clamped into the input; a tap outside becomes the byte za
    u32x4 xv[9];
    {
        bool in_h[3], in_w[3];
        int64_t row[3], col[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            in_h[i] = in_w[i] = true;
            row[i] = static_cast<int64_t>(dw_clamp(ih0 + i, g.H, in_h[i])) * g.W * g.C;
            col[i] = static_cast<int64_t>(dw_clamp(iw0 + i, g.W, in_w[i])) * g.C;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) xv[i * 3 + j] = *reinterpret_cast<const u32x4*>(src + row[i] + col[j]);
        // the nine packets are wanted as loaded: without this the compiler sinks each load into the branch of its select below
        // and waits for it there, nine latencies in a row
        asm volatile("" : "+v"(xv[0]), "+v"(xv[1]), "+v"(xv[2]), "+v"(xv[3]), "+v"(xv[4]), "+v"(xv[5]), "+v"(xv[6]), "+v"(xv[7]), "+v"(xv[8]));
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) xv[i * 3 + j] = (in_h[i] && in_w[j]) ? (xv[i * 3 + j] ^ flipx) : u32x4{pad, pad, pad, pad};
    }
    // the weights of the lane's packet, transposed once
    DwT4 wa[4], wb[4];
    u32x4 w8;
    {
#pragma unroll
        for (int k = 0; k < 9; ++k) wv[k] ^= flipw;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            wa[i] = dw_transpose(wv[0][i], wv[1][i], wv[2][i], wv[3][i]);
            wb[i] = dw_transpose(wv[4][i], wv[5][i], wv[6][i], wv[7][i]);
        }
        w8 = wv[8];
    }
    uint32_t out[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const DwT4 xa = dw_transpose(xv[0][i], xv[1][i], xv[2][i], xv[3][i]);
        const DwT4 xb = dw_transpose(xv[4][i], xv[5][i], xv[6][i], xv[7][i]);
        uint32_t ab[4], sa[4], sb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t x8 = dw_byte_of(xv[8][i], k), b8 = dw_byte_of(w8[i], k);
            ab[k] = __builtin_amdgcn_udot4(xb.c[k], wb[i].c[k], __builtin_amdgcn_udot4(xa.c[k], wa[i].c[k], x8 * b8, false), false);
            sa[k] = __builtin_amdgcn_udot4(xb.c[k], kOnes, __builtin_amdgcn_udot4(xa.c[k], kOnes, x8, false), false);
            sb[k] = __builtin_amdgcn_udot4(wb[i].c[k], kOnes, __builtin_amdgcn_udot4(wa[i].c[k], kOnes, b8, false), false);
        }
        out[i] = dw_group(ab, sa, sb, 9, za, cp * 16 + 4 * i, a, q, y, item * 16 + 4 * i);
    }
    if (q.levels_out) *reinterpret_cast<u32x4*>(static_cast<uint8_t*>(y) + item * 16) = u32x4{out[0], out[1], out[2], out[3]};
}

#if !LSQ_DWCONV_W8_DOT4
// ---- what the experiment's variant alone needs ----
// the per-channel constants of a lane's packet, loaded once and reused over its pixels
struct DwChan {
    float s_w[16], bias[16];
    int zb[16];             // zw[c] + off_w
};

__device__ __forceinline__ void dw_load_channels(DwChan& ch, const DwArg& a, const DwQ& q, int c0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u32x4 s = *reinterpret_cast<const u32x4*>(a.w_scale + c0 + 4 * i);       // c0 % 16 == 0: 16-byte aligned
        const u32x4 z = *reinterpret_cast<const u32x4*>(a.w_zero + c0 + 4 * i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ch.s_w[4 * i + k] = __uint_as_float(s[k]);
            ch.zb[4 * i + k] = static_cast<int>(z[k]) + a.offw;
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) ch.bias[i] = dw_bias(q, c0 + i);
}

// the same in packed 16-bit pairs: e[i] the even bytes of word i, o[i] the odd ones (at most 257 packets: no carry between pairs)
struct DwPairs {
    uint32_t e[4], o[4];
};

__device__ __forceinline__ void dw_add_pairs(DwPairs& s, u32x4 v) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s.e[i] += v[i] & 0x00ff00ffu;
        s.o[i] += (v[i] >> 8) & 0x00ff00ffu;
    }
}

__device__ __forceinline__ int dw_pair_at(const DwPairs& s, int c) {          // the sum of channel c of the packet
    const uint32_t w = (c & 1) ? s.o[c >> 2] : s.e[c >> 2];
    return static_cast<int>((c & 2) ? (w >> 16) : (w & 0xffffu));
}

// ------------------------------------------------------------------------------------------------
// packets, a K x K window without dilation at stride (S, S), P adjacent output pixels per lane
// item = ((b OH + oh) OWG + owg) CP + packet, OWG = ceil(OW / P)
// ------------------------------------------------------------------------------------------------
template <int K, int S, int P>
__global__ __launch_bounds__(kBlock) void dwconv_w8_packets_kernel(DwGeom g, DwArg a, const uint8_t* __restrict__ x,
                                                                   const uint8_t* __restrict__ w, void* __restrict__ y, int64_t items) {
    constexpr int T = K * K, SPAN = (P - 1) * S + K;           // taps; input columns the lane's windows cover
    const int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (item >= items) return;
    const DwQ q = dw_constants(a);
    const DwItem at = dw_decode(item, items, g.CP, (g.OW + P - 1) / P, g.OH);
    const int cp = at.c, oh = at.oh;
    const int64_t b = at.b;
    const int ow0 = at.ow * P;
    const int ih0 = oh * S - g.ph, iw0 = ow0 * S - g.pw;
    const uint8_t* __restrict__ src = x + b * g.image + cp * 16;
    const uint32_t flipx = a.offx ? 0x80808080u : 0u, flipw = a.offw ? 0x80808080u : 0u;
    const int za = q.zx + a.offx;
    const uint32_t pad = static_cast<uint32_t>(za & 0xff) * 0x01010101u;

    u32x4 wv[T];
#pragma unroll
    for (int k = 0; k < T; ++k) wv[k] = *reinterpret_cast<const u32x4*>(w + static_cast<int64_t>(k) * g.C + cp * 16) ^ flipw;

    int acc[P][16];
    DwPairs sa[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[p][i] = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) sa[p].e[i] = sa[p].o[i] = 0u;
    }

    if constexpr (P == 1) {
        u32x4 xv[T];
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                bool inside = true;
                const int ih = dw_clamp(ih0 + i, g.H, inside), iw = dw_clamp(iw0 + j, g.W, inside);
                const u32x4 v = *reinterpret_cast<const u32x4*>(src + (static_cast<int64_t>(ih) * g.W + iw) * g.C) ^ flipx;
                xv[i * K + j] = inside ? v : u32x4{pad, pad, pad, pad};
            }
#pragma unroll
        for (int k = 0; k < T; ++k) {
            dw_mac_packet(acc[0], xv[k], wv[k]);
            dw_add_pairs(sa[0], xv[k]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            bool row_inside = true;
            const int ih = dw_clamp(ih0 + i, g.H, row_inside);
            const uint8_t* __restrict__ row = src + static_cast<int64_t>(ih) * g.W * g.C;
            u32x4 xv[SPAN];
#pragma unroll
            for (int c = 0; c < SPAN; ++c) {
                bool inside = row_inside;
                const int iw = dw_clamp(iw0 + c, g.W, inside);
                const u32x4 v = *reinterpret_cast<const u32x4*>(row + static_cast<int64_t>(iw) * g.C) ^ flipx;
                xv[c] = inside ? v : u32x4{pad, pad, pad, pad};
            }
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    dw_mac_packet(acc[p], xv[p * S + j], wv[i * K + j]);
                    dw_add_pairs(sa[p], xv[p * S + j]);
                }
        }
    }

    // I = sum a b + za (T zb - sum b) - zb sum a
    DwPairs sb;
#pragma unroll
    for (int i = 0; i < 4; ++i) sb.e[i] = sb.o[i] = 0u;
#pragma unroll
    for (int k = 0; k < T; ++k) dw_add_pairs(sb, wv[k]);
    DwChan ch;
    dw_load_channels(ch, a, q, cp * 16);
    const int64_t at0 = (((b * g.OH + oh) * g.OW + ow0) * g.CP + cp) * 16;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (ow0 + p < g.OW) {
            float r[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int I = acc[p][c] + za * (T * ch.zb[c] - dw_pair_at(sb, c)) - ch.zb[c] * dw_pair_at(sa[p], c);
                r[c] = dw_value(I, ch.s_w[c], ch.bias[c], q);
            }
            w8o_store16(y, at0 + static_cast<int64_t>(p) * g.C, r, q);
        }
    }
}

#endif  // !LSQ_DWCONV_W8_DOT4

// ------------------------------------------------------------------------------------------------
// packets, any window: one pixel per lane, the taps inside x in a loop.  item = ((b OH + oh) OW + ow) CP + packet
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock, 4) void dwconv_w8_packets_loop_kernel(DwGeom g, DwArg a, const uint8_t* __restrict__ x,
                                                                        const uint8_t* __restrict__ w, void* __restrict__ y, int64_t items) {
    const int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (item >= items) return;
    const DwQ q = dw_constants(a);
    const DwItem at = dw_decode(item, items, g.CP, g.OW, g.OH);
    const int cp = at.c, ow = at.ow, oh = at.oh;
    const int64_t b = at.b;
    const int ih0 = oh * g.sh - g.ph, iw0 = ow * g.sw - g.pw;
    const uint8_t* __restrict__ src = x + b * g.image + cp * 16;
    const uint8_t* __restrict__ wsrc = w + cp * 16;
    const uint32_t flipx = a.offx ? 0x80808080u : 0u, flipw = a.offw ? 0x80808080u : 0u;
    const int za = q.zx + a.offx;
    int acc[16];
    uint32_t sa[16], sb[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        acc[i] = 0;
        sa[i] = sb[i] = 0u;
    }
    int taps = 0;
    for (int i = 0; i < g.kh; ++i) {
        const unsigned ih = static_cast<unsigned>(ih0 + i * g.dh);             // negative: huge
        if (ih >= static_cast<unsigned>(g.H)) continue;
        for (int j = 0; j < g.kw; ++j) {
            const unsigned iw = static_cast<unsigned>(iw0 + j * g.dw);
            if (iw >= static_cast<unsigned>(g.W)) continue;
            const u32x4 xv = *reinterpret_cast<const u32x4*>(src + (static_cast<int64_t>(ih) * g.W + iw) * g.C) ^ flipx;
            const u32x4 wv = *reinterpret_cast<const u32x4*>(wsrc + static_cast<int64_t>(i * g.kw + j) * g.C) ^ flipw;
            dw_mac_packet(acc, xv, wv);
            dw_add_packet(sa, xv);
            dw_add_packet(sb, wv);
            ++taps;
        }
    }
    uint32_t out[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t ab[4], ga[4], gb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ab[k] = static_cast<uint32_t>(acc[4 * i + k]);
            ga[k] = sa[4 * i + k];
            gb[k] = sb[4 * i + k];
        }
        out[i] = dw_group(ab, ga, gb, taps, za, cp * 16 + 4 * i, a, q, y, item * 16 + 4 * i);
    }
    if (q.levels_out) *reinterpret_cast<u32x4*>(static_cast<uint8_t*>(y) + item * 16) = u32x4{out[0], out[1], out[2], out[3]};
}

// ------------------------------------------------------------------------------------------------
// generic: one lane per output element.  item = ((b OH + oh) OW + ow) C + c
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void dwconv_w8_generic_kernel(DwGeom g, DwArg a, const uint8_t* __restrict__ x,
                                                                   const uint8_t* __restrict__ w, void* __restrict__ y, int64_t items) {
    const int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (item >= items) return;
    const DwQ q = dw_constants(a);
    const DwItem at = dw_decode(item, items, g.C, g.OW, g.OH);
    const int c = at.c, ow = at.ow, oh = at.oh;
    const int64_t b = at.b;
    const int ih0 = oh * g.sh - g.ph, iw0 = ow * g.sw - g.pw;
    const uint8_t* __restrict__ src = x + b * g.image + c;
    const uint8_t fx = a.offx ? 0x80 : 0, fw = a.offw ? 0x80 : 0;
    const int za = q.zx + a.offx, zb = a.w_zero[c] + a.offw;
    int I = 0;
    for (int i = 0; i < g.kh; ++i) {
        const unsigned ih = static_cast<unsigned>(ih0 + i * g.dh);
        if (ih >= static_cast<unsigned>(g.H)) continue;
        for (int j = 0; j < g.kw; ++j) {
            const unsigned iw = static_cast<unsigned>(iw0 + j * g.dw);
            if (iw >= static_cast<unsigned>(g.W)) continue;
            const int av = static_cast<int>(static_cast<uint8_t>(src[(static_cast<int64_t>(ih) * g.W + iw) * g.C] ^ fx)) - za;
            const int bv = static_cast<int>(static_cast<uint8_t>(w[static_cast<int64_t>(i * g.kw + j) * g.C + c] ^ fw)) - zb;
            I += av * bv;
        }
    }
    w8o_store1(y, item, dw_value(I, a.w_scale[c], dw_bias(q, c), q), q);
}

// ------------------------------------------------------------------------------------------------
// host side: the checked geometry and the plan
// ------------------------------------------------------------------------------------------------
struct DwShape {            // a checked geometry
    int64_t OH, OW, pixels, x_bytes, y_elems;
    DwGeom g;
};

struct DwPlan {
    int family, block, pix, unrolled, ustride;
    int64_t grid;
};

inline int64_t dw_items(const DwShape& s, int pix) { return s.pixels / s.OW * ceil_div(s.OW, pix) * s.g.CP; }

inline DwPlan plan_dwconv(const DwShape& s, bool aligned, bool y_aligned) {
    DwPlan pl = {};
    pl.block = kBlock;
    pl.pix = 1;
    if (!(aligned && y_aligned && s.g.C % 16 == 0)) {
        pl.family = LSQ_DWCONV_W8_GENERIC;
        pl.grid = ceil_div(s.y_elems, kBlock);
        return pl;
    }
    pl.family = LSQ_DWCONV_W8_PACKETS;
    const DwGeom& g = s.g;
    if (g.kh == 3 && g.kw == 3 && g.dh == 1 && g.dw == 1 && g.sh == g.sw && (g.sh == 1 || g.sh == 2)) {
        pl.unrolled = 3;
        pl.ustride = g.sh;
        pl.pix = g.sh == 1 ? kDwPixS1 : kDwPixS2;
        const int64_t fill = static_cast<int64_t>(device_info().cu_count) * kDwBlocksPerCU;
        while (pl.pix > 1 && ceil_div(dw_items(s, pl.pix), kBlock) < fill) pl.pix /= 2;
    }
    pl.grid = ceil_div(dw_items(s, pl.pix), kBlock);
    return pl;
}

template <int S, int PMAX>
static void dw_launch_unrolled(const DwPlan& pl, const DwShape& s, const DwArg& a, const uint8_t* x, const uint8_t* w, void* y,
                               hipStream_t st) {
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(kBlock);
    const int64_t items = dw_items(s, pl.pix);
#if LSQ_DWCONV_W8_DOT4
    hipLaunchKernelGGL((dwconv_w8_packets_dot_kernel<S>), grid, block, 0, st, s.g, a, x, w, y, items);
#else
    if constexpr (PMAX >= 4) {
        if (pl.pix == 4) {
            hipLaunchKernelGGL((dwconv_w8_packets_kernel<3, S, 4>), grid, block, 0, st, s.g, a, x, w, y, items);
            return;
        }
    }
    if constexpr (PMAX >= 2) {
        if (pl.pix == 2) {
            hipLaunchKernelGGL((dwconv_w8_packets_kernel<3, S, 2>), grid, block, 0, st, s.g, a, x, w, y, items);
            return;
        }
    }
    hipLaunchKernelGGL((dwconv_w8_packets_kernel<3, S, 1>), grid, block, 0, st, s.g, a, x, w, y, items);
#endif
}

static hipError_t dw_launch(const DwPlan& pl, const DwShape& s, const DwArg& a, const uint8_t* x, const uint8_t* w, void* y, hipStream_t st) {
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(kBlock);
    if (pl.family == LSQ_DWCONV_W8_GENERIC) hipLaunchKernelGGL(dwconv_w8_generic_kernel, grid, block, 0, st, s.g, a, x, w, y, s.y_elems);
    else if (pl.unrolled == 3 && pl.ustride == 1) dw_launch_unrolled<1, kDwPixS1>(pl, s, a, x, w, y, st);
    else if (pl.unrolled == 3) dw_launch_unrolled<2, kDwPixS2>(pl, s, a, x, w, y, st);
    else hipLaunchKernelGGL(dwconv_w8_packets_loop_kernel, grid, block, 0, st, s.g, a, x, w, y, dw_items(s, 1));
    return hipGetLastError();
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_dwconv_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// the geometry's checks: those of lsq_hip_qconv_w8.h's convolution, then Cout == Cin and the tap limit; fills `s`
int check_geom(const char* what, const lsq_qconv_w8_geom* g, lsq::DwShape& s) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (g->B < 1 || g->Cin < 1 || g->H < 1 || g->W < 1)
        return fail(LSQ_EINVAL, "%s: x is [B, H, W, C] = [%lld, %lld, %lld, %lld], every extent must be at least 1", what,
                    static_cast<ll>(g->B), static_cast<ll>(g->H), static_cast<ll>(g->W), static_cast<ll>(g->Cin));
    if (g->Cout != g->Cin)
        return fail(LSQ_EINVAL, "%s: Cout = %lld on Cin = %lld: a depthwise convolution has one output channel per input channel (a "
                    "channel multiplier is not served)", what, static_cast<ll>(g->Cout), static_cast<ll>(g->Cin));
    if (g->kh < 1 || g->kw < 1)
        return fail(LSQ_EINVAL, "%s: the kernel is %lld x %lld, both must be positive", what, static_cast<ll>(g->kh), static_cast<ll>(g->kw));
    if (g->sh < 1 || g->sw < 1)
        return fail(LSQ_EINVAL, "%s: the stride is (%lld, %lld), both must be positive", what, static_cast<ll>(g->sh), static_cast<ll>(g->sw));
    if (g->dh < 1 || g->dw < 1)
        return fail(LSQ_EINVAL, "%s: the dilation is (%lld, %lld), both must be positive", what, static_cast<ll>(g->dh), static_cast<ll>(g->dw));
    if (g->ph < 0 || g->pw < 0)
        return fail(LSQ_EINVAL, "%s: the padding is (%lld, %lld), negative padding is not supported", what, static_cast<ll>(g->ph),
                    static_cast<ll>(g->pw));
    const int64_t lim = INT32_MAX;
    if (g->Cin > lim || g->H > lim || g->W > lim || g->ph > lim || g->pw > lim || g->H + 2 * g->ph > lim || g->W + 2 * g->pw > lim ||
        g->sh > lim || g->sw > lim || g->dh > lim || g->dw > lim)
        return fail(LSQ_EINVAL, "%s: C, a padded extent (H + 2 ph, W + 2 pw), stride or dilation is beyond 31 bits", what);
    const int64_t eh = g->H + 2 * g->ph - 1, ew = g->W + 2 * g->pw - 1;           // the last padded coordinate
    if (g->kh - 1 > eh / g->dh || g->kw - 1 > ew / g->dw)
        return fail(LSQ_EINVAL, "%s: an empty output: the dilated %lld x %lld kernel does not fit the padded [%lld, %lld] image", what,
                    static_cast<ll>(g->kh), static_cast<ll>(g->kw), static_cast<ll>(eh + 1), static_cast<ll>(ew + 1));
    if (g->kh > LSQ_DWCONV_W8_MAX_TAPS / g->kw)
        return fail(LSQ_EINVAL, "%s: a window of %lld x %lld taps, at most %d are served (the 32-bit sum stays exact)", what,
                    static_cast<ll>(g->kh), static_cast<ll>(g->kw), LSQ_DWCONV_W8_MAX_TAPS);
    s.OH = (eh - g->dh * (g->kh - 1)) / g->sh + 1;
    s.OW = (ew - g->dw * (g->kw - 1)) / g->sw + 1;
    const int64_t pix = s.OH * s.OW, img = g->H * g->W;                           // both below 2^62
    if (g->Cin > INT64_MAX / 16 / img || g->B > INT64_MAX / 16 / (img * g->Cin) || g->B > INT64_MAX / 16 / (pix * g->Cin))
        return fail(LSQ_EINVAL, "%s: the shapes are beyond 64-bit offsets", what);
    s.pixels = g->B * pix;
    s.x_bytes = g->B * img * g->Cin;
    s.y_elems = s.pixels * g->Cin;
    s.g = lsq::DwGeom{img * g->Cin, static_cast<int>(g->Cin), static_cast<int>(g->Cin / 16), static_cast<int>(g->H), static_cast<int>(g->W),
                      static_cast<int>(s.OH), static_cast<int>(s.OW), static_cast<int>(g->kh), static_cast<int>(g->kw),
                      static_cast<int>(g->sh), static_cast<int>(g->sw), static_cast<int>(g->ph), static_cast<int>(g->pw),
                      static_cast<int>(g->dh), static_cast<int>(g->dw)};
    return LSQ_OK;
}

int check_level_dtype(const char* what, const char* name, int code) {
    if (code != LSQ_DWCONV_W8_U8 && code != LSQ_DWCONV_W8_I8)
        return fail(LSQ_EINVAL, "%s: %s must be LSQ_DWCONV_W8_U8 (0) or LSQ_DWCONV_W8_I8 (1), got %d", what, name, code);
    return LSQ_OK;
}

// the output's checks, which fill the output side and `act` of `a`; the bytes of one element of y into `y_elem`
int check_out(const char* what, const lsq_dwconv_w8_out* o, lsq::DwArg& a, int64_t& y_elem) {
    if (!o) return fail(LSQ_EINVAL, "%s: NULL output description", what);
    if (int rc = check_out_side(what, *o, a, y_elem)) return rc;
    if (o->act < LSQ_DWCONV_W8_ACT_NONE || o->act > LSQ_DWCONV_W8_ACT_RELU6)
        return fail(LSQ_EINVAL, "%s: act must be 0 (none), 1 (ReLU) or 2 (ReLU6), got %lld", what, static_cast<ll>(o->act));
    a.act = static_cast<int>(o->act);
    return LSQ_OK;
}

int check_grid(const char* what, const lsq::DwPlan& pl) {
    if (pl.grid > INT32_MAX) return fail(LSQ_EINVAL, "%s: %lld workgroups are beyond a 31-bit grid", what, static_cast<ll>(pl.grid));
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_dwconv_w8_abi_version(void) { return LSQ_DWCONV_W8_ABI_VERSION; }

const char* lsq_dwconv_w8_last_error(void) { return g_last_error; }

int lsq_dwconv_w8_forward_levels(int level_dtype, const void* x_levels, const void* s_x, const void* zx, const lsq_qconv_w8_geom* geom,
                                 int w_level_dtype, const void* w_levels, const void* w_scale, const void* w_zero, const void* bias,
                                 int bias_dtype, const lsq_dwconv_w8_out* out, void* y, void* stream) {
    const char* what = "lsq_dwconv_w8_forward_levels";
    lsq::DwShape s;
    lsq::DwArg a{};
    int64_t y_elem = 1;
    if (int rc = check_out(what, out, a, y_elem)) return rc;
    if (int rc = check_geom(what, geom, s)) return rc;
    if (int rc = check_level_dtype(what, "level_dtype", level_dtype)) return rc;
    if (int rc = check_level_dtype(what, "w_level_dtype", w_level_dtype)) return rc;
    if (!x_levels || !s_x || !zx || !w_levels || !w_scale || !w_zero || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(s_x, 4) || !aligned_to(zx, 4)) return fail(LSQ_EINVAL, "%s: s_x and zx must be element-aligned", what);
    if (bias && bias_dtype != LSQ_F32 && bias_dtype != a.mid)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of mid_dtype, got dtype code %d", what, bias_dtype);
    if (!aligned_to(w_scale, 4) || !aligned_to(w_zero, 4) || (bias && !aligned_to(bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: w_scale, w_zero and bias must be element-aligned", what);
    if (!aligned_to(y, static_cast<uintptr_t>(y_elem))) return fail(LSQ_EINVAL, "%s: a floating y must be element-aligned", what);
    const int64_t y_bytes = s.y_elems * y_elem;
    if (overlap(y, y_bytes, x_levels, s.x_bytes))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap x's %lld: a convolution in place is not served", what, static_cast<ll>(y_bytes),
                    static_cast<ll>(s.x_bytes));
    // (the packet kernels read w_scale and w_zero in 16-byte packets from channel c0, c0 % 16 == 0: both must then be aligned too)
    const bool aligned = aligned_to(x_levels, 16) && aligned_to(w_levels, 16) && aligned_to(w_scale, 16) && aligned_to(w_zero, 16);
    const lsq::DwPlan pl = lsq::plan_dwconv(s, aligned, aligned_to(y, 16));
    if (int rc = check_grid(what, pl)) return rc;
    a.s_x = static_cast<const float*>(s_x);
    a.zx = static_cast<const int32_t*>(zx);
    a.w_scale = static_cast<const float*>(w_scale);
    a.w_zero = static_cast<const int32_t*>(w_zero);
    a.bias = bias;
    a.bias_dtype = bias_dtype;
    a.offx = level_dtype == LSQ_DWCONV_W8_I8 ? 128 : 0;
    a.offw = w_level_dtype == LSQ_DWCONV_W8_I8 ? 128 : 0;
    return hip_status(lsq::dw_launch(pl, s, a, static_cast<const uint8_t*>(x_levels), static_cast<const uint8_t*>(w_levels), y,
                                     static_cast<hipStream_t>(stream)), what);
}

int lsq_dwconv_w8_plan(const lsq_qconv_w8_geom* geom, int aligned, int y_aligned, int32_t* out8) {
    const char* what = "lsq_dwconv_w8_plan";
    lsq::DwShape s;
    if (int rc = check_geom(what, geom, s)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::DwPlan pl = lsq::plan_dwconv(s, aligned != 0, y_aligned != 0);
    if (int rc = check_grid(what, pl)) return rc;
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.block;
    out8[3] = pl.pix;
    out8[4] = static_cast<int32_t>(s.OH);
    out8[5] = static_cast<int32_t>(s.OW);
    out8[6] = pl.unrolled;
    out8[7] = pl.ustride;
    return LSQ_OK;
}

}  // extern "C"
