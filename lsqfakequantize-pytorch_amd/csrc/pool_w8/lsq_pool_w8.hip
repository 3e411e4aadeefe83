// lsq_pool_w8.hip -- 2-D max and average pooling on channels-last 8-bit levels on gfx950 (include/lsq_hip_pool_w8.h, which
// states the contract): the kernels and the C ABI of liblsq_hip_pool_w8.so.  Bandwidth kernels on 16-byte packets along C.
//
//  * MAX, packets (C % 16 == 0, x and y 16-byte aligned): a lane owns one 16-channel packet of ONE output pixel
//    (pool_w8_max_packets_kernel<1, K>).  For the 2 x 2 and 3 x 3 windows without dilation (K = 2, 3) all K K loads are issued
//    up front from addresses clamped into the input, and a tap outside is replaced by the least level afterwards; every other
//    window (K = 0) walks its taps in a loop, one bounds test per tap.  The CU has no packed byte max: a packet is widened to
//    eight pairs of 16-bit lanes (even and odd bytes) and reduced with the packed 16-bit max; int8 levels are biased by 0x80
//    on load and store, so both level dtypes share the unsigned path.  The accumulator starts at 0, the least biased level:
//    every legal window holds a tap inside the input.
//    The experiment's variant, NOT shipped: built with -DLSQ_POOL_W8_MAX_PIX=N (tools/exp_pool_w8_ab.py --build-variants), a
//    lane owns N adjacent output pixels, reduces each input column once and folds the column maximum into every output whose
//    window holds it.  It was measured and rejected; the PIX > 1 branches of the kernel below (`span`,
//    `use[]`, pool_wide_fold) exist for that build alone and compile away in the library, where PIX == 1.
//  * AVERAGE, packets, one window per lane: 16 sums of biased bytes in registers over the window clipped to the input,
//    S = sum - taps (z_x + bias), one epilogue per output, 16-byte stores.
//  * AVERAGE, packets, a window shared by L lanes of a workgroup (global pooling): lanes stride over the clipped window's
//    taps for their packet, the partial sums are combined by a tree in LDS (integers: any order), lane 0 of the window runs
//    the epilogue.  No atomics, no second launch.
//  * GENERIC (every other legal call): one lane per output element, byte loads; the average's epilogue function is the
//    packet kernels'.  Correct, not tuned.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../lsq_w8_out_side.hpp"
#include "../lsq_w8_out_side_host.hpp"
#include "../../../include/lsq_hip_pool_w8.h"

#ifndef LSQ_POOL_W8_MAX_PIX
#define LSQ_POOL_W8_MAX_PIX 1       // the library's; N > 1 only in the experiment's variant build (measured, rejected)
#endif

namespace lsq {

typedef __attribute__((ext_vector_type(2))) unsigned short pool_u16x2;

constexpr int kPoolMaxPix = LSQ_POOL_W8_MAX_PIX;
constexpr int kPoolSharedMinTaps = 10;          // below: a lane owns its window (2 x 2, 3 x 3)
constexpr int kPoolBlocksPerCU = 2;             // the grid "fills the chip" from here
constexpr int64_t kPoolMaxTaps = int64_t(1) << 23;

struct PoolGeom {           // kernel argument; the host has checked that the coordinates fit 32 bits
    int64_t image;          // H W C, the bytes of one image of x
    int C, P;               // channels, 16-channel packets
    int H, W, OH, OW, kh, kw, sh, sw, ph, pw, dh, dw;
};

struct PoolAvgArg {         // kernel argument: the average pool's constants
    const float* s_x;
    const int32_t* zx;
    const float* scale;     // the output quantizer; NULL: a floating y
    const float* shift;
    float qmin, qmax, tmin, tmax;
    float divisor;          // has_divisor: float(divisor_override)
    int has_divisor, include_pad;
    int mid;                // LSQ_F32 / LSQ_BF16 / LSQ_F16
    int off;                // 128 for int8 levels (biased on load), 0 for uint8
};

struct PoolAvgQ : W8OutSide {       // the same, read once per thread
    float s_x;
    int zz;                 // z_x + off: what one tap's biased byte carries too much
};

__device__ __forceinline__ PoolAvgQ pool_avg_constants(const PoolAvgArg& a) {
    PoolAvgQ q;
    w8o_constants(q, a);
    q.s_x = a.s_x[0];
    q.zz = a.zx[0] + a.off;
    return q;
}

// the window of output (oh, ow) clipped to the input, and ATen's divisor
struct PoolWindow {
    int hs, ws, nh, nw;     // first tap inside, taps inside per axis (both at least 1)
    float D;
};

__device__ __forceinline__ PoolWindow pool_window(const PoolGeom& g, const PoolAvgArg& a, int oh, int ow) {
    const int h0 = oh * g.sh - g.ph, w0 = ow * g.sw - g.pw;
    PoolWindow w;
    w.hs = max(h0, 0);
    w.ws = max(w0, 0);
    w.nh = min(h0 + g.kh, g.H) - w.hs;
    w.nw = min(w0 + g.kw, g.W) - w.ws;
    if (a.has_divisor) w.D = a.divisor;
    else if (a.include_pad) w.D = static_cast<float>((min(h0 + g.kh, g.H + g.ph) - h0) * (min(w0 + g.kw, g.W + g.pw) - w0));
    else w.D = static_cast<float>(w.nh * w.nw);
    return w;
}

// the fp32 steps of the contract on the exact integer S and the rounding to mid_dtype.  The rounding is w8o_round_mid's, written
// out as branches: with the select form pool_w8_avg_lane_kernel<2> held 45 VGPRs for 32 and measured 3-4 % slower on the 2 x 2
// average pool in both GPU calls that timed it (profiles/r25_w8_out_side_ab.txt)
__device__ __forceinline__ float pool_avg_value(int64_t S, float D, const PoolAvgQ& q) {
    const float v = __fdiv_rn(__fmul_rn(static_cast<float>(S), q.s_x), D);
    if (q.mid == LSQ_BF16) return static_cast<float>(io_bf16::to_elem(v));
    if (q.mid == LSQ_F16) return static_cast<float>(io_f16::to_elem(v));
    return v;
}

// a packet of 16 outputs from their biased sums: `at` in elements of y, y 16-byte aligned
__device__ __forceinline__ void pool_avg_store16(void* y, int64_t at, const uint32_t (&sum)[16], int64_t taps, float D, const PoolAvgQ& q) {
    float u[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) u[i] = pool_avg_value(static_cast<int64_t>(sum[i]) - taps * q.zz, D, q);
    w8o_store16(y, at, u, q);
}

// sum[16] += the 16 biased bytes of a packet
__device__ __forceinline__ void pool_add_packet(uint32_t (&sum)[16], u32x4 v, uint32_t flip) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = v[i] ^ flip;
        sum[4 * i] += w & 0xffu;
        sum[4 * i + 1] += (w >> 8) & 0xffu;
        sum[4 * i + 2] += (w >> 16) & 0xffu;
        sum[4 * i + 3] += w >> 24;
    }
}

// ------------------------------------------------------------------------------------------------
// max pool
// ------------------------------------------------------------------------------------------------
struct PoolWide {           // 16 bytes as eight pairs of 16-bit lanes: e[i] the even bytes of word i, o[i] the odd ones
    pool_u16x2 e[4], o[4];
};

__device__ __forceinline__ void pool_wide_max(PoolWide& acc, u32x4 v, uint32_t flip) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = v[i] ^ flip;
        acc.e[i] = __builtin_elementwise_max(acc.e[i], __builtin_bit_cast(pool_u16x2, w & 0x00ff00ffu));
        acc.o[i] = __builtin_elementwise_max(acc.o[i], __builtin_bit_cast(pool_u16x2, (w >> 8) & 0x00ff00ffu));
    }
}

__device__ __forceinline__ void pool_wide_fold(PoolWide& acc, const PoolWide& col) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc.e[i] = __builtin_elementwise_max(acc.e[i], col.e[i]);
        acc.o[i] = __builtin_elementwise_max(acc.o[i], col.o[i]);
    }
}

__device__ __forceinline__ u32x4 pool_narrow(const PoolWide& a, uint32_t flip) {
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (__builtin_bit_cast(uint32_t, a.e[i]) | __builtin_bit_cast(uint32_t, a.o[i]) << 8) ^ flip;
    return v;
}

// where a tap lies: clamped into the input (a load from there is always legal), and whether it was inside
__device__ __forceinline__ int pool_clamp(int v, int n, bool& inside) {
    inside = inside && static_cast<unsigned>(v) < static_cast<unsigned>(n);
    return min(max(v, 0), n - 1);
}

// item = ((b OH + oh) OWG + owg) P + packet, OWG = ceil(OW / PIX) groups of adjacent output pixels; PIX == 1 in the library
// (OWG = OW, `span` = kw, every `use[]` true), PIX > 1 in the experiment's variant build alone.  K > 0 (PIX == 1 only):
// a K x K window without dilation known at compile time -- all K K loads are issued before the first max (clamped addresses,
// a tap outside replaced by the least level afterwards); a lane that loads tap after tap in a loop is bound by K K load latencies
template <int PIX, int K>
__global__ __launch_bounds__(kBlock) void pool_w8_max_packets_kernel(PoolGeom g, const uint8_t* __restrict__ x, uint8_t* __restrict__ y,
                                                                      uint32_t flip, int64_t items) {
    const int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (item >= items) return;
    const int owg_n = (g.OW + PIX - 1) / PIX;
    int64_t t = item / g.P;
    const int cp = static_cast<int>(item - t * g.P);
    const int owg = static_cast<int>(t % owg_n);
    t /= owg_n;
    const int oh = static_cast<int>(t % g.OH);
    const int64_t b = t / g.OH;
    const int ow0 = owg * PIX;
    const int ih0 = oh * g.sh - g.ph, iw0 = ow0 * g.sw - g.pw;
    const uint8_t* __restrict__ src = x + b * g.image + cp * 16;
    PoolWide acc[PIX];
#pragma unroll
    for (int p = 0; p < PIX; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[p].e[i] = acc[p].o[i] = pool_u16x2{0, 0};
    if constexpr (K > 0) {
        static_assert(PIX == 1, "the unrolled window is the one-pixel kernel's");
        u32x4 v[K * K];
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                bool inside = true;
                const int ih = pool_clamp(ih0 + i, g.H, inside), iw = pool_clamp(iw0 + j, g.W, inside);
                const u32x4 t = *reinterpret_cast<const u32x4*>(src + (static_cast<int64_t>(ih) * g.W + iw) * g.C);
                v[i * K + j] = inside ? t : u32x4{flip, flip, flip, flip};
            }
#pragma unroll
        for (int t = 0; t < K * K; ++t) pool_wide_max(acc[0], v[t], flip);
        *reinterpret_cast<u32x4*>(y + ((b * g.OH + oh) * g.OW + ow0) * g.C + cp * 16) = pool_narrow(acc[0], flip);
        return;
    }
    const int span = PIX == 1 ? g.kw : (PIX - 1) * g.sw + (g.kw - 1) * g.dw + 1;          // input columns the lane's windows cover
    for (int j = 0; j < span; ++j) {
        const int col_at = PIX == 1 ? j * g.dw : j;
        const unsigned iw = static_cast<unsigned>(iw0 + col_at);                          // negative: huge
        if (iw >= static_cast<unsigned>(g.W)) continue;
        bool use[PIX];
        bool any = false;
#pragma unroll
        for (int p = 0; p < PIX; ++p) {
            const int r = col_at - p * g.sw;
            use[p] = PIX == 1 || (r >= 0 && r % g.dw == 0 && r / g.dw < g.kw);
            any = any || use[p];
        }
        if (!any) continue;
        PoolWide col;
#pragma unroll
        for (int i = 0; i < 4; ++i) col.e[i] = col.o[i] = pool_u16x2{0, 0};
        for (int i = 0; i < g.kh; ++i) {
            const unsigned ih = static_cast<unsigned>(ih0 + i * g.dh);
            if (ih < static_cast<unsigned>(g.H))
                pool_wide_max(col, *reinterpret_cast<const u32x4*>(src + (static_cast<int64_t>(ih) * g.W + iw) * g.C), flip);
        }
#pragma unroll
        for (int p = 0; p < PIX; ++p)
            if (use[p]) pool_wide_fold(acc[p], col);
    }
    uint8_t* __restrict__ dst = y + ((b * g.OH + oh) * g.OW + ow0) * g.C + cp * 16;
#pragma unroll
    for (int p = 0; p < PIX; ++p)
        if (ow0 + p < g.OW) *reinterpret_cast<u32x4*>(dst + static_cast<int64_t>(p) * g.C) = pool_narrow(acc[p], flip);
}

// one lane per output byte
__global__ __launch_bounds__(kBlock) void pool_w8_max_generic_kernel(PoolGeom g, const uint8_t* __restrict__ x, uint8_t* __restrict__ y,
                                                                      uint32_t flip, int64_t items) {
    const int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (item >= items) return;
    int64_t t = item / g.C;
    const int c = static_cast<int>(item - t * g.C);
    const int ow = static_cast<int>(t % g.OW);
    t /= g.OW;
    const int oh = static_cast<int>(t % g.OH);
    const int64_t b = t / g.OH;
    const int ih0 = oh * g.sh - g.ph, iw0 = ow * g.sw - g.pw;
    const uint8_t* __restrict__ src = x + b * g.image + c;
    const uint8_t f = static_cast<uint8_t>(flip & 0xffu);
    unsigned m = 0;
    for (int i = 0; i < g.kh; ++i) {
        const unsigned ih = static_cast<unsigned>(ih0 + i * g.dh);
        if (ih >= static_cast<unsigned>(g.H)) continue;
        for (int j = 0; j < g.kw; ++j) {
            const unsigned iw = static_cast<unsigned>(iw0 + j * g.dw);
            if (iw < static_cast<unsigned>(g.W))
                m = max(m, static_cast<unsigned>(static_cast<uint8_t>(src[(static_cast<int64_t>(ih) * g.W + iw) * g.C] ^ f)));
        }
    }
    y[item] = static_cast<uint8_t>(m) ^ f;
}

// ------------------------------------------------------------------------------------------------
// average pool
// ------------------------------------------------------------------------------------------------
// item = ((b OH + oh) OW + ow) P + packet: one lane per item.  K > 0: a K x K window known at compile time, every load issued
// before the first add (a tap outside the clipped window is loaded from its last row / column and adds the biased 0)
template <int K>
__global__ __launch_bounds__(kBlock) void pool_w8_avg_lane_kernel(PoolGeom g, PoolAvgArg a, const uint8_t* __restrict__ x,
                                                                   void* __restrict__ y, uint32_t flip, int64_t items) {
    const int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (item >= items) return;
    const PoolAvgQ q = pool_avg_constants(a);
    int64_t t = item / g.P;
    const int cp = static_cast<int>(item - t * g.P);
    const int ow = static_cast<int>(t % g.OW);
    t /= g.OW;
    const int oh = static_cast<int>(t % g.OH);
    const int64_t b = t / g.OH;
    const PoolWindow w = pool_window(g, a, oh, ow);
    const uint8_t* __restrict__ src = x + b * g.image + cp * 16;
    uint32_t sum[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) sum[i] = 0u;
    if constexpr (K > 0) {
        u32x4 v[K * K];
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int ih = w.hs + min(i, w.nh - 1), iw = w.ws + min(j, w.nw - 1);
                const u32x4 t = *reinterpret_cast<const u32x4*>(src + (static_cast<int64_t>(ih) * g.W + iw) * g.C);
                v[i * K + j] = (i < w.nh && j < w.nw) ? t : u32x4{flip, flip, flip, flip};
            }
#pragma unroll
        for (int t = 0; t < K * K; ++t) pool_add_packet(sum, v[t], flip);
    } else {
        for (int i = 0; i < w.nh; ++i) {
            const uint8_t* __restrict__ row = src + (static_cast<int64_t>(w.hs + i) * g.W + w.ws) * g.C;
            for (int j = 0; j < w.nw; ++j)
                pool_add_packet(sum, *reinterpret_cast<const u32x4*>(row + static_cast<int64_t>(j) * g.C), flip);
        }
    }
    pool_avg_store16(y, item * 16, sum, static_cast<int64_t>(w.nh) * w.nw, w.D, q);
}

// L = kBlock / CPW lanes share an item: thread = slot CPW + (item within the workgroup), the slots stride over the taps
__global__ __launch_bounds__(kBlock) void pool_w8_avg_shared_kernel(PoolGeom g, PoolAvgArg a, const uint8_t* __restrict__ x,
                                                                     void* __restrict__ y, uint32_t flip, int64_t items, int cpw) {
    __shared__ alignas(16) uint32_t part[kBlock * 16];
    const int tid = static_cast<int>(threadIdx.x);
    const int L = kBlock / cpw, slot = tid / cpw;
    const int64_t item = static_cast<int64_t>(blockIdx.x) * cpw + (tid - slot * cpw);
    const bool live = item < items;
    uint32_t sum[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) sum[i] = 0u;
    PoolWindow w = {};
    if (live) {
        int64_t t = item / g.P;
        const int cp = static_cast<int>(item - t * g.P);
        const int ow = static_cast<int>(t % g.OW);
        t /= g.OW;
        const int oh = static_cast<int>(t % g.OH);
        const int64_t b = t / g.OH;
        w = pool_window(g, a, oh, ow);
        const uint8_t* __restrict__ src = x + b * g.image + cp * 16;
        const unsigned taps = static_cast<unsigned>(w.nh) * static_cast<unsigned>(w.nw), nw = static_cast<unsigned>(w.nw);
        for (unsigned k = static_cast<unsigned>(slot); k < taps; k += static_cast<unsigned>(L)) {
            const unsigned i = k / nw, j = k - i * nw;
            pool_add_packet(sum, *reinterpret_cast<const u32x4*>(src + (static_cast<int64_t>(w.hs + i) * g.W + (w.ws + j)) * g.C), flip);
        }
    }
    u32x4* mine = reinterpret_cast<u32x4*>(part + tid * 16);
    for (int s = L >> 1; s >= 1; s >>= 1) {                  // integers: any order
        if (slot >= s && slot < 2 * s) {
#pragma unroll
            for (int i = 0; i < 4; ++i) mine[i] = u32x4{sum[4 * i], sum[4 * i + 1], sum[4 * i + 2], sum[4 * i + 3]};
        }
        __syncthreads();
        if (slot < s) {
            const u32x4* other = reinterpret_cast<const u32x4*>(part + (tid + s * cpw) * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const u32x4 v = other[i];
                sum[4 * i] += v[0];
                sum[4 * i + 1] += v[1];
                sum[4 * i + 2] += v[2];
                sum[4 * i + 3] += v[3];
            }
        }                                                   // (the next step's writers are not this step's partners)
    }
    if (live && slot == 0) {
        const PoolAvgQ q = pool_avg_constants(a);
        pool_avg_store16(y, item * 16, sum, static_cast<int64_t>(w.nh) * w.nw, w.D, q);
    }
}

// one lane per output element
__global__ __launch_bounds__(kBlock) void pool_w8_avg_generic_kernel(PoolGeom g, PoolAvgArg a, const uint8_t* __restrict__ x,
                                                                      void* __restrict__ y, uint32_t flip, int64_t items) {
    const int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (item >= items) return;
    const PoolAvgQ q = pool_avg_constants(a);
    int64_t t = item / g.C;
    const int c = static_cast<int>(item - t * g.C);
    const int ow = static_cast<int>(t % g.OW);
    t /= g.OW;
    const int oh = static_cast<int>(t % g.OH);
    const int64_t b = t / g.OH;
    const PoolWindow w = pool_window(g, a, oh, ow);
    const uint8_t* __restrict__ src = x + b * g.image + c;
    const uint8_t f = static_cast<uint8_t>(flip & 0xffu);
    uint32_t sum = 0u;
    for (int i = 0; i < w.nh; ++i)
        for (int j = 0; j < w.nw; ++j) sum += static_cast<uint8_t>(src[(static_cast<int64_t>(w.hs + i) * g.W + (w.ws + j)) * g.C] ^ f);
    const int64_t taps = static_cast<int64_t>(w.nh) * w.nw;
    w8o_store1(y, item, pool_avg_value(static_cast<int64_t>(sum) - taps * q.zz, w.D, q), q);
}

// ------------------------------------------------------------------------------------------------
// host side: the checked geometry and the plans
// ------------------------------------------------------------------------------------------------
struct PoolShape {          // a checked geometry
    int64_t OH, OW, windows, taps, x_bytes, y_elems;
    PoolGeom g;
};

struct PoolPlan {
    int family, block, per, lds, cpw, unrolled;     // per: pixels per lane (max) / lanes per window (average); unrolled: K or 0
    int64_t grid;
};

// K of a K x K window without dilation that the packet kernels have unrolled (2, 3), else 0
inline int pool_unrolled(const PoolGeom& g) {
    return (g.kh == g.kw && g.dh == 1 && g.dw == 1 && (g.kh == 2 || g.kh == 3)) ? g.kh : 0;
}

inline PoolPlan plan_pool_max(const PoolShape& s, bool aligned) {
    PoolPlan pl = {};
    pl.block = kBlock;
    if (aligned && s.g.C % 16 == 0) {
        pl.family = LSQ_POOL_W8_PACKETS;
        pl.per = kPoolMaxPix;
        pl.unrolled = kPoolMaxPix == 1 ? pool_unrolled(s.g) : 0;
        pl.grid = ceil_div(s.windows / s.OW * ceil_div(s.OW, kPoolMaxPix) * s.g.P, kBlock);
    } else {
        pl.family = LSQ_POOL_W8_GENERIC;
        pl.per = 1;
        pl.grid = ceil_div(s.y_elems, kBlock);
    }
    return pl;
}

inline PoolPlan plan_pool_avg(const PoolShape& s, bool aligned) {
    PoolPlan pl = {};
    pl.block = kBlock;
    pl.per = 1;
    if (!(aligned && s.g.C % 16 == 0)) {
        pl.family = LSQ_POOL_W8_GENERIC;
        pl.grid = ceil_div(s.y_elems, kBlock);
        return pl;
    }
    const int64_t items = s.windows * s.g.P, fill = static_cast<int64_t>(device_info().cu_count) * kPoolBlocksPerCU;
    int lanes = 1;
    if (s.taps >= kPoolSharedMinTaps) {
        int cap = 1;
        while (cap < kBlock && cap * 2 <= s.taps) cap *= 2;
        while (lanes < cap && ceil_div(items, kBlock / lanes) < fill) lanes *= 2;
    }
    pl.per = lanes;
    if (lanes == 1) {
        pl.family = LSQ_POOL_W8_PACKETS;
        pl.unrolled = pool_unrolled(s.g);
        pl.grid = ceil_div(items, kBlock);
    } else {
        pl.family = LSQ_POOL_W8_PACKETS_SHARED;
        pl.cpw = kBlock / lanes;
        pl.lds = kBlock * 16 * 4;
        pl.grid = ceil_div(items, pl.cpw);
    }
    return pl;
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_pool_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// torch.nn.functional's output extent; 0: empty
int64_t out_extent(int64_t in, int64_t k, int64_t s, int64_t p, int64_t d, bool ceil_mode) {
    const int64_t num = in + 2 * p - d * (k - 1) - 1;
    if (num < 0) return 0;
    int64_t out = (ceil_mode ? (num + s - 1) / s : num / s) + 1;
    if (ceil_mode && (out - 1) * s >= in + p) --out;          // the last window starts inside the input or its left padding
    return out;
}

int check_geom(const char* what, const lsq_pool_w8_geom* g, bool average, lsq::PoolShape& s) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (g->B < 1 || g->C < 1 || g->H < 1 || g->W < 1)
        return fail(LSQ_EINVAL, "%s: x is [B, H, W, C] = [%lld, %lld, %lld, %lld], every extent must be at least 1", what,
                    static_cast<ll>(g->B), static_cast<ll>(g->H), static_cast<ll>(g->W), static_cast<ll>(g->C));
    if (g->kh < 1 || g->kw < 1)
        return fail(LSQ_EINVAL, "%s: the kernel is %lld x %lld, both must be positive", what, static_cast<ll>(g->kh), static_cast<ll>(g->kw));
    if (g->sh < 1 || g->sw < 1)
        return fail(LSQ_EINVAL, "%s: the stride is (%lld, %lld), both must be positive", what, static_cast<ll>(g->sh), static_cast<ll>(g->sw));
    if (g->dh < 1 || g->dw < 1)
        return fail(LSQ_EINVAL, "%s: the dilation is (%lld, %lld), both must be positive", what, static_cast<ll>(g->dh), static_cast<ll>(g->dw));
    if (average && (g->dh != 1 || g->dw != 1))
        return fail(LSQ_EINVAL, "%s: the average pool has no dilation, got (%lld, %lld)", what, static_cast<ll>(g->dh), static_cast<ll>(g->dw));
    if (g->ph < 0 || g->pw < 0 || g->ph > g->kh / 2 || g->pw > g->kw / 2)
        return fail(LSQ_EINVAL, "%s: the padding (%lld, %lld) must be non-negative and at most half the kernel (%lld, %lld)", what,
                    static_cast<ll>(g->ph), static_cast<ll>(g->pw), static_cast<ll>(g->kh), static_cast<ll>(g->kw));
    const int64_t lim = INT32_MAX / 4;
    if (g->C > lim || g->H > lim || g->W > lim || g->kh > lim || g->kw > lim || g->sh > lim || g->sw > lim || g->dh > lim || g->dw > lim ||
        g->dh * (g->kh - 1) > lim || g->dw * (g->kw - 1) > lim)
        return fail(LSQ_EINVAL, "%s: an extent, stride or dilated kernel is beyond 29 bits", what);
    if (g->kh > lsq::kPoolMaxTaps / g->kw)
        return fail(LSQ_EINVAL, "%s: a window of %lld x %lld taps, at most 2^23 are served (the 32-bit sum stays exact)", what,
                    static_cast<ll>(g->kh), static_cast<ll>(g->kw));
    if ((g->ph > 0 && g->dh > g->H) || (g->pw > 0 && g->dw > g->W))
        return fail(LSQ_EINVAL, "%s: with padding and a dilation (%lld, %lld) beyond the [%lld, %lld] input a window may hold no tap of it",
                    what, static_cast<ll>(g->dh), static_cast<ll>(g->dw), static_cast<ll>(g->H), static_cast<ll>(g->W));
    s.OH = out_extent(g->H, g->kh, g->sh, g->ph, g->dh, g->ceil_mode != 0);
    s.OW = out_extent(g->W, g->kw, g->sw, g->pw, g->dw, g->ceil_mode != 0);
    if (s.OH < 1 || s.OW < 1)
        return fail(LSQ_EINVAL, "%s: an empty output: the dilated %lld x %lld kernel does not fit the padded image", what,
                    static_cast<ll>(g->kh), static_cast<ll>(g->kw));
    const int64_t img = g->H * g->W, pix = s.OH * s.OW;
    if (g->C > INT64_MAX / 8 / img || g->B > INT64_MAX / 8 / (img * g->C) || g->B > INT64_MAX / 8 / (pix * g->C) / 16)
        return fail(LSQ_EINVAL, "%s: the shapes are beyond 64-bit offsets", what);
    s.windows = g->B * pix;
    s.taps = g->kh * g->kw;
    s.x_bytes = g->B * img * g->C;
    s.y_elems = s.windows * g->C;
    s.g = lsq::PoolGeom{img * g->C, static_cast<int>(g->C), static_cast<int>(g->C / 16), static_cast<int>(g->H), static_cast<int>(g->W),
                        static_cast<int>(s.OH), static_cast<int>(s.OW), static_cast<int>(g->kh), static_cast<int>(g->kw),
                        static_cast<int>(g->sh), static_cast<int>(g->sw), static_cast<int>(g->ph), static_cast<int>(g->pw),
                        static_cast<int>(g->dh), static_cast<int>(g->dw)};
    return LSQ_OK;
}

int check_level_dtype(const char* what, int code) {
    if (code != LSQ_POOL_W8_U8 && code != LSQ_POOL_W8_I8)
        return fail(LSQ_EINVAL, "%s: level_dtype must be LSQ_POOL_W8_U8 (0) or LSQ_POOL_W8_I8 (1), got %d", what, code);
    return LSQ_OK;
}

int check_buffers(const char* what, const void* x, int64_t x_bytes, const void* y, int64_t y_bytes) {
    if (!x || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (overlap(y, y_bytes, x, x_bytes))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap x's %lld: pooling in place is not served", what, static_cast<ll>(y_bytes),
                    static_cast<ll>(x_bytes));
    return LSQ_OK;
}

int check_grid(const char* what, const lsq::PoolPlan& pl) {
    if (pl.grid > INT32_MAX) return fail(LSQ_EINVAL, "%s: %lld workgroups are beyond a 31-bit grid", what, static_cast<ll>(pl.grid));
    return LSQ_OK;
}

// the average pool's constants, into `arg` (the caller's, zeroed); the bytes of one element of y into `y_elem`
int check_avg(const char* what, const lsq_pool_w8_avg* a, int level_dtype, lsq::PoolAvgArg& arg, int64_t& y_elem) {
    if (!a) return fail(LSQ_EINVAL, "%s: NULL constants", what);
    if (!a->s_x || !a->zx) return fail(LSQ_EINVAL, "%s: NULL s_x or zx", what);
    if (!aligned_to(a->s_x, 4) || !aligned_to(a->zx, 4)) return fail(LSQ_EINVAL, "%s: s_x and zx must be element-aligned", what);
    if (int rc = check_out_side(what, *a, arg, y_elem)) return rc;
    if (a->has_divisor && a->divisor_override < 1)
        return fail(LSQ_EINVAL, "%s: divisor_override = %lld, at least 1 is needed", what, static_cast<ll>(a->divisor_override));
    arg.s_x = static_cast<const float*>(a->s_x);
    arg.zx = static_cast<const int32_t*>(a->zx);
    arg.divisor = a->has_divisor ? static_cast<float>(a->divisor_override) : 0.0f;
    arg.has_divisor = a->has_divisor ? 1 : 0;
    arg.include_pad = a->count_include_pad ? 1 : 0;
    arg.off = level_dtype == LSQ_POOL_W8_I8 ? 128 : 0;
    return LSQ_OK;
}

void write_plan(const lsq::PoolPlan& pl, const lsq::PoolShape& s, int32_t* out8) {
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.block;
    out8[3] = pl.per;
    out8[4] = static_cast<int32_t>(s.OH);
    out8[5] = static_cast<int32_t>(s.OW);
    out8[6] = pl.lds;
    out8[7] = pl.family == LSQ_POOL_W8_PACKETS ? pl.unrolled : pl.cpw;
}

}  // namespace

extern "C" {

int lsq_pool_w8_abi_version(void) { return LSQ_POOL_W8_ABI_VERSION; }

const char* lsq_pool_w8_last_error(void) { return g_last_error; }

int lsq_pool_w8_max(int level_dtype, const void* x_levels, const lsq_pool_w8_geom* geom, void* y, void* stream) {
    const char* what = "lsq_pool_w8_max";
    lsq::PoolShape s;
    if (int rc = check_level_dtype(what, level_dtype)) return rc;
    if (int rc = check_geom(what, geom, false, s)) return rc;
    if (int rc = check_buffers(what, x_levels, s.x_bytes, y, s.y_elems)) return rc;
    const lsq::PoolPlan pl = lsq::plan_pool_max(s, aligned_to(x_levels, 16) && aligned_to(y, 16));
    if (int rc = check_grid(what, pl)) return rc;
    const uint32_t flip = level_dtype == LSQ_POOL_W8_I8 ? 0x80808080u : 0u;
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kBlock);
    const uint8_t* x = static_cast<const uint8_t*>(x_levels);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pl.family == LSQ_POOL_W8_PACKETS) {
        const int64_t items = s.windows / s.OW * ceil_div(s.OW, lsq::kPoolMaxPix) * s.g.P;
        uint8_t* yb = static_cast<uint8_t*>(y);
        if constexpr (lsq::kPoolMaxPix == 1) {
            if (pl.unrolled == 3) hipLaunchKernelGGL((lsq::pool_w8_max_packets_kernel<1, 3>), grid, block, 0, st, s.g, x, yb, flip, items);
            else if (pl.unrolled == 2) hipLaunchKernelGGL((lsq::pool_w8_max_packets_kernel<1, 2>), grid, block, 0, st, s.g, x, yb, flip, items);
            else hipLaunchKernelGGL((lsq::pool_w8_max_packets_kernel<1, 0>), grid, block, 0, st, s.g, x, yb, flip, items);
        } else {
            hipLaunchKernelGGL((lsq::pool_w8_max_packets_kernel<lsq::kPoolMaxPix, 0>), grid, block, 0, st, s.g, x, yb, flip, items);
        }
    } else {
        hipLaunchKernelGGL(lsq::pool_w8_max_generic_kernel, grid, block, 0, st, s.g, x, static_cast<uint8_t*>(y), flip, s.y_elems);
    }
    return hip_status(hipGetLastError(), what);
}

int lsq_pool_w8_avg_forward(int level_dtype, const void* x_levels, const lsq_pool_w8_geom* geom, const lsq_pool_w8_avg* avg, void* y,
                            void* stream) {
    const char* what = "lsq_pool_w8_avg_forward";
    lsq::PoolShape s;
    lsq::PoolAvgArg arg{};
    int64_t y_elem = 1;
    if (int rc = check_level_dtype(what, level_dtype)) return rc;
    if (int rc = check_geom(what, geom, true, s)) return rc;
    if (int rc = check_avg(what, avg, level_dtype, arg, y_elem)) return rc;
    if (int rc = check_buffers(what, x_levels, s.x_bytes, y, s.y_elems * y_elem)) return rc;
    if (!aligned_to(y, static_cast<uintptr_t>(y_elem))) return fail(LSQ_EINVAL, "%s: a floating y must be element-aligned", what);
    const lsq::PoolPlan pl = lsq::plan_pool_avg(s, aligned_to(x_levels, 16) && aligned_to(y, 16));
    if (int rc = check_grid(what, pl)) return rc;
    const uint32_t flip = level_dtype == LSQ_POOL_W8_I8 ? 0x80808080u : 0u;
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kBlock);
    const uint8_t* x = static_cast<const uint8_t*>(x_levels);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t items = s.windows * s.g.P;
    if (pl.family == LSQ_POOL_W8_PACKETS) {
        if (pl.unrolled == 3) hipLaunchKernelGGL(lsq::pool_w8_avg_lane_kernel<3>, grid, block, 0, st, s.g, arg, x, y, flip, items);
        else if (pl.unrolled == 2) hipLaunchKernelGGL(lsq::pool_w8_avg_lane_kernel<2>, grid, block, 0, st, s.g, arg, x, y, flip, items);
        else hipLaunchKernelGGL(lsq::pool_w8_avg_lane_kernel<0>, grid, block, 0, st, s.g, arg, x, y, flip, items);
    } else if (pl.family == LSQ_POOL_W8_PACKETS_SHARED)
        hipLaunchKernelGGL(lsq::pool_w8_avg_shared_kernel, grid, block, 0, st, s.g, arg, x, y, flip, items, pl.cpw);
    else hipLaunchKernelGGL(lsq::pool_w8_avg_generic_kernel, grid, block, 0, st, s.g, arg, x, y, flip, s.y_elems);
    return hip_status(hipGetLastError(), what);
}

int lsq_pool_w8_adaptive(int64_t out_h, int64_t out_w, lsq_pool_w8_geom* geom) {
    const char* what = "lsq_pool_w8_adaptive";
    if (!geom) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (geom->H < 1 || geom->W < 1 || out_h < 1 || out_w < 1)
        return fail(LSQ_EINVAL, "%s: an [%lld, %lld] output of an [%lld, %lld] input: every extent must be at least 1", what,
                    static_cast<ll>(out_h), static_cast<ll>(out_w), static_cast<ll>(geom->H), static_cast<ll>(geom->W));
    if (geom->H % out_h || geom->W % out_w)
        return fail(LSQ_EINVAL, "%s: the output size [%lld, %lld] does not divide the input's [%lld, %lld] evenly (not served)", what,
                    static_cast<ll>(out_h), static_cast<ll>(out_w), static_cast<ll>(geom->H), static_cast<ll>(geom->W));
    geom->kh = geom->sh = geom->H / out_h;
    geom->kw = geom->sw = geom->W / out_w;
    geom->ph = geom->pw = 0;
    geom->dh = geom->dw = 1;
    geom->ceil_mode = 0;
    return LSQ_OK;
}

int lsq_pool_w8_plan_max(const lsq_pool_w8_geom* geom, int aligned, int32_t* out8) {
    const char* what = "lsq_pool_w8_plan_max";
    lsq::PoolShape s;
    if (int rc = check_geom(what, geom, false, s)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::PoolPlan pl = lsq::plan_pool_max(s, aligned != 0);
    if (int rc = check_grid(what, pl)) return rc;
    write_plan(pl, s, out8);
    return LSQ_OK;
}

int lsq_pool_w8_plan_avg(const lsq_pool_w8_geom* geom, int aligned, int32_t* out8) {
    const char* what = "lsq_pool_w8_plan_avg";
    lsq::PoolShape s;
    if (int rc = check_geom(what, geom, true, s)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::PoolPlan pl = lsq::plan_pool_avg(s, aligned != 0);
    if (int rc = check_grid(what, pl)) return rc;
    write_plan(pl, s, out8);
    return LSQ_OK;
}

}  // extern "C"
