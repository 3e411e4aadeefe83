// lsq_eltwise_w8.hip -- elementwise ops on 8-bit levels on gfx950 (include/lsq_hip_eltwise_w8.h, which states the contract): the
// kernels and the C ABI of liblsq_hip_eltwise_w8.so.  Bandwidth kernels on 16-byte packets.
//
//  * TABLE, packets (x and y 16-byte aligned, n >= 16): the 256-byte table is staged once per workgroup into LDS, one byte per
//    thread (so the table needs no alignment), at a 256-byte-aligned offset: exactly one bank row of 64 dwords, so two lanes
//    either read the same dword (a broadcast) or different banks.  A lane owns P packets, kBlock packets apart (a wave's
//    accesses stay contiguous); all P loads are issued before the first lookup, each byte is looked up with a byte read of LDS,
//    the words are rebuilt and stored as 16 bytes.  The n % 16 last bytes are served by the first workgroup, one per lane, from
//    the same LDS copy: no second launch.
//    The experiment's variants, NOT shipped (tools/exp_eltwise_w8_ab.py --build-variants):
//    -DLSQ_ELTWISE_W8_LUT_P=N caps the packets per lane at N (the library: 2; 1 and 4 were measured and not kept);
//    -DLSQ_ELTWISE_W8_LUT_COPIES=N keeps N copies of the table, one per group of 32 lanes in turn (the library: 1).
//  * GATE MULTIPLY, packets (C % 16 == 0, x, g and y 16-byte aligned): a lane owns one 16-channel packet position (b, c0),
//    dequantizes its 16 gate values once and walks PIX pixels with them.  Within an image lane l takes the packets l, l + L,
//    l + 2 L, ... with L = C / 16 * ceil(H W / PIX) lanes per image, a multiple of C / 16: the packet's channel position is the
//    lane's at every step and adjacent lanes sit on adjacent packets.  All PIX loads are issued up front from clamped
//    addresses.  The epilogue is selects on mid_dtype, not branches; only the store branches on the kind of y.
//  * GENERIC (every other legal call): one lane per byte / element.  Correct, not tuned.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../lsq_w8_out_side.hpp"
#include "../lsq_w8_out_side_host.hpp"
#include "../../../include/lsq_hip_eltwise_w8.h"

#ifndef LSQ_ELTWISE_W8_LUT_P
#define LSQ_ELTWISE_W8_LUT_P 2          // the library's; 1 / 4 only in the experiment's variant builds
#endif
#ifndef LSQ_ELTWISE_W8_LUT_COPIES
#define LSQ_ELTWISE_W8_LUT_COPIES 1     // the library's; 2 / 4 only in the experiment's variant builds
#endif

namespace lsq {

constexpr int kEltLutMaxP = LSQ_ELTWISE_W8_LUT_P;
constexpr int kEltLutCopies = LSQ_ELTWISE_W8_LUT_COPIES;
constexpr int kEltMulMaxPix = 4;
constexpr int kEltBlocksPerCU = 2;              // the grid "fills the chip" from here
static_assert(kBlock == 256, "the table is staged one byte per thread");
static_assert(kEltLutMaxP == 1 || kEltLutMaxP == 2 || kEltLutMaxP == 4, "packets per lane: 1, 2 or 4");
static_assert(kEltLutCopies == 1 || kEltLutCopies == 2 || kEltLutCopies == 4, "table copies: 1, 2 or 4");

__device__ __forceinline__ int64_t elt_min(int64_t a, int64_t b) { return a < b ? a : b; }

// ------------------------------------------------------------------------------------------------
// the table op
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t elt_lookup4(const uint8_t* tab, uint32_t w) {
    return static_cast<uint32_t>(tab[w & 0xffu]) | static_cast<uint32_t>(tab[(w >> 8) & 0xffu]) << 8 |
           static_cast<uint32_t>(tab[(w >> 16) & 0xffu]) << 16 | static_cast<uint32_t>(tab[w >> 24]) << 24;
}

// workgroup w serves the packets [w kBlock P, (w + 1) kBlock P): lane t takes w kBlock P + j kBlock + t, j < P
template <int P>
__global__ __launch_bounds__(kBlock) void eltwise_w8_lut_packets_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ table,
                                                                         uint8_t* __restrict__ y, int64_t packets, int tail) {
    __shared__ alignas(256) uint8_t tab[256 * kEltLutCopies];
    const int tid = static_cast<int>(threadIdx.x);
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (kBlock * P) + tid;
    const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(x);
    const uint8_t e = table[tid];                                   // issued first: it is waited for first
    u32x4 v[P];
#pragma unroll
    for (int j = 0; j < P; ++j) v[j] = src[elt_min(first + j * kBlock, packets - 1)];         // clamped: always a packet of x
#pragma unroll
    for (int c = 0; c < kEltLutCopies; ++c) tab[c * 256 + tid] = e;
    __syncthreads();
    // the P packets are wanted as loaded, all in flight at once: without this the compiler sinks a load into the branch of its
    // store below and waits for it there, one latency after the other
#pragma unroll
    for (int j = 0; j < P; ++j) asm volatile("" : "+v"(v[j]));
    const uint8_t* mine = tab + ((tid >> 5) & (kEltLutCopies - 1)) * 256;
    u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(y);
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int64_t q = first + j * kBlock;
        const u32x4 r = u32x4{elt_lookup4(mine, v[j][0]), elt_lookup4(mine, v[j][1]), elt_lookup4(mine, v[j][2]),
                                      elt_lookup4(mine, v[j][3])};
        if (q < packets) dst[q] = r;
    }
    if (blockIdx.x == 0 && tid < tail) y[packets * 16 + tid] = mine[x[packets * 16 + tid]];
}

// one lane per byte, the table read from global memory (256 bytes: it stays in the cache)
__global__ __launch_bounds__(kBlock) void eltwise_w8_lut_generic_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ table,
                                                                         uint8_t* __restrict__ y, int64_t n) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n) y[i] = table[x[i]];
}

// ------------------------------------------------------------------------------------------------
// the gate multiply
// ------------------------------------------------------------------------------------------------
struct EltMulArg {          // kernel argument: the constants
    const float* s_x;
    const int32_t* zx;
    const float* s_g;
    const int32_t* zg;
    const float* scale;     // the output quantizer; NULL: a floating y
    const float* shift;
    float qmin, qmax, tmin, tmax;
    int mid;                // LSQ_F32 / LSQ_BF16 / LSQ_F16
    uint32_t flip_x, flip_g;    // 0x80808080 for int8 levels (biased by 128 on load), 0 for uint8
};

struct EltMulGeom {         // kernel argument; the host has checked that every product fits 63 bits
    int64_t image;          // H W C, the bytes of one image of x
    int64_t image_packets;  // H W C / 16
    int64_t lanes;          // lanes per image (packets kernel)
    int C, P;               // channels, 16-channel packets
    int small;              // every item index of the launch fits 32 bits
};

struct EltMulQ : W8OutSide {        // the constants, read once per thread
    float s_x, zx, s_g, zg;
    float off_x, off_g;     // 128.0f for int8 levels, what the flipped byte carries too much; 0.0f for uint8
};

__device__ __forceinline__ EltMulQ elt_mul_constants(const EltMulArg& a) {
    EltMulQ q;
    w8o_constants(q, a);
    q.s_x = a.s_x[0];
    q.zx = static_cast<float>(a.zx[0]);
    q.s_g = a.s_g[0];
    q.zg = static_cast<float>(a.zg[0]);
    q.off_x = a.flip_x ? 128.0f : 0.0f;
    q.off_g = a.flip_g ? 128.0f : 0.0f;
    return q;
}

// LevelsTensor.dequantize(mid) of byte `i` of a packet's word `w`, which was flipped by 0x80 per byte for int8 levels so that
// it holds level + off (off = 128.0f, else 0.0f) as an unsigned byte: float(level) = float(byte) - off exactly, then
// (float(level) - float(zero)) * scale, rounded to mid
template <int I>
__device__ __forceinline__ float elt_dequant(uint32_t w, float off, float zero, float scale, int mid) {
    const float l = __fsub_rn(static_cast<float>((w >> (8 * I)) & 0xffu), off);
    return w8o_round_mid(__fmul_rn(__fsub_rn(l, zero), scale), mid);
}

// the four bytes of a word
__device__ __forceinline__ void elt_dequant4(float* out, uint32_t w, float off, float zero, float scale, int mid) {
    out[0] = elt_dequant<0>(w, off, zero, scale, mid);
    out[1] = elt_dequant<1>(w, off, zero, scale, mid);
    out[2] = elt_dequant<2>(w, off, zero, scale, mid);
    out[3] = elt_dequant<3>(w, off, zero, scale, mid);
}

// t of the contract: one rounded fp32 multiply (never an fma), one rounding to mid
__device__ __forceinline__ float elt_product(float a, float g, int mid) { return w8o_round_mid(__fmul_rn(a, g), mid); }

// (b, l) of item = b L + l; `small`: the items fit 32 bits, where the division is a handful of instructions without a branch
__device__ __forceinline__ void elt_split(int64_t item, int64_t L, int small, int64_t& b, int64_t& l) {
    if (small) {
        const uint32_t it = static_cast<uint32_t>(item), q = it / static_cast<uint32_t>(L);
        b = q;
        l = it - q * static_cast<uint32_t>(L);
    } else {
        b = item / L;
        l = item - b * L;
    }
}

// item = b L + l: lane l of image b takes the image's packets l + k L, k < PIX (L = g.lanes, a multiple of g.P)
template <int PIX>
__global__ __launch_bounds__(kBlock) void eltwise_w8_mul_packets_kernel(EltMulGeom g, EltMulArg a, const uint8_t* __restrict__ x,
                                                                         const uint8_t* __restrict__ gate, void* __restrict__ y, int64_t items) {
    const int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (item >= items) return;
    int64_t b, l;
    elt_split(item, g.lanes, g.small, b, l);
    // L is a multiple of P: the lane's packet position along C is l mod P at every step
    const int cp = g.small ? static_cast<int>(static_cast<uint32_t>(l) % static_cast<uint32_t>(g.P)) : static_cast<int>(l % g.P);
    const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(x + b * g.image);
    u32x4 gv = *reinterpret_cast<const u32x4*>(gate + (b * g.P + cp) * 16);
    u32x4 v[PIX];
#pragma unroll
    for (int k = 0; k < PIX; ++k) v[k] = src[elt_min(l + k * g.lanes, g.image_packets - 1)];      // clamped: always a packet of the image
    const EltMulQ q = elt_mul_constants(a);
    // the packets are wanted as loaded, all in flight at once (the compiler would sink each into the branch of its store)
    asm volatile("" : "+v"(gv));
#pragma unroll
    for (int k = 0; k < PIX; ++k) asm volatile("" : "+v"(v[k]));
    float gf[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) elt_dequant4(gf + 4 * i, gv[i] ^ a.flip_g, q.off_g, q.zg, q.s_g, q.mid);
#pragma unroll
    for (int k = 0; k < PIX; ++k) {
        const int64_t p = l + k * g.lanes;
        float t[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) elt_dequant4(t + 4 * i, v[k][i] ^ a.flip_x, q.off_x, q.zx, q.s_x, q.mid);
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = elt_product(t[i], gf[i], q.mid);
        if (p < g.image_packets) w8o_store16(y, (b * g.image_packets + p) * 16, t, q);
    }
}

// one lane per element
__global__ __launch_bounds__(kBlock) void eltwise_w8_mul_generic_kernel(EltMulGeom g, EltMulArg a, const uint8_t* __restrict__ x,
                                                                         const uint8_t* __restrict__ gate, void* __restrict__ y, int64_t items) {
    const int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (item >= items) return;
    const EltMulQ q = elt_mul_constants(a);
    int64_t b, r;
    elt_split(item, g.image, g.small, b, r);
    const int c = g.small ? static_cast<int>(static_cast<uint32_t>(r) % static_cast<uint32_t>(g.C)) : static_cast<int>(r % g.C);
    const float av = elt_dequant<0>(static_cast<uint32_t>(x[item]) ^ (a.flip_x & 0xffu), q.off_x, q.zx, q.s_x, q.mid);
    const float gv = elt_dequant<0>(static_cast<uint32_t>(gate[b * g.C + c]) ^ (a.flip_g & 0xffu), q.off_g, q.zg, q.s_g, q.mid);
    w8o_store1(y, item, elt_product(av, gv, q.mid), q);
}

// ------------------------------------------------------------------------------------------------
// host side: the plans
// ------------------------------------------------------------------------------------------------
struct EltPlan {
    int family, block, per, lds;
    int64_t grid, aux0, aux1;       // lut: packets, tail bytes; mul: lanes per image, 0
};

inline EltPlan plan_lut(int64_t n, bool aligned) {
    EltPlan pl = {};
    pl.block = kBlock;
    pl.per = 1;
    if (!(aligned && n >= 16)) {
        pl.family = LSQ_ELTWISE_W8_GENERIC;
        pl.grid = ceil_div(n, kBlock);
        return pl;
    }
    const int64_t packets = n / 16, fill = static_cast<int64_t>(device_info().cu_count) * kEltBlocksPerCU;
    int per = kEltLutMaxP;
    while (per > 1 && ceil_div(packets, static_cast<int64_t>(kBlock) * per) < fill) per /= 2;
    pl.family = LSQ_ELTWISE_W8_PACKETS;
    pl.per = per;
    pl.lds = 256 * kEltLutCopies;
    pl.grid = ceil_div(packets, static_cast<int64_t>(kBlock) * per);
    pl.aux0 = packets;
    pl.aux1 = n % 16;
    return pl;
}

struct EltMulShape {        // a checked shape
    int64_t pixels, elems, g_bytes;
    EltMulGeom g;
};

inline EltPlan plan_mul(EltMulShape& s, bool aligned) {
    EltPlan pl = {};
    pl.block = kBlock;
    pl.per = 1;
    if (!(aligned && s.g.C % 16 == 0)) {
        pl.family = LSQ_ELTWISE_W8_GENERIC;
        pl.grid = ceil_div(s.elems, kBlock);
        return pl;
    }
    const int64_t B = s.elems / s.g.image, fill = static_cast<int64_t>(device_info().cu_count) * kEltBlocksPerCU;
    int pix = kEltMulMaxPix;
    while (pix > 1 && pix > s.pixels) pix /= 2;
    while (pix > 1 && ceil_div(B * s.g.P * ceil_div(s.pixels, pix), kBlock) < fill) pix /= 2;
    pl.family = LSQ_ELTWISE_W8_PACKETS;
    pl.per = pix;
    s.g.lanes = s.g.P * ceil_div(s.pixels, pix);
    pl.aux0 = s.g.lanes;
    pl.grid = ceil_div(B * s.g.lanes, kBlock);
    return pl;
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_eltwise_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

int check_grid(const char* what, const lsq::EltPlan& pl) {
    if (pl.grid > INT32_MAX) return fail(LSQ_EINVAL, "%s: %lld workgroups are beyond a 31-bit grid", what, static_cast<ll>(pl.grid));
    return LSQ_OK;
}

int check_n(const char* what, int64_t n) {
    if (n < 1) return fail(LSQ_EINVAL, "%s: n = %lld, at least 1 byte is needed", what, static_cast<ll>(n));
    return LSQ_OK;
}

int check_shape(const char* what, const lsq_eltwise_w8_shape* sh, lsq::EltMulShape& s) {
    if (!sh) return fail(LSQ_EINVAL, "%s: NULL shape", what);
    if (sh->B < 1 || sh->C < 1 || sh->H < 1 || sh->W < 1)
        return fail(LSQ_EINVAL, "%s: x is [B, H, W, C] = [%lld, %lld, %lld, %lld], every extent must be at least 1", what,
                    static_cast<ll>(sh->B), static_cast<ll>(sh->H), static_cast<ll>(sh->W), static_cast<ll>(sh->C));
    const int64_t lim = INT32_MAX / 4;
    if (sh->B > lim || sh->C > lim || sh->H > lim || sh->W > lim) return fail(LSQ_EINVAL, "%s: an extent is beyond 29 bits", what);
    const int64_t pix = sh->H * sh->W;
    if (sh->C > INT64_MAX / 64 / pix || sh->B > INT64_MAX / 64 / (pix * sh->C))
        return fail(LSQ_EINVAL, "%s: the shapes are beyond 64-bit offsets", what);
    s.pixels = pix;
    s.elems = sh->B * pix * sh->C;
    s.g_bytes = sh->B * sh->C;
    s.g = lsq::EltMulGeom{pix * sh->C, pix * sh->C / 16, 0, static_cast<int>(sh->C), static_cast<int>(sh->C / 16),
                          s.elems <= static_cast<int64_t>(UINT32_MAX) ? 1 : 0};
    return LSQ_OK;
}

int check_level_dtype(const char* what, const char* name, int code) {
    if (code != LSQ_ELTWISE_W8_U8 && code != LSQ_ELTWISE_W8_I8)
        return fail(LSQ_EINVAL, "%s: %s must be LSQ_ELTWISE_W8_U8 (0) or LSQ_ELTWISE_W8_I8 (1), got %d", what, name, code);
    return LSQ_OK;
}

// the constants, into `arg` (the caller's, zeroed); the bytes of one element of y into `y_elem`
int check_mul(const char* what, const lsq_eltwise_w8_mul* m, int x_dtype, int g_dtype, lsq::EltMulArg& arg, int64_t& y_elem) {
    if (!m) return fail(LSQ_EINVAL, "%s: NULL constants", what);
    if (!m->s_x || !m->zx || !m->s_g || !m->zg) return fail(LSQ_EINVAL, "%s: NULL s_x, zx, s_g or zg", what);
    if (!aligned_to(m->s_x, 4) || !aligned_to(m->zx, 4) || !aligned_to(m->s_g, 4) || !aligned_to(m->zg, 4))
        return fail(LSQ_EINVAL, "%s: s_x, zx, s_g and zg must be element-aligned", what);
    if (int rc = check_out_side(what, *m, arg, y_elem)) return rc;
    arg.s_x = static_cast<const float*>(m->s_x);
    arg.zx = static_cast<const int32_t*>(m->zx);
    arg.s_g = static_cast<const float*>(m->s_g);
    arg.zg = static_cast<const int32_t*>(m->zg);
    arg.flip_x = x_dtype == LSQ_ELTWISE_W8_I8 ? 0x80808080u : 0u;
    arg.flip_g = g_dtype == LSQ_ELTWISE_W8_I8 ? 0x80808080u : 0u;
    return LSQ_OK;
}

void write_plan(const lsq::EltPlan& pl, int32_t* out8) {
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.block;
    out8[3] = pl.per;
    out8[4] = pl.lds;
    out8[5] = static_cast<int32_t>(std::min<int64_t>(pl.aux0, INT32_MAX));
    out8[6] = static_cast<int32_t>(pl.aux1);
    out8[7] = 0;
}

}  // namespace

extern "C" {

int lsq_eltwise_w8_abi_version(void) { return LSQ_ELTWISE_W8_ABI_VERSION; }

const char* lsq_eltwise_w8_last_error(void) { return g_last_error; }

int lsq_eltwise_w8_lut(const void* x, const void* table, int64_t n, void* y, void* stream) {
    const char* what = "lsq_eltwise_w8_lut";
    if (!x || !table || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (int rc = check_n(what, n)) return rc;
    if (overlap(y, n, x, n)) return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap x's: the table op in place is not served", what, static_cast<ll>(n));
    if (overlap(y, n, table, 256)) return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap the table's 256", what, static_cast<ll>(n));
    const lsq::EltPlan pl = lsq::plan_lut(n, aligned_to(x, 16) && aligned_to(y, 16));
    if (int rc = check_grid(what, pl)) return rc;
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kBlock);
    const uint8_t* xb = static_cast<const uint8_t*>(x);
    const uint8_t* tb = static_cast<const uint8_t*>(table);
    uint8_t* yb = static_cast<uint8_t*>(y);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pl.family == LSQ_ELTWISE_W8_PACKETS) {
        const int tail = static_cast<int>(pl.aux1);
        if (pl.per == 4) {
            if constexpr (lsq::kEltLutMaxP >= 4) hipLaunchKernelGGL(lsq::eltwise_w8_lut_packets_kernel<4>, grid, block, 0, st, xb, tb, yb, pl.aux0, tail);
        } else if (pl.per == 2) {
            if constexpr (lsq::kEltLutMaxP >= 2) hipLaunchKernelGGL(lsq::eltwise_w8_lut_packets_kernel<2>, grid, block, 0, st, xb, tb, yb, pl.aux0, tail);
        } else {
            hipLaunchKernelGGL(lsq::eltwise_w8_lut_packets_kernel<1>, grid, block, 0, st, xb, tb, yb, pl.aux0, tail);
        }
    } else {
        hipLaunchKernelGGL(lsq::eltwise_w8_lut_generic_kernel, grid, block, 0, st, xb, tb, yb, n);
    }
    return hip_status(hipGetLastError(), what);
}

int lsq_eltwise_w8_mul_gate(int x_dtype, const void* x_levels, int g_dtype, const void* g_levels, const lsq_eltwise_w8_shape* shape,
                            const lsq_eltwise_w8_mul* mul, void* y, void* stream) {
    const char* what = "lsq_eltwise_w8_mul_gate";
    lsq::EltMulShape s;
    lsq::EltMulArg arg{};
    int64_t y_elem = 1;
    if (int rc = check_level_dtype(what, "x_dtype", x_dtype)) return rc;
    if (int rc = check_level_dtype(what, "g_dtype", g_dtype)) return rc;
    if (int rc = check_shape(what, shape, s)) return rc;
    if (int rc = check_mul(what, mul, x_dtype, g_dtype, arg, y_elem)) return rc;
    if (!x_levels || !g_levels || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (overlap(y, s.elems * y_elem, x_levels, s.elems))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap x's %lld: the multiply in place is not served", what,
                    static_cast<ll>(s.elems * y_elem), static_cast<ll>(s.elems));
    if (overlap(y, s.elems * y_elem, g_levels, s.g_bytes))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap the gate's %lld", what, static_cast<ll>(s.elems * y_elem), static_cast<ll>(s.g_bytes));
    if (!aligned_to(y, static_cast<uintptr_t>(y_elem))) return fail(LSQ_EINVAL, "%s: a floating y must be element-aligned", what);
    const lsq::EltPlan pl = lsq::plan_mul(s, aligned_to(x_levels, 16) && aligned_to(g_levels, 16) && aligned_to(y, 16));
    if (int rc = check_grid(what, pl)) return rc;
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kBlock);
    const uint8_t* x = static_cast<const uint8_t*>(x_levels);
    const uint8_t* g = static_cast<const uint8_t*>(g_levels);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pl.family == LSQ_ELTWISE_W8_PACKETS) {
        const int64_t items = s.elems / s.g.image * s.g.lanes;
        if (pl.per == 4) hipLaunchKernelGGL(lsq::eltwise_w8_mul_packets_kernel<4>, grid, block, 0, st, s.g, arg, x, g, y, items);
        else if (pl.per == 2) hipLaunchKernelGGL(lsq::eltwise_w8_mul_packets_kernel<2>, grid, block, 0, st, s.g, arg, x, g, y, items);
        else hipLaunchKernelGGL(lsq::eltwise_w8_mul_packets_kernel<1>, grid, block, 0, st, s.g, arg, x, g, y, items);
    } else {
        hipLaunchKernelGGL(lsq::eltwise_w8_mul_generic_kernel, grid, block, 0, st, s.g, arg, x, g, y, s.elems);
    }
    return hip_status(hipGetLastError(), what);
}

int lsq_eltwise_w8_plan_lut(int64_t n, int aligned, int32_t* out8) {
    const char* what = "lsq_eltwise_w8_plan_lut";
    if (int rc = check_n(what, n)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::EltPlan pl = lsq::plan_lut(n, aligned != 0);
    if (int rc = check_grid(what, pl)) return rc;
    write_plan(pl, out8);
    return LSQ_OK;
}

int lsq_eltwise_w8_plan_mul(const lsq_eltwise_w8_shape* shape, int aligned, int32_t* out8) {
    const char* what = "lsq_eltwise_w8_plan_mul";
    lsq::EltMulShape s;
    if (int rc = check_shape(what, shape, s)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::EltPlan pl = lsq::plan_mul(s, aligned != 0);
    if (int rc = check_grid(what, pl)) return rc;
    write_plan(pl, out8);
    return LSQ_OK;
}

}  // extern "C"
