// lsq_glu_w8.hip -- the gated product act(gate) * up on 8-bit levels on gfx950 (include/lsq_hip_glu_w8.h, which states the
// contract): the kernels and the C ABI of liblsq_hip_glu_w8.so.  A bandwidth kernel on 16-byte packets: 2 bytes read and 1
// written per element.
//
//  * PACKETS (C % 16 == 0; gate, up and y 16-byte aligned; both row strides % 16 == 0): the 256-entry float table is staged once
//    per workgroup into LDS, one entry per thread (1 KB), rounded to mid_dtype on the way (the identity for a table that holds
//    values of mid_dtype; the CPU path's `table.to(mid_dtype)` for any other).  A lane owns P packet positions, kBlock packets
//    apart (a wave's accesses stay contiguous within a row); packet q of the dense y is (row, c0) = (q / (C / 16), q % (C / 16) * 16), and the lane reads
//    the packet of gate and the packet of up at row * their row stride + c0.  All 2 P loads are issued up front from clamped
//    positions; each gate byte is looked up with a 4-byte read of LDS, each up byte is dequantized as in the gate multiply of
//    eltwise_w8, and the 16 outputs leave as one packet (levels) or as 2 / 4 packets (floats).  The epilogue is selects on
//    mid_dtype, not branches; only the store branches on the kind of y.
//  * GENERIC (every other legal call): one lane per element, the table read from global memory (1 KB: it stays in the cache).
//    Correct, not tuned.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../lsq_w8_out_side.hpp"
#include "../lsq_w8_out_side_host.hpp"
#include "../../../include/lsq_hip_glu_w8.h"

namespace lsq {

constexpr int kGluMaxP = 2;                     // packet positions per lane: the table op's rule
constexpr int kGluBlocksPerCU = 2;              // the grid "fills the chip" from here
static_assert(kBlock == 256, "the table is staged one entry per thread");

struct GluArg {             // kernel argument: the constants
    const float* s_u;
    const int32_t* z_u;
    const float* scale;     // the output quantizer; NULL: a floating y
    const float* shift;
    float qmin, qmax, tmin, tmax;
    int mid;                // LSQ_F32 / LSQ_BF16 / LSQ_F16
    uint32_t flip_u;        // 0x80808080 for int8 levels of up (biased by 128 on load), 0 for uint8
};

struct GluGeom {            // kernel argument; the host has checked that every product fits 63 bits
    int64_t gs, us;         // the row strides of gate and up, bytes
    int C, P;               // columns, 16-column packets of a row
    int small;              // every item index of the launch fits 32 bits
};

struct GluQ : W8OutSide {   // the constants, read once per thread
    float s_u, z_u, off_u;  // off_u: 128.0f for int8 levels, what the flipped byte carries too much; 0.0f for uint8
};

__device__ __forceinline__ GluQ glu_constants(const GluArg& a) {
    GluQ q;
    w8o_constants(q, a);
    q.s_u = a.s_u[0];
    q.z_u = static_cast<float>(a.z_u[0]);
    q.off_u = a.flip_u ? 128.0f : 0.0f;
    return q;
}

__device__ __forceinline__ int64_t glu_min(int64_t a, int64_t b) { return a < b ? a : b; }

// (row, col) of item = row per + col; `small`: the items fit 32 bits, where the division is a handful of instructions
__device__ __forceinline__ void glu_split(int64_t item, int per, int small, int64_t& row, int64_t& col) {
    if (small) {
        const uint32_t it = static_cast<uint32_t>(item), q = it / static_cast<uint32_t>(per);
        row = q;
        col = it - q * static_cast<uint32_t>(per);
    } else {
        row = item / per;
        col = item - row * per;
    }
}

// LevelsTensor.dequantize(mid) of byte `I` of a packet's word `w` of up, which was flipped by 0x80 per byte for int8 levels so
// that it holds level + off as an unsigned byte: float(level) = float(byte) - off exactly, then (float(level) - float(zero)) *
// scale, rounded to mid
template <int I>
__device__ __forceinline__ float glu_dequant(uint32_t w, const GluQ& q) {
    const float l = __fsub_rn(static_cast<float>((w >> (8 * I)) & 0xffu), q.off_u);
    return w8o_round_mid(__fmul_rn(__fsub_rn(l, q.z_u), q.s_u), q.mid);
}

// t of the contract: one rounded fp32 multiply (never an fma), one rounding to mid
__device__ __forceinline__ float glu_product(float a, float d, int mid) { return w8o_round_mid(__fmul_rn(a, d), mid); }

// the four elements of one word of gate (as stored) and of up (flipped)
__device__ __forceinline__ void glu_word(float* t, const float* tab, uint32_t gw, uint32_t uw, const GluQ& q) {
    t[0] = glu_product(tab[gw & 0xffu], glu_dequant<0>(uw, q), q.mid);
    t[1] = glu_product(tab[(gw >> 8) & 0xffu], glu_dequant<1>(uw, q), q.mid);
    t[2] = glu_product(tab[(gw >> 16) & 0xffu], glu_dequant<2>(uw, q), q.mid);
    t[3] = glu_product(tab[gw >> 24], glu_dequant<3>(uw, q), q.mid);
}

// workgroup w serves the packets [w kBlock P, (w + 1) kBlock P) of y: lane t takes w kBlock P + j kBlock + t, j < P
template <int P>
__global__ __launch_bounds__(kBlock) void glu_w8_packets_kernel(GluGeom g, GluArg a, const uint8_t* __restrict__ gate,
                                                                 const uint8_t* __restrict__ up, const float* __restrict__ table,
                                                                 void* __restrict__ y, int64_t packets) {
    __shared__ alignas(256) float tab[256];
    const int tid = static_cast<int>(threadIdx.x);
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (kBlock * P) + tid;
    const float e = table[tid];                                     // issued first: it is waited for first
    u32x4 gv[P], uv[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        int64_t row, cp;
        glu_split(glu_min(first + j * kBlock, packets - 1), g.P, g.small, row, cp);      // clamped: always a packet of the operands
        gv[j] = *reinterpret_cast<const u32x4*>(gate + row * g.gs + cp * 16);
        uv[j] = *reinterpret_cast<const u32x4*>(up + row * g.us + cp * 16);
    }
    const GluQ q = glu_constants(a);
    tab[tid] = w8o_round_mid(e, q.mid);         // a value of mid already (the contract): the identity, once per entry and not per element
    __syncthreads();
    // the 2 P packets are wanted as loaded, all in flight at once: without this the compiler sinks a load into the branch of its
    // store below and waits for it there, one latency after the other
#pragma unroll
    for (int j = 0; j < P; ++j) {
        asm volatile("" : "+v"(gv[j]));
        asm volatile("" : "+v"(uv[j]));
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int64_t p = first + j * kBlock;
        float t[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) glu_word(t + 4 * i, tab, gv[j][i], uv[j][i] ^ a.flip_u, q);
        if (p < packets) w8o_store16(y, p * 16, t, q);
    }
}

// one lane per element
__global__ __launch_bounds__(kBlock) void glu_w8_generic_kernel(GluGeom g, GluArg a, const uint8_t* __restrict__ gate,
                                                                 const uint8_t* __restrict__ up, const float* __restrict__ table,
                                                                 void* __restrict__ y, int64_t items) {
    const int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (item >= items) return;
    const GluQ q = glu_constants(a);
    int64_t row, c;
    glu_split(item, g.C, g.small, row, c);
    const float av = w8o_round_mid(table[gate[row * g.gs + c]], q.mid);
    const float d = glu_dequant<0>(static_cast<uint32_t>(up[row * g.us + c]) ^ (a.flip_u & 0xffu), q);
    w8o_store1(y, item, glu_product(av, d, q.mid), q);
}

// ------------------------------------------------------------------------------------------------
// host side: the plan
// ------------------------------------------------------------------------------------------------
struct GluPlan {
    int family, block, per, lds;
    int64_t grid, packets;
};

struct GluShape {           // a checked shape
    int64_t rows, elems, gate_span, up_span;    // the spans in bytes: (rows - 1) * row stride + C
    GluGeom g;
};

inline GluPlan plan_glu(const GluShape& s, bool aligned) {
    GluPlan pl = {};
    pl.block = kBlock;
    pl.per = 1;
    if (!(aligned && s.g.C % 16 == 0 && s.g.gs % 16 == 0 && s.g.us % 16 == 0)) {
        pl.family = LSQ_GLU_W8_GENERIC;
        pl.grid = ceil_div(s.elems, kBlock);
        return pl;
    }
    const int64_t packets = s.elems / 16, fill = static_cast<int64_t>(device_info().cu_count) * kGluBlocksPerCU;
    int per = kGluMaxP;
    while (per > 1 && ceil_div(packets, static_cast<int64_t>(kBlock) * per) < fill) per /= 2;
    pl.family = LSQ_GLU_W8_PACKETS;
    pl.per = per;
    pl.lds = 256 * static_cast<int>(sizeof(float));
    pl.grid = ceil_div(packets, static_cast<int64_t>(kBlock) * per);
    pl.packets = packets;
    return pl;
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_glu_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

int check_grid(const char* what, const lsq::GluPlan& pl) {
    if (pl.grid > INT32_MAX) return fail(LSQ_EINVAL, "%s: %lld workgroups are beyond a 31-bit grid", what, static_cast<ll>(pl.grid));
    return LSQ_OK;
}

int check_shape(const char* what, const lsq_glu_w8_shape* sh, lsq::GluShape& s) {
    if (!sh) return fail(LSQ_EINVAL, "%s: NULL shape", what);
    if (sh->rows < 1 || sh->C < 1)
        return fail(LSQ_EINVAL, "%s: gate, up and y are [rows, C] = [%lld, %lld], every extent must be at least 1", what,
                    static_cast<ll>(sh->rows), static_cast<ll>(sh->C));
    if (sh->gate_row_stride < sh->C || sh->up_row_stride < sh->C)
        return fail(LSQ_EINVAL, "%s: the row strides of gate and up, %lld and %lld, must be at least C = %lld", what,
                    static_cast<ll>(sh->gate_row_stride), static_cast<ll>(sh->up_row_stride), static_cast<ll>(sh->C));
    // C <= a row stride, so rows * C * (4 bytes of a float y) stays below the bound too
    const int64_t lim = INT64_MAX / 64;
    if (sh->C > INT32_MAX || sh->gate_row_stride > lim / sh->rows || sh->up_row_stride > lim / sh->rows)
        return fail(LSQ_EINVAL, "%s: the shapes are beyond 64-bit offsets", what);
    s.rows = sh->rows;
    s.elems = sh->rows * sh->C;
    s.gate_span = (sh->rows - 1) * sh->gate_row_stride + sh->C;
    s.up_span = (sh->rows - 1) * sh->up_row_stride + sh->C;
    s.g = lsq::GluGeom{sh->gate_row_stride, sh->up_row_stride, static_cast<int>(sh->C), static_cast<int>(sh->C / 16),
                       s.elems <= static_cast<int64_t>(UINT32_MAX) ? 1 : 0};
    return LSQ_OK;
}

int check_level_dtype(const char* what, const char* name, int code) {
    if (code != LSQ_GLU_W8_U8 && code != LSQ_GLU_W8_I8)
        return fail(LSQ_EINVAL, "%s: %s must be LSQ_GLU_W8_U8 (0) or LSQ_GLU_W8_I8 (1), got %d", what, name, code);
    return LSQ_OK;
}

// the constants, into `arg` (the caller's, zeroed); the bytes of one element of y into `y_elem`
int check_consts(const char* what, const lsq_glu_w8_consts* c, int up_dtype, lsq::GluArg& arg, int64_t& y_elem) {
    if (!c) return fail(LSQ_EINVAL, "%s: NULL constants", what);
    if (!c->s_u || !c->z_u) return fail(LSQ_EINVAL, "%s: NULL s_u or z_u", what);
    if (!aligned_to(c->s_u, 4) || !aligned_to(c->z_u, 4)) return fail(LSQ_EINVAL, "%s: s_u and z_u must be element-aligned", what);
    if (int rc = check_out_side(what, *c, arg, y_elem)) return rc;
    arg.s_u = static_cast<const float*>(c->s_u);
    arg.z_u = static_cast<const int32_t*>(c->z_u);
    arg.flip_u = up_dtype == LSQ_GLU_W8_I8 ? 0x80808080u : 0u;
    return LSQ_OK;
}

void write_plan(const lsq::GluPlan& pl, int32_t* out8) {
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.block;
    out8[3] = pl.per;
    out8[4] = pl.lds;
    out8[5] = static_cast<int32_t>(std::min<int64_t>(pl.packets, INT32_MAX));
    out8[6] = 0;
    out8[7] = 0;
}

}  // namespace

extern "C" {

int lsq_glu_w8_abi_version(void) { return LSQ_GLU_W8_ABI_VERSION; }

const char* lsq_glu_w8_last_error(void) { return g_last_error; }

int lsq_glu_w8(int gate_dtype, const void* gate_levels, int up_dtype, const void* up_levels, const void* table,
               const lsq_glu_w8_shape* shape, const lsq_glu_w8_consts* consts, void* y, void* stream) {
    const char* what = "lsq_glu_w8";
    lsq::GluShape s;
    lsq::GluArg arg{};
    int64_t y_elem = 1;
    if (int rc = check_level_dtype(what, "gate_dtype", gate_dtype)) return rc;
    if (int rc = check_level_dtype(what, "up_dtype", up_dtype)) return rc;
    if (int rc = check_shape(what, shape, s)) return rc;
    if (int rc = check_consts(what, consts, up_dtype, arg, y_elem)) return rc;
    if (!gate_levels || !up_levels || !table || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(table, 4)) return fail(LSQ_EINVAL, "%s: the table's 256 float32 values must be 4-byte aligned", what);
    const int64_t y_bytes = s.elems * y_elem;
    if (overlap(y, y_bytes, gate_levels, s.gate_span))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap the gate's span of %lld: the product in place is not served", what,
                    static_cast<ll>(y_bytes), static_cast<ll>(s.gate_span));
    if (overlap(y, y_bytes, up_levels, s.up_span))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap up's span of %lld: the product in place is not served", what,
                    static_cast<ll>(y_bytes), static_cast<ll>(s.up_span));
    if (overlap(y, y_bytes, table, 1024)) return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap the table's 1024", what, static_cast<ll>(y_bytes));
    if (!aligned_to(y, static_cast<uintptr_t>(y_elem))) return fail(LSQ_EINVAL, "%s: a floating y must be element-aligned", what);
    const lsq::GluPlan pl = lsq::plan_glu(s, aligned_to(gate_levels, 16) && aligned_to(up_levels, 16) && aligned_to(y, 16));
    if (int rc = check_grid(what, pl)) return rc;
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kBlock);
    const uint8_t* g = static_cast<const uint8_t*>(gate_levels);
    const uint8_t* u = static_cast<const uint8_t*>(up_levels);
    const float* t = static_cast<const float*>(table);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pl.family == LSQ_GLU_W8_PACKETS) {
        if (pl.per == 2) hipLaunchKernelGGL(lsq::glu_w8_packets_kernel<2>, grid, block, 0, st, s.g, arg, g, u, t, y, pl.packets);
        else hipLaunchKernelGGL(lsq::glu_w8_packets_kernel<1>, grid, block, 0, st, s.g, arg, g, u, t, y, pl.packets);
    } else {
        hipLaunchKernelGGL(lsq::glu_w8_generic_kernel, grid, block, 0, st, s.g, arg, g, u, t, y, s.elems);
    }
    return hip_status(hipGetLastError(), what);
}

int lsq_glu_w8_plan(const lsq_glu_w8_shape* shape, int aligned, int32_t* out8) {
    const char* what = "lsq_glu_w8_plan";
    lsq::GluShape s;
    if (int rc = check_shape(what, shape, s)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::GluPlan pl = lsq::plan_glu(s, aligned != 0);
    if (int rc = check_grid(what, pl)) return rc;
    write_plan(pl, out8);
    return LSQ_OK;
}

}  // extern "C"
