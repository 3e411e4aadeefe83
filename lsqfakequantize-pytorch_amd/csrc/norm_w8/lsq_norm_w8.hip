// lsq_norm_w8.hip -- LayerNorm and RMSNorm on 8-bit levels on gfx950 (include/lsq_hip_norm_w8.h, which states the contract): the
// kernels and the C ABI of liblsq_hip_norm_w8.so.
//
//  * PACKETS (C % 16 == 0, C <= 8192, x and y 16-byte aligned): a row lives in the registers of a group of L lanes (a power of
//    two, 4 .. 64: never wider than a wave), P 16-byte packets per lane, lane l holding the row's packets l, l + L, ...: x is read
//    from memory exactly once.  All P loads of a row are issued before the first use.  The sums S1 = sum b and S2 = sum b^2 come
//    from v_dot4_u32_u8 on the words as loaded (with 0x01010101 and with the word itself), int8 levels flipped by 0x80 per byte
//    first: LayerNorm is invariant under that shift, for RMS it is folded into the zero point.  The group's two sums go across
//    its lanes with __shfl_xor: no LDS, no barrier.  A group walks K rows, 256 / L apart, keeping its columns, so its w and bias
//    values are loaded once: into registers for P == 1, else staged once per workgroup into LDS as float32.
//  * GENERIC (every other legal call): one wave per row, two passes over its bytes, w and bias read as they are needed.
//    Correct, not tuned.
// Both end in norm_finish(): the same fp32 steps, each one rounded operation.
// The experiment's variants, NOT shipped (tools/exp_norm_w8_ab.py --build-variants):
//    -DLSQ_NORM_W8_MAX_ROWS=N caps the rows a group walks at N (the library: 8; 1 and 16 were measured and not kept);
//    -DLSQ_NORM_W8_WIDE=1 takes the fewest packets per lane, hence the widest group, whatever lanes that masks (C = 768: 64 lanes
//    of one packet, 16 of them idle, where the library takes 16 lanes of three).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../lsq_w8_out_side.hpp"
#include "../lsq_w8_out_side_host.hpp"
#include "../../../include/lsq_hip_norm_w8.h"

#ifndef LSQ_NORM_W8_MAX_ROWS
#define LSQ_NORM_W8_MAX_ROWS 8          // the library's; 1 / 16 only in the experiment's variant builds
#endif
#ifndef LSQ_NORM_W8_WIDE
#define LSQ_NORM_W8_WIDE 0              // the library's; 1 only in the experiment's variant build
#endif

namespace lsq {

constexpr int kNormMaxP = 8;                    // packets per lane
constexpr int kNormMaxRows = LSQ_NORM_W8_MAX_ROWS;      // rows a group walks
constexpr int kNormRegsP = 1;                   // w and bias in registers up to this P (32 VGPRs a packet), in LDS above
constexpr int kNormBlocksPerCU = 2;             // the grid "fills the chip" from here
constexpr int kNormWave = 64;
constexpr uint32_t kNormOnes = 0x01010101u;
static_assert(kBlock == 256, "four waves per workgroup");

struct NormArg {            // kernel argument: the constants
    const float* s_x;
    const int32_t* zx;
    const void* w;          // NULL: no multiply
    const void* b;          // NULL: no add
    const float* scale;     // the output quantizer; NULL: a floating y
    const float* shift;
    float qmin, qmax, tmin, tmax, eps;
    int pdt;                // LSQ_F32 / LSQ_BF16 / LSQ_F16 of w and b
    int mid;                // LSQ_F32 / LSQ_BF16 / LSQ_F16
    int rms;
    uint32_t flip;          // 0x80808080 for int8 levels (biased by 128 on load), 0 for uint8
};

struct NormGeom {           // kernel argument
    int64_t R;
    int C, packets, K;      // channels, C / 16, rows per group
};

// The output side's four fields are W8OutSide's by name, and lsq_w8_out_side.hpp's helpers read them; they are formed here and
// not by w8o_constants(): the order in which these constants are formed is what the compiler reacts to, and through the shared
// function 40 of the 41 kernels came out with their row-statistics loop reordered.
struct NormQ {              // the constants, read once per thread
    QParams<float> qp;
    Range<float> r;
    float e, fC;
    int z;                  // RMS: the zero point of the byte as loaded (zx + 128 for flipped int8 levels)
    int levels_out, mid, rms, has_w, has_b;
};

__device__ __forceinline__ NormQ norm_constants(const NormArg& a, int C) {
    NormQ q;
    q.r = Range<float>{a.qmin, a.qmax, a.tmin, a.tmax};
    q.levels_out = a.scale != nullptr;
    if (q.levels_out) q.qp = make_qparams<float>(sanitize_scale_per_tensor<float>(a.scale[0]), a.shift[0], q.r);
    else q.qp = QParams<float>{1.0f, 1.0f, 0.0f};
    const float s = a.s_x[0];
    q.e = __fdiv_rn(a.eps, __fmul_rn(s, s));
    q.fC = static_cast<float>(C);
    q.z = a.rms ? a.zx[0] + (a.flip ? 128 : 0) : 0;
    q.mid = a.mid;
    q.rms = a.rms;
    q.has_w = a.w != nullptr;
    q.has_b = a.b != nullptr;
    return q;
}

// element i of w or bias, widened exactly
__device__ __forceinline__ float norm_param(const void* p, int pdt, int i) {
    if (pdt == LSQ_F32) return static_cast<const float*>(p)[i];
    if (pdt == LSQ_BF16) return __uint_as_float(static_cast<uint32_t>(static_cast<const unsigned short*>(p)[i]) << 16);
    return static_cast<float>(static_cast<const _Float16*>(p)[i]);
}

// A row's two per-row numbers from its exact sums (of the bytes as loaded): t_i = float(mul_i) * rc with
//     LayerNorm   mul_i = C b_i - S1 (`sub` = S1, `cmul` = C)       rc = (1 / sqrt(V / C^2 + e)) / C
//     RMS         mul_i = b_i - z    (`sub` = z,  `cmul` = 1)       rc = 1 / sqrt(Q / C + e),  Q = S2 - 2 z S1 + C z^2
struct NormRow {
    float rc;
    int sub, cmul;
};

// The correctly rounded fp32 square root.  NOT __fsqrt_rn: hipcc's header gives that name to the native v_sqrt_f32 (1 ulp), which
// differed from the CPU path in one row of eight.  The builtin is expanded to v_sqrt_f32 plus its fma correction under
// -fhip-fp32-correctly-rounded-divide-sqrt (the Makefile's flag); tests/test_norm_w8_cpu.py looks for that expansion in the ISA.
__device__ __forceinline__ float norm_sqrt_rn(float v) { return __builtin_sqrtf(v); }

__device__ __forceinline__ NormRow norm_row(uint32_t s1, uint32_t s2, int C, const NormQ& q) {
    NormRow o;
    float var;
    if (q.rms) {
        const int64_t z = q.z;
        const int64_t Q = static_cast<int64_t>(s2) - 2 * z * static_cast<int64_t>(s1) + static_cast<int64_t>(C) * z * z;
        var = __fdiv_rn(static_cast<float>(Q), q.fC);
        o.sub = q.z;
        o.cmul = 1;
    } else {
        const uint64_t V = static_cast<uint64_t>(C) * s2 - static_cast<uint64_t>(s1) * s1;
        var = __fdiv_rn(static_cast<float>(V), __fmul_rn(q.fC, q.fC));
        o.sub = static_cast<int>(s1);
        o.cmul = C;
    }
    const float r = __fdiv_rn(1.0f, norm_sqrt_rn(__fadd_rn(var, q.e)));
    o.rc = q.rms ? r : __fdiv_rn(r, q.fC);
    return o;
}

// u of the contract for the byte `b` as loaded: one conversion, one multiply, a multiply, an add, one rounding to mid
__device__ __forceinline__ float norm_finish(uint32_t b, const NormRow& row, float w, float bias, const NormQ& q) {
    const float t = __fmul_rn(static_cast<float>(static_cast<int>(b) * row.cmul - row.sub), row.rc);
    const float tw = q.has_w ? __fmul_rn(t, w) : t;
    const float a = q.has_b ? __fadd_rn(tw, bias) : tw;
    return w8o_round_mid(a, q.mid);
}

// Workgroup b serves the rows [b G K, (b + 1) G K), G = kBlock / L groups: group g takes b G K + g + k G, k < K.  Lane l of a
// group holds the row's packets l + j L, j < P.
template <int L, int P>
__global__ __launch_bounds__(kBlock) void norm_w8_packets_kernel(NormGeom g, NormArg a, const uint8_t* __restrict__ x, void* __restrict__ y) {
    constexpr bool kRegs = P <= kNormRegsP;
    constexpr int G = kBlock / L;
    extern __shared__ float norm_lds[];             // kRegs: none; else w's C floats (if given), then bias's C floats (if given)
    const int tid = static_cast<int>(threadIdx.x), lane = tid & (L - 1), grp = tid / L;
    const NormQ q = norm_constants(a, g.C);
    const float* lw = norm_lds;
    const float* lb = norm_lds + (q.has_w ? g.C : 0);
    float rw[kRegs ? P * 16 : 1], rb[kRegs ? P * 16 : 1];
    if constexpr (kRegs) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int p = min(lane + j * L, g.packets - 1);         // clamped: always inside w and bias
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                rw[j * 16 + i] = q.has_w ? norm_param(a.w, a.pdt, p * 16 + i) : 1.0f;
                rb[j * 16 + i] = q.has_b ? norm_param(a.b, a.pdt, p * 16 + i) : 0.0f;
            }
        }
    } else {
        float* stage = norm_lds;
        if (q.has_w) {
            for (int i = tid; i < g.C; i += kBlock) stage[i] = norm_param(a.w, a.pdt, i);
            stage += g.C;
        }
        if (q.has_b)
            for (int i = tid; i < g.C; i += kBlock) stage[i] = norm_param(a.b, a.pdt, i);
        __syncthreads();
    }
    const int64_t first = static_cast<int64_t>(blockIdx.x) * (G * g.K) + grp;
    for (int k = 0; k < g.K; ++k) {
        // a group past the last row recomputes the last row and stores nothing: every lane of the wave takes part in the
        // exchange below
        const int64_t row = first + static_cast<int64_t>(k) * G;
        const bool live = row < g.R;
        const int64_t base = (live ? row : g.R - 1) * g.packets;
        const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(x) + base;
        u32x4 v[P];
#pragma unroll
        for (int j = 0; j < P; ++j) v[j] = src[min(lane + j * L, g.packets - 1)];       // clamped: always a packet of the row
        // the P packets are wanted as loaded, all in flight at once (the compiler would sink a load to its first use)
#pragma unroll
        for (int j = 0; j < P; ++j) asm volatile("" : "+v"(v[j]));
        uint32_t s1 = 0, s2 = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            uint32_t p1 = 0, p2 = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[j][i] ^= a.flip;
                p1 = __builtin_amdgcn_udot4(v[j][i], kNormOnes, p1, false);
                p2 = __builtin_amdgcn_udot4(v[j][i], v[j][i], p2, false);
            }
            const bool mine = lane + j * L < g.packets;
            s1 += mine ? p1 : 0u;
            s2 += mine ? p2 : 0u;
        }
#pragma unroll
        for (int m = L / 2; m >= 1; m /= 2) {
            s1 += static_cast<uint32_t>(__shfl_xor(static_cast<int>(s1), m));
            s2 += static_cast<uint32_t>(__shfl_xor(static_cast<int>(s2), m));
        }
        const NormRow r = norm_row(s1, s2, g.C, q);
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int p = lane + j * L;
            const int pc = min(p, g.packets - 1);
            float u[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float w, b;
                if constexpr (kRegs) {
                    w = rw[j * 16 + i];
                    b = rb[j * 16 + i];
                } else {
                    w = q.has_w ? lw[pc * 16 + i] : 1.0f;
                    b = q.has_b ? lb[pc * 16 + i] : 0.0f;
                }
                u[i] = norm_finish((v[j][i / 4] >> (8 * (i % 4))) & 0xffu, r, w, b, q);
            }
            if (live && p < g.packets) w8o_store16(y, (base + p) * 16, u, q);
        }
    }
}

// one wave per row: lane l takes the bytes l, l + 64, ... in both passes
__global__ __launch_bounds__(kBlock) void norm_w8_generic_kernel(NormGeom g, NormArg a, const uint8_t* __restrict__ x, void* __restrict__ y) {
    const int lane = static_cast<int>(threadIdx.x) & (kNormWave - 1);
    const int64_t row = static_cast<int64_t>(blockIdx.x) * (kBlock / kNormWave) + static_cast<int>(threadIdx.x) / kNormWave;
    if (row >= g.R) return;                        // a whole wave leaves
    const NormQ q = norm_constants(a, g.C);
    const uint8_t* __restrict__ src = x + row * g.C;
    const uint32_t flip = a.flip & 0xffu;
    uint32_t s1 = 0, s2 = 0;
    for (int i = lane; i < g.C; i += kNormWave) {
        const uint32_t b = static_cast<uint32_t>(src[i]) ^ flip;
        s1 += b;
        s2 += b * b;
    }
#pragma unroll
    for (int m = kNormWave / 2; m >= 1; m /= 2) {
        s1 += static_cast<uint32_t>(__shfl_xor(static_cast<int>(s1), m));
        s2 += static_cast<uint32_t>(__shfl_xor(static_cast<int>(s2), m));
    }
    const NormRow r = norm_row(s1, s2, g.C, q);
    for (int i = lane; i < g.C; i += kNormWave) {
        const float w = q.has_w ? norm_param(a.w, a.pdt, i) : 1.0f;
        const float b = q.has_b ? norm_param(a.b, a.pdt, i) : 0.0f;
        w8o_store1(y, row * g.C + i, norm_finish(static_cast<uint32_t>(src[i]) ^ flip, r, w, b, q), q);
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan
// ------------------------------------------------------------------------------------------------
struct NormPlan {
    int family, block, L, P, rows, params, lds;
    int64_t grid;
    NormGeom g;
};

inline NormPlan plan_norm(int64_t R, int64_t C, bool aligned, bool has_w, bool has_b) {
    NormPlan pl = {};
    pl.block = kBlock;
    pl.g = NormGeom{R, static_cast<int>(C), static_cast<int>(C / 16), 1};
    if (!(aligned && C % 16 == 0 && C <= 16 * kNormWave * kNormMaxP)) {
        pl.family = LSQ_NORM_W8_GENERIC;
        pl.L = kNormWave;
        pl.rows = kBlock / kNormWave;
        pl.grid = ceil_div(R, pl.rows);
        return pl;
    }
    const int packets = static_cast<int>(C / 16);
    int bestL = 0, bestP = 0, best_masked = 1 << 30;
    for (int P = 1; P <= kNormMaxP; ++P) {
        const int lanes = static_cast<int>(ceil_div(packets, P));
        int L = 4;
        while (L < lanes) L *= 2;
        if (L > kNormWave) continue;
        if (L - lanes < best_masked && !(LSQ_NORM_W8_WIDE && bestL)) {
            best_masked = L - lanes;
            bestL = L;
            bestP = P;
        }
    }
    const int G = kBlock / bestL;
    const int64_t fill = static_cast<int64_t>(device_info().cu_count) * kNormBlocksPerCU;
    int K = kNormMaxRows;
    while (K > 1 && ceil_div(R, static_cast<int64_t>(G) * K) < fill) K /= 2;
    pl.family = LSQ_NORM_W8_PACKETS;
    pl.L = bestL;
    pl.P = bestP;
    pl.rows = G * K;
    pl.g.K = K;
    pl.grid = ceil_div(R, pl.rows);
    if (has_w || has_b) pl.params = bestP <= kNormRegsP ? LSQ_NORM_W8_PARAMS_REGS : LSQ_NORM_W8_PARAMS_LDS;
    if (pl.params == LSQ_NORM_W8_PARAMS_LDS) pl.lds = static_cast<int>(4 * C * ((has_w ? 1 : 0) + (has_b ? 1 : 0)));
    return pl;
}

typedef void (*NormKernel)(NormGeom, NormArg, const uint8_t*, void*);

template <int L>
inline NormKernel packets_kernel_of(int P) {
    switch (P) {
        case 1: return norm_w8_packets_kernel<L, 1>;
        case 2: return norm_w8_packets_kernel<L, 2>;
        case 3: return norm_w8_packets_kernel<L, 3>;
        case 4: return norm_w8_packets_kernel<L, 4>;
        case 5: return norm_w8_packets_kernel<L, 5>;
        case 6: return norm_w8_packets_kernel<L, 6>;
        case 7: return norm_w8_packets_kernel<L, 7>;
        default: return norm_w8_packets_kernel<L, 8>;
    }
}

inline NormKernel packets_kernel(int L, int P) {
    switch (L) {
        case 4: return packets_kernel_of<4>(P);
        case 8: return packets_kernel_of<8>(P);
        case 16: return packets_kernel_of<16>(P);
        case 32: return packets_kernel_of<32>(P);
        default: return packets_kernel_of<64>(P);
    }
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_norm_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

int check_geom(const char* what, const lsq_norm_w8_geom* g) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (g->kind != LSQ_NORM_W8_LAYER && g->kind != LSQ_NORM_W8_RMS)
        return fail(LSQ_EINVAL, "%s: kind must be LSQ_NORM_W8_LAYER (0) or LSQ_NORM_W8_RMS (1), got %lld", what, static_cast<ll>(g->kind));
    if (g->x_dtype != LSQ_NORM_W8_U8 && g->x_dtype != LSQ_NORM_W8_I8)
        return fail(LSQ_EINVAL, "%s: x_dtype must be LSQ_NORM_W8_U8 (0) or LSQ_NORM_W8_I8 (1), got %lld", what, static_cast<ll>(g->x_dtype));
    if (g->R < 1 || g->C < 1)
        return fail(LSQ_EINVAL, "%s: x is [R, C] = [%lld, %lld], every extent must be at least 1", what, static_cast<ll>(g->R), static_cast<ll>(g->C));
    if (g->C > LSQ_NORM_W8_MAX_C)
        return fail(LSQ_EINVAL, "%s: C = %lld, at most %d elements per row are served (the row sums stay in 32 bits)", what,
                    static_cast<ll>(g->C), LSQ_NORM_W8_MAX_C);
    if (g->R > INT32_MAX / 4) return fail(LSQ_EINVAL, "%s: R = %lld is beyond 29 bits", what, static_cast<ll>(g->R));
    return LSQ_OK;
}

// the constants, into `arg` (the caller's, zeroed); the bytes of one element of y into `y_elem`
int check_consts(const char* what, const lsq_norm_w8_geom* g, const lsq_norm_w8_consts* c, lsq::NormArg& arg, int64_t& y_elem) {
    if (!c) return fail(LSQ_EINVAL, "%s: NULL constants", what);
    if ((c->weight || c->bias) && !float_dtype(c->param_dtype))
        return fail(LSQ_EINVAL, "%s: param_dtype must be LSQ_F32, LSQ_BF16 or LSQ_F16, got code %lld", what, static_cast<ll>(c->param_dtype));
    if (!c->s_x || !c->zx) return fail(LSQ_EINVAL, "%s: NULL s_x or zx", what);
    if (!aligned_to(c->s_x, 4) || !aligned_to(c->zx, 4)) return fail(LSQ_EINVAL, "%s: s_x and zx must be element-aligned", what);
    const uintptr_t pb = (c->weight || c->bias) ? elem_bytes(static_cast<int>(c->param_dtype)) : 1;
    if ((c->weight && !aligned_to(c->weight, pb)) || (c->bias && !aligned_to(c->bias, pb)))
        return fail(LSQ_EINVAL, "%s: weight and bias must be element-aligned", what);
    if (int rc = check_out_side(what, *c, arg, y_elem)) return rc;
    if (!(c->eps >= 0.0f)) return fail(LSQ_EINVAL, "%s: eps = %g must be a number that is not negative", what, static_cast<double>(c->eps));
    arg.s_x = static_cast<const float*>(c->s_x);
    arg.zx = static_cast<const int32_t*>(c->zx);
    arg.w = c->weight;
    arg.b = c->bias;
    arg.eps = c->eps;
    arg.pdt = static_cast<int>(c->param_dtype);
    arg.rms = g->kind == LSQ_NORM_W8_RMS ? 1 : 0;
    arg.flip = g->x_dtype == LSQ_NORM_W8_I8 ? 0x80808080u : 0u;
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_norm_w8_abi_version(void) { return LSQ_NORM_W8_ABI_VERSION; }

const char* lsq_norm_w8_last_error(void) { return g_last_error; }

int lsq_norm_w8(const lsq_norm_w8_geom* geom, const lsq_norm_w8_consts* consts, const void* x_levels, void* y, void* stream) {
    const char* what = "lsq_norm_w8";
    lsq::NormArg arg{};
    int64_t y_elem = 1;
    if (int rc = check_geom(what, geom)) return rc;
    if (int rc = check_consts(what, geom, consts, arg, y_elem)) return rc;
    if (!x_levels || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    const int64_t elems = geom->R * geom->C, y_bytes = elems * y_elem;
    if (overlap(y, y_bytes, x_levels, elems))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap x's %lld: the norm in place is not served", what, static_cast<ll>(y_bytes),
                    static_cast<ll>(elems));
    const int64_t p_bytes = geom->C * static_cast<int64_t>((consts->weight || consts->bias) ? elem_bytes(static_cast<int>(consts->param_dtype)) : 1);
    if ((consts->weight && overlap(y, y_bytes, consts->weight, p_bytes)) || (consts->bias && overlap(y, y_bytes, consts->bias, p_bytes)))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap the weight's or the bias's %lld", what, static_cast<ll>(y_bytes), static_cast<ll>(p_bytes));
    if (!aligned_to(y, static_cast<uintptr_t>(y_elem))) return fail(LSQ_EINVAL, "%s: a floating y must be element-aligned", what);
    const lsq::NormPlan pl = lsq::plan_norm(geom->R, geom->C, aligned_to(x_levels, 16) && aligned_to(y, 16), consts->weight != nullptr,
                                            consts->bias != nullptr);
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kBlock);
    const uint8_t* x = static_cast<const uint8_t*>(x_levels);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pl.family == LSQ_NORM_W8_PACKETS)
        hipLaunchKernelGGL(lsq::packets_kernel(pl.L, pl.P), grid, block, static_cast<size_t>(pl.lds), st, pl.g, arg, x, y);
    else
        hipLaunchKernelGGL(lsq::norm_w8_generic_kernel, grid, block, 0, st, pl.g, arg, x, y);
    return hip_status(hipGetLastError(), what);
}

int lsq_norm_w8_plan(const lsq_norm_w8_geom* geom, int aligned, int has_weight, int has_bias, int32_t* out8) {
    const char* what = "lsq_norm_w8_plan";
    if (int rc = check_geom(what, geom)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::NormPlan pl = lsq::plan_norm(geom->R, geom->C, aligned != 0, has_weight != 0, has_bias != 0);
    out8[0] = pl.family;
    out8[1] = static_cast<int32_t>(pl.grid);
    out8[2] = pl.block;
    out8[3] = pl.L;
    out8[4] = pl.P;
    out8[5] = pl.rows;
    out8[6] = pl.params;
    out8[7] = pl.lds;
    return LSQ_OK;
}

}  // extern "C"
