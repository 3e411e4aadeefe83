// lsq_attn_mask_w8.hip -- the masked softmax on 8-bit levels on gfx950 (include/lsq_hip_attn_mask_w8.h, which states the contract):
// the kernels and the C ABI of liblsq_hip_attn_mask_w8.so.  The integer-table softmax of ../attn_w8/lsq_attn_w8.hip over the first
// n_r bytes of row r; every output beyond n_r is the output side's level of 0 (or +0.0f).
//
//  * PACKETS (C <= 8192, bases and ldx, ldy multiples of 16): a row lives in the registers of a group of L lanes, P packets per lane
//    (L, P and the rows per workgroup by lsq_softmax_w8_plan's rule applied to C).  A lane computes its row's n (key_lengths is
//    read once per row), loads packet p only if 16 p < n -- a predicated load: no address outside the prefix's packets is formed --,
//    masks the tail with n - 16 p, and looks up the table for the valid bytes of a packet that has any.  The byte max, the 32-bit
//    partial sum widened to 64 bits before it crosses lanes, the one division (none for n = 0) and the value are the unmasked
//    kernel's.  All ceil(C / 16) packets of y are stored; a masked position is u = 0 through the same w8o_byte or float store.
//    Every lane of a group takes part in every shuffle, whatever its n; a group past the last row recomputes the last row and
//    stores nothing.
//  * GENERIC (every other legal call): one wave per row, three passes over i < n, then the zero tail, the table from memory.
//
// msk_store16 is smx_store16 of lsq_attn_w8.hip and plan_softmax_mask is its plan_softmax, copied: moved into a shared header
// they would have to leave that library's machine code exactly as it is, and this file must not depend on it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../lsq_kernels.hpp"
#include "../lsq_companion_abi.hpp"
#include "../qlinear_w8/lsq_w8_shared.hpp"
#include "../attn_w8/lsq_attn_w8_dev.hpp"
#include "../attn_w8/lsq_attn_w8_checks.hpp"
#include "../../../include/lsq_hip_attn_mask_w8.h"

namespace lsq {

typedef __attribute__((ext_vector_type(2))) unsigned short msk_u16x2;

constexpr int kMskMaxP = 8;
constexpr int kMskWave = 64;
constexpr int kMskRows = 4;                     // rows a group walks where the grid stays large
constexpr int64_t kMskFill = 512;               // ... that is: at least this many workgroups
static_assert(kBlock == 256, "four waves per workgroup");

struct MskGeom {            // kernel argument
    int64_t R, ldx, ldy;
    int64_t off;            // causal: row t sees t + 1 + off keys
    int C, packets, K;      // elements of a row, ceil(C / 16), rows per group
    int Tq, rpl;            // rows of one matrix; rows that share one length
    int causal;
    uint32_t flip;          // 0x80808080 for int8 levels (biased by 128 on load), 0 for uint8
};

// n_r of the contract; row < R < 2^29
__device__ __forceinline__ int msk_prefix(const MskGeom& g, const int32_t* __restrict__ lens, int64_t row) {
    const uint32_t r = static_cast<uint32_t>(row);
    int64_t n = g.C;
    if (g.causal) n = min(n, static_cast<int64_t>(r % static_cast<uint32_t>(g.Tq)) + 1 + g.off);
    if (lens) n = min(n, static_cast<int64_t>(max(lens[r / static_cast<uint32_t>(g.rpl)], 0)));
    return static_cast<int>(n);
}

// a packet of outputs, the first `cnt` of them stored: `at` in elements of y; y 16-byte aligned, at % 16 == 0
__device__ __forceinline__ void msk_store16(void* y, int64_t at, const float (&u)[16], int cnt, const AttnQ& q) {
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
__global__ __launch_bounds__(kBlock) void softmax_mask_w8_packets_kernel(MskGeom g, AttnOut o, const int32_t* __restrict__ table,
                                                                         const int32_t* __restrict__ lens,
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
        const int n = msk_prefix(g, lens, rr);          // the same in every lane of the group; 0 <= n <= C
        const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(x + rr * g.ldx);
        u32x4 v[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int p = lane + j * L;
            v[j] = u32x4{0u, 0u, 0u, 0u};
            if (16 * p < n) v[j] = src[p];              // 16 p < n <= C: a packet of the row that holds a byte of the prefix
        }
#pragma unroll
        for (int j = 0; j < P; ++j) asm volatile("" : "+v"(v[j]));                      // all in flight at once
        // the byte max over the prefix: bytes beyond n (and whole packets beyond it) count as 0, the least biased byte
        msk_u16x2 me = {0, 0}, mo = {0, 0};
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int p = lane + j * L;
            v[j] = attn_mask_tail(v[j] ^ g.flip, max(n - 16 * p, 0));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                me = __builtin_elementwise_max(me, __builtin_bit_cast(msk_u16x2, v[j][i] & 0x00ff00ffu));
                mo = __builtin_elementwise_max(mo, __builtin_bit_cast(msk_u16x2, (v[j][i] >> 8) & 0x00ff00ffu));
            }
        }
        me = __builtin_elementwise_max(me, mo);
        int m = max(static_cast<int>(me[0]), static_cast<int>(me[1]));
#pragma unroll
        for (int s = L / 2; s >= 1; s /= 2) m = max(m, __shfl_xor(m, s));
        // the sum over the prefix: at most 128 entries of at most 2^24 per lane fit 32 bits; 64 across lanes
        uint32_t part = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int valid = min(max(n - 16 * (lane + j * L), 0), 16);
            if (valid > 0) {                            // a wholly masked packet looks nothing up
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int b = static_cast<int>((v[j][i / 4] >> (8 * (i % 4))) & 0xffu);
                    part += i < valid ? static_cast<uint32_t>(tab[(m - b) & 0xff]) : 0u;
                }
            }
        }
        uint64_t S = part;
#pragma unroll
        for (int s = L / 2; s >= 1; s /= 2) S += smx_shfl_xor_u64(S, s);
        float r = 0.0f;
        if (n > 0) r = __fdiv_rn(1.0f, static_cast<float>(S));      // n = 0: S = 0, nothing is divided and no p is formed
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int p = lane + j * L;
            const int cnt = min(max(g.C - 16 * p, 0), 16), valid = min(max(n - 16 * p, 0), 16);
            float u[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) u[i] = 0.0f;   // +0.0f beyond the prefix: the output side's own level of 0
            if (valid > 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int b = static_cast<int>((v[j][i / 4] >> (8 * (i % 4))) & 0xffu);
                    const float pv = smx_value(tab[(m - b) & 0xff], r, q.mid);
                    u[i] = i < valid ? pv : 0.0f;
                }
            }
            if (live && cnt > 0) msk_store16(y, rr * g.ldy + 16 * static_cast<int64_t>(p), u, cnt, q);
        }
    }
}

// one wave per row: lane l takes the bytes l, l + 64, ... < n in all three passes, then the zeros of n .. C - 1
__global__ __launch_bounds__(kBlock) void softmax_mask_w8_generic_kernel(MskGeom g, AttnOut o, const int32_t* __restrict__ table,
                                                                         const int32_t* __restrict__ lens,
                                                                         const uint8_t* __restrict__ x, void* __restrict__ y) {
    const int lane = static_cast<int>(threadIdx.x) & (kMskWave - 1);
    const int64_t row = static_cast<int64_t>(blockIdx.x) * (kBlock / kMskWave) + static_cast<int>(threadIdx.x) / kMskWave;
    if (row >= g.R) return;                        // a whole wave leaves
    const AttnQ q = attn_constants(o);
    const int n = msk_prefix(g, lens, row);
    const uint8_t* __restrict__ src = x + row * g.ldx;
    const uint32_t flip = g.flip & 0xffu;
    int m = 0;
    for (int i = lane; i < n; i += kMskWave) m = max(m, static_cast<int>(static_cast<uint32_t>(src[i]) ^ flip));
#pragma unroll
    for (int s = kMskWave / 2; s >= 1; s /= 2) m = max(m, __shfl_xor(m, s));
    uint64_t S = 0;
    for (int i = lane; i < n; i += kMskWave) S += static_cast<uint32_t>(table[(m - static_cast<int>(static_cast<uint32_t>(src[i]) ^ flip)) & 0xff]);
#pragma unroll
    for (int s = kMskWave / 2; s >= 1; s /= 2) S += smx_shfl_xor_u64(S, s);
    float r = 0.0f;
    if (n > 0) r = __fdiv_rn(1.0f, static_cast<float>(S));
    for (int i = lane; i < g.C; i += kMskWave) {
        float u = 0.0f;
        if (i < n) u = smx_value(table[(m - static_cast<int>(static_cast<uint32_t>(src[i]) ^ flip)) & 0xff], r, q.mid);
        const int64_t at = row * g.ldy + i;
        if (q.levels_out) static_cast<uint8_t*>(y)[at] = static_cast<uint8_t>(w8o_byte(u, q));
        else w8o_store_float(y, at, u, q.mid);
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan -- lsq_softmax_w8_plan's rule applied to C
// ------------------------------------------------------------------------------------------------
struct MskPlan {
    int family, block, L, P, rows, lds;
    int64_t grid;
    MskGeom g;
};

inline MskPlan plan_softmax_mask(const lsq_softmax_mask_w8_geom& ge, bool aligned, bool has_lengths) {
    MskPlan pl = {};
    pl.block = kBlock;
    const int packets = static_cast<int>(ceil_div(ge.C, 16));
    pl.g = MskGeom{ge.R, ge.ldx, ge.ldy, ge.causal_offset, static_cast<int>(ge.C), packets, 1, static_cast<int>(ge.Tq),
                   has_lengths ? static_cast<int>(ge.rows_per_length) : 1, static_cast<int>(ge.causal),
                   ge.x_dtype == LSQ_ATTN_W8_I8 ? 0x80808080u : 0u};
    if (!(aligned && ge.ldx % 16 == 0 && ge.ldy % 16 == 0 && ge.C <= 16 * kMskWave * kMskMaxP)) {
        pl.family = LSQ_ATTN_W8_GENERIC;
        pl.L = kMskWave;
        pl.rows = kBlock / kMskWave;
        pl.grid = ceil_div(ge.R, pl.rows);
        return pl;
    }
    int P = 1;
    while (ceil_div(packets, P) > kMskWave) P *= 2;
    int L = 4;
    while (L < ceil_div(packets, P)) L *= 2;
    const int G = kBlock / L;
    const int K = ceil_div(ge.R, static_cast<int64_t>(G) * kMskRows) >= kMskFill ? kMskRows : 1;
    pl.family = LSQ_ATTN_W8_PACKETS;
    pl.L = L;
    pl.P = P;
    pl.rows = G * K;
    pl.g.K = K;
    pl.grid = ceil_div(ge.R, pl.rows);
    pl.lds = 1024;
    return pl;
}

typedef void (*MskKernel)(MskGeom, AttnOut, const int32_t*, const int32_t*, const uint8_t*, void*);

inline MskKernel mask_packets_kernel(int L, int P) {
    switch (L) {
        case 4: return softmax_mask_w8_packets_kernel<4, 1>;
        case 8: return softmax_mask_w8_packets_kernel<8, 1>;
        case 16: return softmax_mask_w8_packets_kernel<16, 1>;
        case 32: return softmax_mask_w8_packets_kernel<32, 1>;
        default: break;
    }
    switch (P) {            // more than one packet per lane: the group is a whole wave
        case 1: return softmax_mask_w8_packets_kernel<64, 1>;
        case 2: return softmax_mask_w8_packets_kernel<64, 2>;
        case 4: return softmax_mask_w8_packets_kernel<64, 4>;
        default: return softmax_mask_w8_packets_kernel<64, 8>;
    }
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_attn_mask_w8.h: validation, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

int check_mask_geom(const char* what, const lsq_softmax_mask_w8_geom* g, bool has_lengths) {
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
    if (g->Tq < 1 || g->R % g->Tq != 0)
        return fail(LSQ_EINVAL, "%s: Tq = %lld must be at least 1 and divide R = %lld", what, static_cast<ll>(g->Tq), static_cast<ll>(g->R));
    if (has_lengths && (g->rows_per_length < 1 || g->rows_per_length % g->Tq != 0 || g->R % g->rows_per_length != 0))
        return fail(LSQ_EINVAL, "%s: rows_per_length = %lld must be at least 1, a multiple of Tq = %lld and divide R = %lld", what,
                    static_cast<ll>(g->rows_per_length), static_cast<ll>(g->Tq), static_cast<ll>(g->R));
    if (g->causal != 0 && g->causal != 1) return fail(LSQ_EINVAL, "%s: causal must be 0 or 1, got %lld", what, static_cast<ll>(g->causal));
    if (g->causal_offset < 0 || g->causal_offset > INT32_MAX)
        return fail(LSQ_EINVAL, "%s: causal_offset = %lld must be at least 0 and within 31 bits", what, static_cast<ll>(g->causal_offset));
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_attn_mask_w8_abi_version(void) { return LSQ_ATTN_MASK_W8_ABI_VERSION; }

const char* lsq_attn_mask_w8_last_error(void) { return g_last_error; }

int lsq_softmax_mask_w8(const lsq_softmax_mask_w8_geom* geom, const lsq_attn_w8_out* out, const void* table, const void* key_lengths,
                        const void* x_levels, void* y, void* stream) {
    const char* what = "lsq_softmax_mask_w8";
    lsq::AttnOut oarg{};
    int64_t y_elem = 1;
    const bool has_lengths = key_lengths != nullptr;
    if (int rc = check_mask_geom(what, geom, has_lengths)) return rc;
    if (int rc = check_out(what, out, oarg, y_elem)) return rc;
    if (!table || !x_levels || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(table, 4)) return fail(LSQ_EINVAL, "%s: the table must be element-aligned", what);
    if (has_lengths && !aligned_to(key_lengths, 4)) return fail(LSQ_EINVAL, "%s: key_lengths must be 4-byte aligned", what);
    if (!aligned_to(y, static_cast<uintptr_t>(y_elem))) return fail(LSQ_EINVAL, "%s: a floating y must be element-aligned", what);
    const int64_t x_bytes = (geom->R - 1) * geom->ldx + geom->C, y_bytes = ((geom->R - 1) * geom->ldy + geom->C) * y_elem;
    if (overlap(y, y_bytes, x_levels, x_bytes) || overlap(y, y_bytes, table, 1024))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap x's %lld or the table: the softmax in place is not served", what,
                    static_cast<ll>(y_bytes), static_cast<ll>(x_bytes));
    if (has_lengths && overlap(y, y_bytes, key_lengths, 4 * (geom->R / geom->rows_per_length)))
        return fail(LSQ_EINVAL, "%s: y's %lld bytes overlap the %lld entries of key_lengths", what, static_cast<ll>(y_bytes),
                    static_cast<ll>(geom->R / geom->rows_per_length));
    const lsq::MskPlan pl = lsq::plan_softmax_mask(*geom, aligned_to(x_levels, 16) && aligned_to(y, 16), has_lengths);
    if (int rc = check_grid(what, pl.grid)) return rc;
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(lsq::kBlock);
    const uint8_t* x = static_cast<const uint8_t*>(x_levels);
    const int32_t* tb = static_cast<const int32_t*>(table);
    const int32_t* ln = static_cast<const int32_t*>(key_lengths);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pl.family == LSQ_ATTN_W8_PACKETS) hipLaunchKernelGGL(lsq::mask_packets_kernel(pl.L, pl.P), grid, block, 0, st, pl.g, oarg, tb, ln, x, y);
    else hipLaunchKernelGGL(lsq::softmax_mask_w8_generic_kernel, grid, block, 0, st, pl.g, oarg, tb, ln, x, y);
    return hip_status(hipGetLastError(), what);
}

int lsq_softmax_mask_w8_plan(const lsq_softmax_mask_w8_geom* geom, int aligned, int has_lengths, int32_t* out8) {
    const char* what = "lsq_softmax_mask_w8_plan";
    if (int rc = check_mask_geom(what, geom, has_lengths != 0)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::MskPlan pl = lsq::plan_softmax_mask(*geom, aligned != 0, has_lengths != 0);
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
