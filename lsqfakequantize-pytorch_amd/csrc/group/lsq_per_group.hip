// lsq_per_group.hip -- group-wise LSQ on gfx950 (include/lsq_hip_group.h): one scale / shift per run of G consecutive
// elements, the per-channel arithmetic of lsq_math.hpp on the [1, n / G, G] view.
//
// Both ops are flat streams, like K1 / K2 (lsq_per_tensor.hip): a persistent grid, 16-byte packets moved with one
// global_load / global_store_dwordx4 each, UNROLL independent packets per lane in flight, non-temporal hints on the
// streams.  Two forms, chosen on the host:
//  * PACKET form (G % V == 0, V = elements per packet): a packet lies in one group; its constants are derived once per
//    packet from scale[g] / shift[g] (small arrays: 8 / G bytes per fp32 element, served by the caches);
//  * ELEMENT form (G % V != 0, G < V included): one element per lane, its group's constants per element.
// Backward: a WAVE owns whole groups, so every group's d_scale / d_shift is finished in registers -- one launch, no
// workspace, no finalize, no atomics, and a summation order that depends only on (n, G, grid): bit-identical launch
// after launch.  Per lane the terms of a packet are added in fp64, then
//  * P2 (packet form, packets per group PG a power of two): the wave walks units of max(64 * UNROLL, PG) packets, a
//    unit being whole groups.  PG <= 64: a butterfly over the PG lanes of each group per pass of 64 packets; PG > 64:
//    lane sums accumulate over the group's passes, one butterfly over the wave at its end.  The group's first lane stores.
//  * SCAN (every other G): a wave owns a contiguous range of whole groups and walks it 64 items (packets or elements) per
//    pass; a segmented inclusive scan keyed by "this item starts a group" leaves each group's pass total on its last
//    item's lane, and the part of a group that continues into the next pass is carried in a wave-uniform register.
// All indexing is 64-bit (tensors and group counts beyond 2^31).
#include "../lsq_kernels.hpp"

namespace lsq {

constexpr int kGrpUnroll = 4;
constexpr int kGrpFwdBlocksPerCU = 16;   // K1's tuned forward grid (kDefaultFwdVariant)
constexpr int kGrpBwdBlocksPerCU = 4;

enum GrpBwdMode { kP2 = 0, kScanPacket = 1, kScanElem = 2 };

// n / d for the group index of an element or packet: a multiply-high by floor((2^64 - 1) / d) and at most two
// corrections -- integer instructions only (hipcc expands a 64-bit `/` into float reciprocal + FMA sequences, which would
// blur the "no FMA outside the IEEE division" rule of the device-code tests, and costs more)
struct DivU64 {
    uint64_t d, m;
    __device__ __forceinline__ int64_t div(int64_t n) const {
        uint64_t q = __umul64hi(static_cast<uint64_t>(n), m);
        uint64_t r = static_cast<uint64_t>(n) - q * d;
        if (r >= d) { ++q; r -= d; }
        if (r >= d) ++q;
        return static_cast<int64_t>(q);
    }
};
inline DivU64 make_div(int64_t d) { return DivU64{static_cast<uint64_t>(d), ~uint64_t{0} / static_cast<uint64_t>(d)}; }

// lane `src`'s value, in every lane
__device__ __forceinline__ double bcast_f64(double v, int src) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl(lo, src, 64);
    hi = __shfl(hi, src, 64);
    return __hiloint2double(hi, lo);
}

template <typename T>
__device__ __forceinline__ QParams<T> group_qparams(const T* __restrict__ scale, const T* __restrict__ shift, int64_t g,
                                                    const Range<T>& r) {
    return make_qparams<T>(sanitize_scale_per_channel<T>(scale[g]), shift[g], r);   // lsq_kernel.h:157-158, :12
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <typename IO, bool INIT, bool LEVELS, bool PACKET>
__global__ __launch_bounds__(kBlock) void fwd_grp_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                         int8_t* __restrict__ levels, int level_bias, int aux_kind,
                                                         int64_t n, int64_t G, int pg_shift, DivU64 per_group,
                                                         const typename IO::arith* __restrict__ scale,
                                                         const typename IO::arith* __restrict__ shift,
                                                         Range<typename IO::arith> r) {
    // per_group: division by the elements (element form) resp. packets (packet form) of one group
    using T = typename IO::arith;
    constexpr int VEC = IO::VEC;
    const T bias = static_cast<T>(level_bias);
    if constexpr (!PACKET) {
        for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
             i += static_cast<int64_t>(gridDim.x) * kBlock) {
            const QParams<T> q = group_qparams<T>(scale, shift, per_group.div(i), r);
            const T xv = IO::load1(x, i);
            const T c = clamped<T>(xv, q, r);
            if (!LEVELS || y != nullptr) store_out<IO, INIT>(y, i, INIT ? xv : dequant<T>(rne(c), q));
            if (LEVELS) levels[i] = aux_byte<T>(c, r, bias, aux_kind);
        }
        return;
    } else {
        const int64_t n_packets = n / VEC;          // exact: n % G == 0 and G % VEC == 0
        constexpr int64_t kTile = static_cast<int64_t>(kBlock) * kGrpUnroll;
        const int64_t n_full = n_packets / kTile;
        auto emit = [&](const Packet<IO>& in, int64_t p) {
            const QParams<T> q = group_qparams<T>(scale, shift, pg_shift >= 0 ? (p >> pg_shift) : per_group.div(p), r);
            Packet<IO> out;
            LevelPack<VEC> lv;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const T xv = static_cast<T>(in.v[j]);
                const T c = clamped<T>(xv, q, r);
                out.v[j] = out_elem<IO, INIT>(INIT ? xv : dequant<T>(rne(c), q));   // lsq_kernel.h:13
                if (LEVELS) lv.b[j] = aux_byte<T>(c, r, bias, aux_kind);
            }
            if (!LEVELS || y != nullptr) store_packet_nt<IO>(y, p * VEC, out);
            if (LEVELS) lv.store(levels + p * VEC);
        };
        for (int64_t tile = blockIdx.x; tile < n_full; tile += gridDim.x) {
            const int64_t p0 = tile * kTile + threadIdx.x;
            Packet<IO> in[kGrpUnroll];
#pragma unroll
            for (int u = 0; u < kGrpUnroll; ++u) in[u] = load_packet_nt<IO>(x, (p0 + static_cast<int64_t>(u) * kBlock) * VEC);
#pragma unroll
            for (int u = 0; u < kGrpUnroll; ++u) emit(in[u], p0 + static_cast<int64_t>(u) * kBlock);
        }
        if (static_cast<int64_t>(blockIdx.x) == n_full % gridDim.x) {     // the one partial tile
            for (int64_t p = n_full * kTile + threadIdx.x; p < n_packets; p += kBlock) emit(load_packet<IO>(x, p * VEC), p);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
template <typename T, bool SYM, bool INIT, bool EVAL>
struct GrpTerms {
    // dx of one element and its d_scale / d_shift terms (scaled, lsq_kernel.h:122) added to the lane's fp64 sums
    __device__ __forceinline__ static T step(T g, T x, const QParams<T>& q, const Range<T>& r, T gs, double& s, double& b) {
        if (EVAL) return backward_elem_eval<T, INIT>(g, x, q, r);
        T ds_t, db_t;
        const T dX = backward_elem<T, SYM, INIT>(g, x, q, r, gs, ds_t, db_t);
        s += static_cast<double>(ds_t);
        if (!SYM) b += static_cast<double>(db_t);
        return dX;
    }
};

template <typename T, bool SYM, bool EVAL>
__device__ __forceinline__ void store_group(T* __restrict__ ds, T* __restrict__ db, int64_t g, double s, double b, T sym_term) {
    if (EVAL) {                                   // lsq_kernel.h:142-144
        ds[g] = static_cast<T>(0);
        db[g] = static_cast<T>(0);
        return;
    }
    ds[g] = static_cast<T>(s);
    db[g] = SYM ? static_cast<T>(0.0 + static_cast<double>(sym_term)) : static_cast<T>(b);   // sum of G copies of 0 * gs
}

template <typename IO, bool SYM, bool INIT, bool EVAL, int MODE>
__global__ __launch_bounds__(kBlock) void bwd_grp_kernel(const void* __restrict__ grad, const void* __restrict__ x,
                                                         void* __restrict__ dx, typename IO::arith* __restrict__ ds,
                                                         typename IO::arith* __restrict__ db, int64_t n, int64_t G,
                                                         int pg_shift, DivU64 per_group, int64_t groups_per_wave,
                                                         const typename IO::arith* __restrict__ scale,
                                                         const typename IO::arith* __restrict__ shift,
                                                         Range<typename IO::arith> r, typename IO::arith gs,
                                                         typename IO::arith sym_term) {
    using T = typename IO::arith;
    using Acc = GrpTerms<T, SYM, INIT, EVAL>;
    constexpr int VEC = IO::VEC;
    constexpr bool PACKET = MODE != kScanElem;
    const int lane = threadIdx.x & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    const int64_t n_items = PACKET ? n / VEC : n;
    const int64_t gi = PACKET ? G / VEC : G;      // items per group

    // one item (packet or element) -> dx, and its terms into (s, b)
    auto item = [&](const Packet<IO>& gp, const Packet<IO>& xp, int64_t it, int64_t grp, double& s, double& b) {
        const QParams<T> q = group_qparams<T>(scale, shift, grp, r);
        if constexpr (PACKET) {
            Packet<IO> out;
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                out.v[j] = out_elem<IO, INIT>(Acc::step(static_cast<T>(gp.v[j]), static_cast<T>(xp.v[j]), q, r, gs, s, b));
            store_packet_nt<IO>(dx, it * VEC, out);
        } else {
            store_out<IO, INIT>(dx, it, Acc::step(static_cast<T>(gp.v[0]), static_cast<T>(xp.v[0]), q, r, gs, s, b));
        }
    };
    auto load = [&](const void* base, int64_t it) {
        Packet<IO> pk;
        if constexpr (PACKET) {
            pk = load_packet_nt<IO>(base, it * VEC);
        } else {
            pk.v[0] = static_cast<const typename IO::elem*>(base)[it];
        }
        return pk;
    };

    if constexpr (MODE == kP2) {
        // units of max(64 * UNROLL, PG) packets: whole groups, walked 64 * UNROLL packets at a time
        constexpr int64_t kStep = 64 * kGrpUnroll;
        const int64_t pg = gi;
        const int64_t unit = pg > kStep ? pg : kStep;
        const int64_t n_units = (n_items + unit - 1) / unit;
        double acc_s = 0.0, acc_b = 0.0;          // PG > 64: the lane's share of the current group
        for (int64_t u0 = wave; u0 < n_units; u0 += n_waves) {
            const int64_t u_end = (u0 + 1) * unit < n_items ? (u0 + 1) * unit : n_items;
            for (int64_t base = u0 * unit; base < u_end; base += kStep) {
                const bool whole = base + kStep <= u_end;
                Packet<IO> gp[kGrpUnroll], xp[kGrpUnroll];
#pragma unroll
                for (int k = 0; k < kGrpUnroll; ++k) {
                    const int64_t it = base + k * 64 + lane;
                    if (whole || it < u_end) {
                        gp[k] = load(grad, it);
                        xp[k] = load(x, it);
                    }
                }
#pragma unroll
                for (int k = 0; k < kGrpUnroll; ++k) {
                    const int64_t pass = base + k * 64;            // first packet of this pass (wave-uniform)
                    if (!whole && pass >= u_end) break;            // (a partial unit ends on a group boundary)
                    const int64_t it = pass + lane;
                    const bool live = whole || it < u_end;
                    const int64_t grp = it >> pg_shift;            // (P2: PG is a power of two)
                    double s = 0.0, b = 0.0;
                    if (live) item(gp[k], xp[k], it, grp, s, b);
                    if constexpr (EVAL) {
                        if (live && (it & (pg - 1)) == 0) store_group<T, SYM, EVAL>(ds, db, grp, 0.0, 0.0, sym_term);
                    } else if (pg <= 64) {
                        for (int d = 1; d < pg; d <<= 1) {             // butterfly inside each group's PG lanes
                            s += shfl_xor_f64(s, d);
                            if (!SYM) b += shfl_xor_f64(b, d);
                        }
                        if (live && (lane & (pg - 1)) == 0) store_group<T, SYM, EVAL>(ds, db, grp, s, b, sym_term);
                    } else {
                        acc_s += s;
                        acc_b += b;
                        if (((pass + 64) & (pg - 1)) == 0) {           // the group's last pass
                            acc_s = wave_sum(acc_s);
                            if (!SYM) acc_b = wave_sum(acc_b);
                            if (lane == 0) store_group<T, SYM, EVAL>(ds, db, grp, acc_s, acc_b, sym_term);
                            acc_s = 0.0;
                            acc_b = 0.0;
                        }
                    }
                }
            }
        }
    } else {
        // SCAN: this wave's groups [g_lo, g_hi), items [g_lo * gi, g_hi * gi), 64 items per pass
        const int64_t n_groups = n / G;
        const int64_t g_lo = wave * groups_per_wave;
        if (g_lo >= n_groups) return;
        const int64_t g_hi = g_lo + groups_per_wave < n_groups ? g_lo + groups_per_wave : n_groups;
        const int64_t i_end = g_hi * gi;
        int64_t g0 = g_lo, r0 = 0;                // group and offset in it of the pass's first item (wave-uniform)
        double carry_s = 0.0, carry_b = 0.0;      // sums of the pass's first group from earlier passes
        for (int64_t base = g_lo * gi; base < i_end; base += 64 * kGrpUnroll) {
            Packet<IO> gp[kGrpUnroll], xp[kGrpUnroll];
#pragma unroll
            for (int k = 0; k < kGrpUnroll; ++k) {
                const int64_t it = base + k * 64 + lane;
                if (it < i_end) {
                    gp[k] = load(grad, it);
                    xp[k] = load(x, it);
                }
            }
#pragma unroll
            for (int k = 0; k < kGrpUnroll; ++k) {
                const int64_t it = base + k * 64 + lane;
                if (base + k * 64 >= i_end) break;
                const bool live = it < i_end;
                // this lane's group and offset: r0 + lane, reduced once (gi >= 64) or by a division (gi < 64)
                int64_t rl, gl;
                const int64_t t = r0 + lane;
                if (gi >= 64) {
                    const bool over = t >= gi;
                    rl = over ? t - gi : t;
                    gl = g0 + (over ? 1 : 0);
                } else {
                    const int64_t qd = per_group.div(t);
                    rl = t - qd * gi;
                    gl = g0 + qd;
                }
                double s = 0.0, b = 0.0;
                if (live) item(gp[k], xp[k], it, gl, s, b);
                const bool last = live && rl == gi - 1;
                if constexpr (EVAL) {
                    if (last) store_group<T, SYM, EVAL>(ds, db, gl, 0.0, 0.0, sym_term);
                } else {
                    // segmented inclusive scan; a head (an item that starts a group, or lane 0) stops the sums from below
                    int head = (rl == 0 || lane == 0) ? 1 : 0;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const double os = shfl_up_f64(s, d);
                        const double ob = SYM ? 0.0 : shfl_up_f64(b, d);
                        const int oh = __shfl_up(head, d, 64);
                        if (lane >= d && !head) {
                            s = os + s;
                            if (!SYM) b = ob + b;
                        }
                        if (lane >= d) head |= oh;
                    }
                    if (lane < gi - r0) {                          // the pass's first group: add what earlier passes summed
                        s = carry_s + s;
                        if (!SYM) b = carry_b + b;
                    }
                    if (last) store_group<T, SYM, EVAL>(ds, db, gl, s, b, sym_term);
                    // lane 63's group continues into the next pass unless it ends here
                    const double ts = bcast_f64(s, 63), tb = SYM ? 0.0 : bcast_f64(b, 63);
                    const bool ends = __shfl(last ? 1 : 0, 63, 64) != 0;
                    carry_s = ends ? 0.0 : ts;
                    carry_b = ends ? 0.0 : tb;
                }
                const int64_t t64 = r0 + 64;
                if (gi >= 64) {
                    const bool over = t64 >= gi;
                    r0 = over ? t64 - gi : t64;
                    g0 += over ? 1 : 0;
                } else {
                    const int64_t qd = per_group.div(t64);
                    r0 = t64 - qd * gi;
                    g0 += qd;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan (one rule for the launches and for lsq_group_plan) and the launchers
// ------------------------------------------------------------------------------------------------
struct GrpPlan {
    bool packet;            // G % V == 0
    int pg_shift;           // log2(items per group) when that is a power of two, else -1
    int mode;               // GrpBwdMode
    int fwd_grid, bwd_grid;
    int64_t items_per_group;
    int64_t groups_per_wave;  // SCAN modes
};

inline int log2_exact(int64_t v) {
    if (v <= 0 || (v & (v - 1)) != 0) return -1;
    int k = 0;
    while ((int64_t{1} << k) < v) ++k;
    return k;
}

inline GrpPlan plan_group(int vec, int64_t n, int64_t G) {
    const DeviceInfo& dev = device_info();
    GrpPlan pl;
    pl.packet = G % vec == 0;
    pl.items_per_group = pl.packet ? G / vec : G;
    pl.pg_shift = log2_exact(pl.items_per_group);
    pl.mode = (pl.packet && pl.pg_shift >= 0) ? kP2 : (pl.packet ? kScanPacket : kScanElem);
    pl.groups_per_wave = 0;
    const int64_t fwd_round = static_cast<int64_t>(dev.cu_count) * kGrpFwdBlocksPerCU;
    const int64_t bwd_round = static_cast<int64_t>(dev.cu_count) * kGrpBwdBlocksPerCU;
    constexpr int kWaves = kBlock / 64;
    if (pl.packet) {
        const int64_t tiles = std::max<int64_t>(1, (n / vec + int64_t{kBlock} * kGrpUnroll - 1) / (int64_t{kBlock} * kGrpUnroll));
        pl.fwd_grid = static_cast<int>(std::min(tiles, fwd_round));
    } else {
        pl.fwd_grid = static_cast<int>(std::min(std::max<int64_t>(1, (n + kBlock - 1) / kBlock), fwd_round));
    }
    const int64_t n_items = pl.packet ? n / vec : n;
    if (pl.mode == kP2) {
        const int64_t unit = std::max<int64_t>(64 * kGrpUnroll, pl.items_per_group);
        const int64_t units = std::max<int64_t>(1, (n_items + unit - 1) / unit);
        pl.bwd_grid = static_cast<int>(std::min((units + kWaves - 1) / kWaves, bwd_round));
    } else {
        const int64_t n_groups = std::max<int64_t>(1, n / G);
        const int64_t want = std::min(n_groups, std::max<int64_t>(1, std::min(bwd_round * kWaves,
                                                                              (n_items + 64 * kGrpUnroll - 1) / (64 * kGrpUnroll))));
        pl.groups_per_wave = (n_groups + want - 1) / want;
        const int64_t waves = (n_groups + pl.groups_per_wave - 1) / pl.groups_per_wave;
        pl.bwd_grid = static_cast<int>((waves + kWaves - 1) / kWaves);
    }
    return pl;
}

template <typename IO, bool INIT, bool LEVELS>
static void launch_fwd_grp(const GrpPlan& pl, bool packet, const void* x, void* y, int8_t* levels, int bias, int aux_kind,
                           int64_t n, int64_t G, const void* scale, const void* shift, const Range<typename IO::arith>& r,
                           hipStream_t stream) {
    using T = typename IO::arith;
    const T* sc = static_cast<const T*>(scale);
    const T* sh = static_cast<const T*>(shift);
    if (packet) {
        hipLaunchKernelGGL((fwd_grp_kernel<IO, INIT, LEVELS, true>), dim3(pl.fwd_grid), dim3(kBlock), 0, stream, x, y, levels,
                           bias, aux_kind, n, G, pl.pg_shift, make_div(pl.items_per_group), sc, sh, r);
    } else {
        const int grid = static_cast<int>(std::min<int64_t>(std::max<int64_t>(1, (n + kBlock - 1) / kBlock),
                                                            static_cast<int64_t>(device_info().cu_count) * kGrpFwdBlocksPerCU));
        hipLaunchKernelGGL((fwd_grp_kernel<IO, INIT, LEVELS, false>), dim3(grid), dim3(kBlock), 0, stream, x, y, levels, bias,
                           aux_kind, n, G, -1, make_div(G), sc, sh, r);
    }
}

template <typename IO>
hipError_t forward_per_group(const void* x, void* y, int64_t n, int64_t G, const void* scale, const void* shift,
                             const lsq_params& p, const lsq_fwd_extras* ex, hipStream_t stream) {
    using T = typename IO::arith;
    const Range<T> r = make_range<T>(p);
    int8_t* levels = ex ? static_cast<int8_t*>(ex->levels) : nullptr;
    const int bias = ex ? ex->level_bias : 0;
    const int aux_kind = ex ? ex->aux_kind : 0;
    const GrpPlan pl = plan_group(IO::VEC, n, G);
    // the VEC level bytes of a packet are stored as one word: a levels buffer without that alignment takes the element form
    const bool packet = pl.packet && (!levels || (reinterpret_cast<uintptr_t>(levels) & (IO::VEC - 1)) == 0);
    if (p.init_mode) {
        if (levels) launch_fwd_grp<IO, true, true>(pl, packet, x, y, levels, bias, aux_kind, n, G, scale, shift, r, stream);
        else launch_fwd_grp<IO, true, false>(pl, packet, x, y, levels, bias, aux_kind, n, G, scale, shift, r, stream);
    } else {
        if (levels) launch_fwd_grp<IO, false, true>(pl, packet, x, y, levels, bias, aux_kind, n, G, scale, shift, r, stream);
        else launch_fwd_grp<IO, false, false>(pl, packet, x, y, levels, bias, aux_kind, n, G, scale, shift, r, stream);
    }
    return hipGetLastError();
}

template <typename IO, bool SYM, bool INIT, bool EVAL>
static void launch_bwd_grp(const GrpPlan& pl, const void* grad, const void* x, void* dx, void* ds, void* db, int64_t n,
                           int64_t G, const void* scale, const void* shift, const lsq_params& p, hipStream_t stream) {
    using T = typename IO::arith;
    const Range<T> r = make_range<T>(p);
    const int64_t n4s = p.numel_for_scaler > 0 ? p.numel_for_scaler : n;
    const T gs = grad_scaler_per_channel<T>(n4s, p.quant_max, n / G, p.use_grad_scaling != 0, p.grad_scaler);
    const T sym_term = static_cast<T>(0) * gs;
    const T* sc = static_cast<const T*>(scale);
    const T* sh = static_cast<const T*>(shift);
    T* dsT = static_cast<T*>(ds);
    T* dbT = static_cast<T*>(db);
#define LSQ_LAUNCH_BWD_GRP(M)                                                                                             \
    hipLaunchKernelGGL((bwd_grp_kernel<IO, SYM, INIT, EVAL, M>), dim3(pl.bwd_grid), dim3(kBlock), 0, stream, grad, x, dx, dsT, \
                       dbT, n, G, pl.pg_shift, make_div(pl.items_per_group), pl.groups_per_wave, sc, sh, r, gs, sym_term)
    if (pl.mode == kP2) LSQ_LAUNCH_BWD_GRP(kP2);
    else if (pl.mode == kScanPacket) LSQ_LAUNCH_BWD_GRP(kScanPacket);
    else LSQ_LAUNCH_BWD_GRP(kScanElem);
#undef LSQ_LAUNCH_BWD_GRP
}

template <typename IO>
hipError_t backward_per_group(const void* grad, const void* x, void* dx, void* ds, void* db, int64_t n, int64_t G,
                              const void* scale, const void* shift, const lsq_params& p, hipStream_t stream) {
    const GrpPlan pl = plan_group(IO::VEC, n, G);
#define LSQ_BWD_GRP_CASE(S, I, E) launch_bwd_grp<IO, S, I, E>(pl, grad, x, dx, ds, db, n, G, scale, shift, p, stream)
    const bool sym = p.sym != 0, init = p.init_mode != 0;
    if (p.eval_mode) {
        if (init) LSQ_BWD_GRP_CASE(false, true, true);
        else LSQ_BWD_GRP_CASE(false, false, true);
    } else if (sym) {
        if (init) LSQ_BWD_GRP_CASE(true, true, false);
        else LSQ_BWD_GRP_CASE(true, false, false);
    } else {
        if (init) LSQ_BWD_GRP_CASE(false, true, false);
        else LSQ_BWD_GRP_CASE(false, false, false);
    }
#undef LSQ_BWD_GRP_CASE
    return hipGetLastError();
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_group.h
// ------------------------------------------------------------------------------------------------
#include <cstdarg>
#include <cstdio>

#include "../../../include/lsq_hip_group.h"

namespace {

thread_local char g_group_error[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_group_error, sizeof(g_group_error), fmt, ap);
    va_end(ap);
    return code;
}

int hip_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return LSQ_OK;
    return fail(static_cast<int>(e), "%s: %s (%s)", what, hipGetErrorName(e), hipGetErrorString(e));
}

int io_vec(int dtype) { return dtype == LSQ_F32 ? 4 : dtype == LSQ_F64 ? 2 : 8; }
uintptr_t elem_bytes(int dtype) { return dtype == LSQ_F64 ? 8 : (dtype == LSQ_F32 ? 4 : 2); }
uintptr_t param_bytes(int dtype) { return dtype == LSQ_F64 ? 8 : 4; }
bool aligned_to(const void* a, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(a) & (bytes - 1)) == 0; }

int check_shape(int dtype, int64_t n, int64_t G, const char* what) {
    if (dtype < LSQ_F32 || dtype > LSQ_F16) return fail(LSQ_EINVAL, "%s: unknown dtype code %d", what, dtype);
    if (G <= 0) return fail(LSQ_EINVAL, "%s: group_size must be positive, got %lld", what, static_cast<long long>(G));
    if (n < 0) return fail(LSQ_EINVAL, "%s: negative element count %lld", what, static_cast<long long>(n));
    if (n % G != 0)
        return fail(LSQ_EINVAL, "%s: element count %lld is not a multiple of group_size %lld", what, static_cast<long long>(n),
                    static_cast<long long>(G));
    return LSQ_OK;
}

int check_params(const lsq_params* p, const char* what) {
    if (!p) return fail(LSQ_EINVAL, "%s: lsq_params pointer is NULL", what);
    if (p->quant_min > p->quant_max) return fail(LSQ_EINVAL, "%s: quant_min %d > quant_max %d", what, p->quant_min, p->quant_max);
    if (p->type_min > p->type_max) return fail(LSQ_EINVAL, "%s: type_min %d > type_max %d", what, p->type_min, p->type_max);
    return LSQ_OK;
}

}  // namespace

#define LSQ_GRP_DISPATCH_IO(dtype, CALL)                         \
    switch (dtype) {                                             \
        case LSQ_F32: { using IO = lsq::io_f32; CALL; } break;   \
        case LSQ_F64: { using IO = lsq::io_f64; CALL; } break;   \
        case LSQ_BF16: { using IO = lsq::io_bf16; CALL; } break; \
        default: { using IO = lsq::io_f16; CALL; } break;        \
    }

extern "C" {

int lsq_group_abi_version(void) { return LSQ_GROUP_ABI_VERSION; }

const char* lsq_group_last_error(void) { return g_group_error; }

int lsq_group_forward(int dtype, const void* x, void* y, int64_t n, int64_t group_size, const void* scale, const void* shift,
                      const lsq_params* p, const lsq_fwd_extras* extras, void* stream) {
    const char* what = "lsq_group_forward";
    if (int rc = check_shape(dtype, n, group_size, what)) return rc;
    if (int rc = check_params(p, what)) return rc;
    const void* levels = extras ? extras->levels : nullptr;
    if (!x || !scale || !shift || (!y && !levels)) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (levels && extras->aux_kind == 0) {
        const int lo = p->quant_min - extras->level_bias, hi = p->quant_max - extras->level_bias;
        if (!((lo >= -128 && hi <= 127) || (lo >= 0 && hi <= 255)))
            return fail(LSQ_EINVAL, "%s: levels: [quant_min, quant_max] - level_bias = [%d, %d] fits neither int8 nor uint8", what,
                        lo, hi);
    }
    if (!aligned_to(x, elem_bytes(dtype)) || (y && !aligned_to(y, elem_bytes(dtype))))
        return fail(LSQ_EINVAL, "%s: x and y must be element-aligned", what);
    if (!aligned_to(scale, param_bytes(dtype)) || !aligned_to(shift, param_bytes(dtype)))
        return fail(LSQ_EINVAL, "%s: scale and shift must be element-aligned", what);
    if (n == 0) return LSQ_OK;
    hipError_t e = hipSuccess;
    LSQ_GRP_DISPATCH_IO(dtype, e = lsq::forward_per_group<IO>(x, y, n, group_size, scale, shift, *p, extras,
                                                               static_cast<hipStream_t>(stream)));
    return hip_status(e, what);
}

int lsq_group_backward(int dtype, const void* grad, const void* x, void* dx, void* ds, void* db, int64_t n, int64_t group_size,
                       const void* scale, const void* shift, const lsq_params* p, void* stream) {
    const char* what = "lsq_group_backward";
    if (int rc = check_shape(dtype, n, group_size, what)) return rc;
    if (int rc = check_params(p, what)) return rc;
    if (!grad || !x || !dx || !ds || !db || !scale || !shift) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    const uintptr_t eb = elem_bytes(dtype), pb = param_bytes(dtype);
    if (!aligned_to(grad, eb) || !aligned_to(x, eb) || !aligned_to(dx, eb))
        return fail(LSQ_EINVAL, "%s: grad, x and dx must be element-aligned", what);
    if (!aligned_to(scale, pb) || !aligned_to(shift, pb) || !aligned_to(ds, pb) || !aligned_to(db, pb))
        return fail(LSQ_EINVAL, "%s: scale, shift, ds and db must be element-aligned", what);
    if (n == 0) return LSQ_OK;
    hipError_t e = hipSuccess;
    LSQ_GRP_DISPATCH_IO(dtype, e = lsq::backward_per_group<IO>(grad, x, dx, ds, db, n, group_size, scale, shift, *p,
                                                                static_cast<hipStream_t>(stream)));
    return hip_status(e, what);
}

int lsq_group_plan(int dtype, int64_t n, int64_t group_size, int32_t* out8) {
    const char* what = "lsq_group_plan";
    if (int rc = check_shape(dtype, n, group_size, what)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::GrpPlan pl = lsq::plan_group(io_vec(dtype), n, group_size);
    const int64_t ipg = pl.items_per_group;
    out8[0] = pl.fwd_grid;
    out8[1] = pl.bwd_grid;
    out8[2] = lsq::kBlock;
    out8[3] = pl.packet ? 1 : 0;
    out8[4] = static_cast<int32_t>(ipg < INT32_MAX ? ipg : INT32_MAX);
    out8[5] = pl.mode == lsq::kP2 ? 1 : 2;
    out8[6] = io_vec(dtype);
    out8[7] = 0;
    return LSQ_OK;
}

}  // extern "C"
