// lsq_grp_body.hpp -- what the two translation units of liblsq_hip_group.so share: the single-tensor kernels
// (lsq_per_group.hip, which also holds the C ABI) and the multi-tensor ones (lsq_per_group_multi.hip).  lsq_per_group.hip
// describes the forms and the reductions.
//  * the device helpers below, and on the host the launch plan (plan_group), the kernel arguments an item gets from its
//    plan (grp_fwd_item / grp_bwd_item) and the entry points of the multi-tensor translation unit;
//  * the kernel bodies, lsq_grp_fwd_body.inc and lsq_grp_bwd_body.inc: statement fragments that a kernel #includes as its
//    body, with LSQ_GRP_BLOCK / LSQ_GRP_GRID defined as the workgroup's index and the number of workgroups that walk the
//    tensor -- blockIdx.x / gridDim.x in a single-tensor kernel, the index within the item and the item's own grid in a
//    multi-tensor one.  An item therefore runs the same walk, and sums d_scale / d_shift in the same order, as its single
//    call.  (Fragments, not inlined __device__ functions: inlining a body that returns early lays out the kernel's blocks
//    differently, so the single-tensor kernels would no longer compile to the instructions they were measured with.)
#pragma once

#include "../lsq_kernels.hpp"
#include "../../../include/lsq_hip_group.h"

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

// ------------------------------------------------------------------------------------------------
// host side: the plan -- one rule for the single and the fused launches, lsq_group_plan and lsq_group_multi_plan
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

// the forward grid of the element form (one element per lane)
inline int grp_elem_fwd_grid(int64_t n) {
    const int64_t fwd_round = static_cast<int64_t>(device_info().cu_count) * kGrpFwdBlocksPerCU;
    return static_cast<int>(std::min(std::max<int64_t>(1, (n + kBlock - 1) / kBlock), fwd_round));
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
        pl.fwd_grid = grp_elem_fwd_grid(n);
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


// The kernel arguments of one tensor, from its plan: the single-tensor launchers pass the fields to fwd_grp_kernel /
// bwd_grp_kernel, the multi-tensor launchers put the structs in their kernel-argument tables -- so a fused item runs with
// exactly the arguments of its single call.
template <typename T>
struct GrpFwdItem {
    const void* x;
    void* y;
    const T* scale;
    const T* shift;
    int64_t n, G;
    DivU64 per_group;   // packets per group in the packet form, G in the element form
    int pg_shift;
};

template <typename T>
struct GrpBwdItem {
    const void* grad;
    const void* x;
    void* dx;
    const T* scale;
    const T* shift;
    T* ds;
    T* db;
    int64_t n, G;
    DivU64 per_group;
    int64_t groups_per_wave;
    int pg_shift;
    T gs;               // the gradient scaler (numel_for_scaler or n, quant_max, n / G)
    T sym_term;
};

template <typename T>
inline GrpFwdItem<T> grp_fwd_item(const GrpPlan& pl, const lsq_group_item& s) {
    GrpFwdItem<T> d;
    d.x = s.x;
    d.y = s.y;
    d.scale = static_cast<const T*>(s.scale);
    d.shift = static_cast<const T*>(s.shift);
    d.n = s.n;
    d.G = s.group_size;
    d.per_group = make_div(pl.packet ? pl.items_per_group : s.group_size);
    d.pg_shift = pl.packet ? pl.pg_shift : -1;
    return d;
}

template <typename T>
inline GrpBwdItem<T> grp_bwd_item(const GrpPlan& pl, const lsq_group_item& s, const lsq_params& p) {
    GrpBwdItem<T> d;
    d.grad = s.grad;
    d.x = s.x;
    d.dx = s.dx;
    d.scale = static_cast<const T*>(s.scale);
    d.shift = static_cast<const T*>(s.shift);
    d.ds = static_cast<T*>(s.ds);
    d.db = static_cast<T*>(s.db);
    d.n = s.n;
    d.G = s.group_size;
    d.per_group = make_div(pl.items_per_group);
    d.groups_per_wave = pl.groups_per_wave;
    d.pg_shift = pl.pg_shift;
    const int64_t n4s = p.numel_for_scaler > 0 ? p.numel_for_scaler : s.n;
    d.gs = grad_scaler_per_channel<T>(n4s, p.quant_max, s.n / s.group_size, p.use_grad_scaling != 0, p.grad_scaler);
    d.sym_term = static_cast<T>(0) * d.gs;
    return d;
}

// lsq_per_group_multi.hip, for the C ABI (which has validated the items): the fused launches of one direction, and the
// plan walk of lsq_group_multi_plan (per_item3 filled for the items with n > 0; returns the launches per direction)
hipError_t forward_per_group_multi(int dtype, const lsq_group_item* items, int32_t count, const lsq_params& p,
                                   hipStream_t stream);
hipError_t backward_per_group_multi(int dtype, const lsq_group_item* items, int32_t count, const lsq_params& p,
                                    hipStream_t stream);
int32_t plan_group_multi(int vec, const lsq_group_item* items, int32_t count, int32_t* per_item3);

}  // namespace lsq
