// lsq_per_group_multi.hip -- MANY group-wise quantizers in one launch each way: the kernels and launchers of the fused
// calls of include/lsq_hip_group.h (their C ABI is in lsq_per_group.hip).
//
// A QAT model with group-wise weights runs one lsq_group_forward / lsq_group_backward pair per layer and step.  Most of
// those tensors are small next to the chip: a ViT-B 768 x 768 fp32 weight at G = 128 gets 144 workgroups each way from
// plan_group, less than one per CU of a 256-CU part, so every call under-fills the chip and pays a whole launch.  Here
// the items of up to kGrpItems tensors share ONE grid:
//  * item i gets exactly the forward and backward workgroup counts plan_group gives its single call, and workgroup b of
//    the grid runs the kernel body (lsq_grp_body.hpp) as block b - first[i] of a grid of first[i + 1] - first[i]: the same walk,
//    the same d_scale / d_shift summation order, so the same bits as the single calls (by construction, not tolerance);
//  * the item table travels in the KERNEL ARGUMENTS, as in lsq_multi.hip: no device table to build, upload or keep
//    alive, nothing to synchronise, capturable in a HIP graph; the workgroup finds its item with a scalar scan of first[];
//  * the form (PACKET) and the backward reduction (MODE) are template parameters of the bodies, so the host launches the
//    items in classes of one reduction each -- P2, scan over packets, scan over elements -- the forward with the same
//    classes (its form follows from the reduction), so an item has one launch index in both directions.
// All indexing is 64-bit, as in the single-tensor kernels: one item may hold more than 2^31 elements.
#include "lsq_grp_body.hpp"

namespace lsq {

constexpr int kGrpItems = LSQ_GROUP_MULTI_ITEMS;

template <typename Item, typename T>
struct GrpMultiArgs {
    int32_t first[kGrpItems + 1];   // first[i] = workgroups before item i; first[count] and beyond = the grid size
    Range<T> r;
    Item item[kGrpItems];
};

// the kernel-argument segment is 4 KB, and the hidden arguments follow the explicit ones: keep 512 bytes for them
static_assert(sizeof(GrpMultiArgs<GrpBwdItem<double>, double>) <= 4096 - 512, "backward item table too big for the kernarg segment");
static_assert(sizeof(GrpMultiArgs<GrpFwdItem<double>, double>) <= 4096 - 512, "forward item table too big for the kernarg segment");
static_assert(sizeof(GrpMultiArgs<GrpBwdItem<float>, float>) <= 4096 - 512, "backward item table too big for the kernarg segment");

// item of workgroup b: the number of k >= 1 with first[k] <= b (entries past the last item hold the grid size, which no
// workgroup index reaches).  Branch-free, wave-uniform: scalar loads and compares only.
template <typename A>
__device__ __forceinline__ int grp_item_of(const A& a, int32_t b) {
    int i = 0;
#pragma unroll
    for (int k = 1; k < kGrpItems; ++k) i += (a.first[k] <= b) ? 1 : 0;
    return i;
}

// The kernels: the item's fields under the names the bodies use, then the body (lsq_grp_body.hpp), walked as block
// b - first[i] of the item's own grid of first[i + 1] - first[i] workgroups.
#define LSQ_GRP_BLOCK item_block
#define LSQ_GRP_GRID item_grid
template <typename IO, bool INIT, bool PACKET>
__global__ __launch_bounds__(kBlock) void fwd_grp_multi_kernel(const GrpMultiArgs<GrpFwdItem<typename IO::arith>, typename IO::arith> a) {
    using T = typename IO::arith;
    constexpr bool LEVELS = false;          // (no levels / inside-mask output in the fused call)
    const int32_t b = static_cast<int32_t>(blockIdx.x);
    const int i = __builtin_amdgcn_readfirstlane(grp_item_of(a, b));
    const GrpFwdItem<T>& it = a.item[i];
    const int64_t item_block = b - a.first[i], item_grid = a.first[i + 1] - a.first[i];
    const void* __restrict__ x = it.x;
    void* __restrict__ y = it.y;
    int8_t* const levels = nullptr;
    const int level_bias = 0, aux_kind = 0;
    const int64_t n = it.n, G = it.G;
    const int pg_shift = it.pg_shift;
    const DivU64 per_group = it.per_group;
    const T* __restrict__ scale = it.scale;
    const T* __restrict__ shift = it.shift;
    const Range<T> r = a.r;
    (void)G;
#include "lsq_grp_fwd_body.inc"
}

template <typename IO, bool SYM, bool INIT, bool EVAL, int MODE>
__global__ __launch_bounds__(kBlock) void bwd_grp_multi_kernel(const GrpMultiArgs<GrpBwdItem<typename IO::arith>, typename IO::arith> a) {
    using T = typename IO::arith;
    const int32_t b = static_cast<int32_t>(blockIdx.x);
    const int i = __builtin_amdgcn_readfirstlane(grp_item_of(a, b));
    const GrpBwdItem<T>& it = a.item[i];
    const int64_t item_block = b - a.first[i], item_grid = a.first[i + 1] - a.first[i];
    const void* __restrict__ grad = it.grad;
    const void* __restrict__ x = it.x;
    void* __restrict__ dx = it.dx;
    T* __restrict__ ds = it.ds;
    T* __restrict__ db = it.db;
    const int64_t n = it.n, G = it.G;
    const int pg_shift = it.pg_shift;
    const DivU64 per_group = it.per_group;
    const int64_t groups_per_wave = it.groups_per_wave;
    const T* __restrict__ scale = it.scale;
    const T* __restrict__ shift = it.shift;
    const Range<T> r = a.r;
    const T gs = it.gs, sym_term = it.sym_term;
#include "lsq_grp_bwd_body.inc"
}
#undef LSQ_GRP_BLOCK
#undef LSQ_GRP_GRID

// ------------------------------------------------------------------------------------------------
// host side: one rule for the launches and for lsq_group_multi_plan
// ------------------------------------------------------------------------------------------------
struct GrpLaunch {
    int mode;                       // GrpBwdMode of every item of the launch
    int count;
    int32_t index[kGrpItems];       // the items (indices into the caller's array), in the caller's order
    GrpPlan plan[kGrpItems];        // their single-call plans
};

// emit(launch) for every launch, in launch order: the reduction classes P2, scan over packets, scan over elements; in each
// class the items in the caller's order, kGrpItems per launch (and fewer if a grid would pass 2^31 - 1 workgroups)
template <typename F>
static void for_each_launch(int vec, const lsq_group_item* items, int32_t count, F&& emit) {
    for (int mode = kP2; mode <= kScanElem; ++mode) {
        GrpLaunch l;
        l.mode = mode;
        l.count = 0;
        int64_t fwd = 0, bwd = 0;
        for (int32_t i = 0; i < count; ++i) {
            if (items[i].n == 0) continue;
            const GrpPlan pl = plan_group(vec, items[i].n, items[i].group_size);
            if (pl.mode != mode) continue;
            if (l.count == kGrpItems || fwd + pl.fwd_grid > INT32_MAX || bwd + pl.bwd_grid > INT32_MAX) {
                emit(l);
                l.count = 0;
                fwd = bwd = 0;
            }
            l.index[l.count] = i;
            l.plan[l.count] = pl;
            ++l.count;
            fwd += pl.fwd_grid;
            bwd += pl.bwd_grid;
        }
        if (l.count > 0) emit(l);
    }
}

template <typename IO>
static hipError_t launch_fwd_multi(const GrpLaunch& l, const lsq_group_item* items, const lsq_params& p, hipStream_t stream) {
    using T = typename IO::arith;
    GrpMultiArgs<GrpFwdItem<T>, T> a;
    a.r = make_range<T>(p);
    int64_t blocks = 0;
    for (int k = 0; k < l.count; ++k) {
        const GrpPlan& pl = l.plan[k];
        a.first[k] = static_cast<int32_t>(blocks);
        a.item[k] = grp_fwd_item<T>(pl, items[l.index[k]]);
        blocks += pl.fwd_grid;
    }
    for (int k = l.count; k <= kGrpItems; ++k) a.first[k] = static_cast<int32_t>(blocks);
    for (int k = l.count; k < kGrpItems; ++k) a.item[k] = a.item[0];
    const dim3 grid(static_cast<unsigned>(blocks));
#define LSQ_FWD_GRP_MULTI(I, P) hipLaunchKernelGGL((fwd_grp_multi_kernel<IO, I, P>), grid, dim3(kBlock), 0, stream, a)
    const bool packet = l.mode != kScanElem;
    if (p.init_mode) { if (packet) LSQ_FWD_GRP_MULTI(true, true); else LSQ_FWD_GRP_MULTI(true, false); }
    else { if (packet) LSQ_FWD_GRP_MULTI(false, true); else LSQ_FWD_GRP_MULTI(false, false); }
#undef LSQ_FWD_GRP_MULTI
    return hipGetLastError();
}

template <typename IO, bool SYM, bool INIT, bool EVAL>
static void launch_bwd_multi_mode(int mode, const dim3& grid, const GrpMultiArgs<GrpBwdItem<typename IO::arith>, typename IO::arith>& a,
                                  hipStream_t stream) {
#define LSQ_BWD_GRP_MULTI(M) hipLaunchKernelGGL((bwd_grp_multi_kernel<IO, SYM, INIT, EVAL, M>), grid, dim3(kBlock), 0, stream, a)
    if (mode == kP2) LSQ_BWD_GRP_MULTI(kP2);
    else if (mode == kScanPacket) LSQ_BWD_GRP_MULTI(kScanPacket);
    else LSQ_BWD_GRP_MULTI(kScanElem);
#undef LSQ_BWD_GRP_MULTI
}

template <typename IO>
static hipError_t launch_bwd_multi(const GrpLaunch& l, const lsq_group_item* items, const lsq_params& p, hipStream_t stream) {
    using T = typename IO::arith;
    GrpMultiArgs<GrpBwdItem<T>, T> a;
    a.r = make_range<T>(p);
    int64_t blocks = 0;
    for (int k = 0; k < l.count; ++k) {
        const GrpPlan& pl = l.plan[k];
        a.first[k] = static_cast<int32_t>(blocks);
        a.item[k] = grp_bwd_item<T>(pl, items[l.index[k]], p);
        blocks += pl.bwd_grid;
    }
    for (int k = l.count; k <= kGrpItems; ++k) a.first[k] = static_cast<int32_t>(blocks);
    for (int k = l.count; k < kGrpItems; ++k) a.item[k] = a.item[0];
    const dim3 grid(static_cast<unsigned>(blocks));
    const bool sym = p.sym != 0, init = p.init_mode != 0;
    if (p.eval_mode) {
        if (init) launch_bwd_multi_mode<IO, false, true, true>(l.mode, grid, a, stream);
        else launch_bwd_multi_mode<IO, false, false, true>(l.mode, grid, a, stream);
    } else if (sym) {
        if (init) launch_bwd_multi_mode<IO, true, true, false>(l.mode, grid, a, stream);
        else launch_bwd_multi_mode<IO, true, false, false>(l.mode, grid, a, stream);
    } else {
        if (init) launch_bwd_multi_mode<IO, false, true, false>(l.mode, grid, a, stream);
        else launch_bwd_multi_mode<IO, false, false, false>(l.mode, grid, a, stream);
    }
    return hipGetLastError();
}

template <typename IO>
static hipError_t per_group_multi(bool backward, const lsq_group_item* items, int32_t count, const lsq_params& p,
                                  hipStream_t stream) {
    hipError_t e = hipSuccess;
    for_each_launch(IO::VEC, items, count, [&](const GrpLaunch& l) {
        if (e != hipSuccess) return;
        e = backward ? launch_bwd_multi<IO>(l, items, p, stream) : launch_fwd_multi<IO>(l, items, p, stream);
    });
    return e;
}

static hipError_t per_group_multi(bool backward, int dtype, const lsq_group_item* items, int32_t count, const lsq_params& p,
                                  hipStream_t stream) {
    switch (dtype) {
        case LSQ_F32: return per_group_multi<io_f32>(backward, items, count, p, stream);
        case LSQ_F64: return per_group_multi<io_f64>(backward, items, count, p, stream);
        case LSQ_BF16: return per_group_multi<io_bf16>(backward, items, count, p, stream);
        default: return per_group_multi<io_f16>(backward, items, count, p, stream);
    }
}

hipError_t forward_per_group_multi(int dtype, const lsq_group_item* items, int32_t count, const lsq_params& p,
                                   hipStream_t stream) {
    return per_group_multi(false, dtype, items, count, p, stream);
}

hipError_t backward_per_group_multi(int dtype, const lsq_group_item* items, int32_t count, const lsq_params& p,
                                    hipStream_t stream) {
    return per_group_multi(true, dtype, items, count, p, stream);
}

int32_t plan_group_multi(int vec, const lsq_group_item* items, int32_t count, int32_t* per_item3) {
    int32_t n_launch = 0;
    for_each_launch(vec, items, count, [&](const GrpLaunch& l) {
        for (int k = 0; k < l.count; ++k) {
            int32_t* o = per_item3 + 3 * l.index[k];
            o[0] = n_launch;
            o[1] = l.plan[k].fwd_grid;
            o[2] = l.plan[k].bwd_grid;
        }
        ++n_launch;
    });
    return n_launch;
}

}  // namespace lsq
