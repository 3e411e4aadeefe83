// lsq_per_group_multi.hip -- MANY group-wise quantizers in one launch each way (include/lsq_hip_group_multi.h,
// liblsq_hip_group_multi.so).
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

#include "../../../include/lsq_hip_group_multi.h"

namespace lsq {

constexpr int kGrpItems = LSQ_GROUP_MULTI_ITEMS;

template <typename T>
struct GrpFwdItem {     // one tensor of a forward launch (kernel-argument image)
    const void* x;
    void* y;
    const T* scale;
    const T* shift;
    int64_t n, G;
    DivU64 per_group;   // (as the single launch: packets per group in the packet form, G in the element form)
    int pg_shift;
};

template <typename T>
struct GrpBwdItem {     // one tensor of a backward launch
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
    T gs;               // the item's own gradient scaler (n, quant_max, n / G), as in its single call
    T sym_term;
};

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
        const lsq_group_item& s = items[l.index[k]];
        const GrpPlan& pl = l.plan[k];
        GrpFwdItem<T>& d = a.item[k];
        a.first[k] = static_cast<int32_t>(blocks);
        d.x = s.x;
        d.y = s.y;
        d.scale = static_cast<const T*>(s.scale);
        d.shift = static_cast<const T*>(s.shift);
        d.n = s.n;
        d.G = s.group_size;
        d.pg_shift = pl.packet ? pl.pg_shift : -1;               // (launch_fwd_grp's arguments)
        d.per_group = make_div(pl.packet ? pl.items_per_group : s.group_size);
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
        const lsq_group_item& s = items[l.index[k]];
        const GrpPlan& pl = l.plan[k];
        GrpBwdItem<T>& d = a.item[k];
        a.first[k] = static_cast<int32_t>(blocks);
        d.grad = s.grad;
        d.x = s.x;
        d.dx = s.dx;
        d.scale = static_cast<const T*>(s.scale);
        d.shift = static_cast<const T*>(s.shift);
        d.ds = static_cast<T*>(s.ds);
        d.db = static_cast<T*>(s.db);
        d.n = s.n;
        d.G = s.group_size;
        d.pg_shift = pl.pg_shift;                                  // (launch_bwd_grp's arguments)
        d.per_group = make_div(pl.items_per_group);
        d.groups_per_wave = pl.groups_per_wave;
        d.gs = grad_scaler_per_channel<T>(s.n, p.quant_max, s.n / s.group_size, p.use_grad_scaling != 0, p.grad_scaler);
        d.sym_term = static_cast<T>(0) * d.gs;
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
hipError_t per_group_multi(bool backward, const lsq_group_item* items, int32_t count, const lsq_params& p, hipStream_t stream) {
    hipError_t e = hipSuccess;
    for_each_launch(IO::VEC, items, count, [&](const GrpLaunch& l) {
        if (e != hipSuccess) return;
        e = backward ? launch_bwd_multi<IO>(l, items, p, stream) : launch_fwd_multi<IO>(l, items, p, stream);
    });
    return e;
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_group_multi.h
// ------------------------------------------------------------------------------------------------
#include <cstdarg>
#include <cstdio>

namespace {

thread_local char g_multi_error[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_multi_error, sizeof(g_multi_error), fmt, ap);
    va_end(ap);
    return code;
}

int io_vec(int dtype) { return dtype == LSQ_F32 ? 4 : dtype == LSQ_F64 ? 2 : 8; }
uintptr_t elem_bytes(int dtype) { return dtype == LSQ_F64 ? 8 : (dtype == LSQ_F32 ? 4 : 2); }
uintptr_t param_bytes(int dtype) { return dtype == LSQ_F64 ? 8 : 4; }
bool aligned_to(const void* a, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(a) & (bytes - 1)) == 0; }

// dtype, count, the items' sizes -- and, for a launch (dir 0 = forward, 1 = backward), their buffers and lsq_params
int check_items(int dtype, const lsq_group_item* items, int32_t count, const lsq_params* p, int dir, const char* what) {
    if (dtype < LSQ_F32 || dtype > LSQ_F16) return fail(LSQ_EINVAL, "%s: unknown dtype code %d", what, dtype);
    if (count < 0) return fail(LSQ_EINVAL, "%s: negative item count %d", what, count);
    if (count > 0 && !items) return fail(LSQ_EINVAL, "%s: items is NULL", what);
    if (dir >= 0) {
        if (!p) return fail(LSQ_EINVAL, "%s: lsq_params pointer is NULL", what);
        if (p->quant_min > p->quant_max) return fail(LSQ_EINVAL, "%s: quant_min %d > quant_max %d", what, p->quant_min, p->quant_max);
        if (p->type_min > p->type_max) return fail(LSQ_EINVAL, "%s: type_min %d > type_max %d", what, p->type_min, p->type_max);
        if (p->numel_for_scaler != 0)
            return fail(LSQ_EINVAL, "%s: numel_for_scaler must be 0 (there is no sharded group op), got %lld", what,
                        static_cast<long long>(p->numel_for_scaler));
    }
    const uintptr_t eb = elem_bytes(dtype), pb = param_bytes(dtype);
    for (int32_t i = 0; i < count; ++i) {
        const lsq_group_item& it = items[i];
        const long long n = it.n, G = it.group_size;
        if (G <= 0) return fail(LSQ_EINVAL, "%s: item %d: group_size must be positive, got %lld", what, i, G);
        if (n < 0) return fail(LSQ_EINVAL, "%s: item %d: negative element count %lld", what, i, n);
        if (n % G != 0)
            return fail(LSQ_EINVAL, "%s: item %d: element count %lld is not a multiple of group_size %lld", what, i, n, G);
        if (dir < 0 || n == 0) continue;
        if (dir == 0) {
            if (!it.x || !it.y || !it.scale || !it.shift) return fail(LSQ_EINVAL, "%s: item %d: NULL buffer", what, i);
            if (!aligned_to(it.x, eb) || !aligned_to(it.y, eb))
                return fail(LSQ_EINVAL, "%s: item %d: x and y must be element-aligned", what, i);
        } else {
            if (!it.grad || !it.x || !it.dx || !it.ds || !it.db || !it.scale || !it.shift)
                return fail(LSQ_EINVAL, "%s: item %d: NULL buffer", what, i);
            if (!aligned_to(it.grad, eb) || !aligned_to(it.x, eb) || !aligned_to(it.dx, eb))
                return fail(LSQ_EINVAL, "%s: item %d: grad, x and dx must be element-aligned", what, i);
            if (!aligned_to(it.ds, pb) || !aligned_to(it.db, pb))
                return fail(LSQ_EINVAL, "%s: item %d: ds and db must be element-aligned", what, i);
        }
        if (!aligned_to(it.scale, pb) || !aligned_to(it.shift, pb))
            return fail(LSQ_EINVAL, "%s: item %d: scale and shift must be element-aligned", what, i);
    }
    return LSQ_OK;
}

int run(bool backward, int dtype, const lsq_group_item* items, int32_t count, const lsq_params* p, void* stream) {
    const char* what = backward ? "lsq_group_multi_backward" : "lsq_group_multi_forward";
    if (int rc = check_items(dtype, items, count, p, backward ? 1 : 0, what)) return rc;
    hipError_t e = hipSuccess;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case LSQ_F32: e = lsq::per_group_multi<lsq::io_f32>(backward, items, count, *p, s); break;
        case LSQ_F64: e = lsq::per_group_multi<lsq::io_f64>(backward, items, count, *p, s); break;
        case LSQ_BF16: e = lsq::per_group_multi<lsq::io_bf16>(backward, items, count, *p, s); break;
        default: e = lsq::per_group_multi<lsq::io_f16>(backward, items, count, *p, s); break;
    }
    if (e == hipSuccess) return LSQ_OK;
    return fail(static_cast<int>(e), "%s: %s (%s)", what, hipGetErrorName(e), hipGetErrorString(e));
}

}  // namespace

extern "C" {

int lsq_group_multi_abi_version(void) { return LSQ_GROUP_MULTI_ABI_VERSION; }

const char* lsq_group_multi_last_error(void) { return g_multi_error; }

int lsq_group_multi_forward(int dtype, const lsq_group_item* items, int32_t count, const lsq_params* p, void* stream) {
    return run(false, dtype, items, count, p, stream);
}

int lsq_group_multi_backward(int dtype, const lsq_group_item* items, int32_t count, const lsq_params* p, void* stream) {
    return run(true, dtype, items, count, p, stream);
}

int lsq_group_multi_plan(int dtype, const lsq_group_item* items, int32_t count, int32_t* per_item3, int32_t* launches) {
    const char* what = "lsq_group_multi_plan";
    if (int rc = check_items(dtype, items, count, nullptr, -1, what)) return rc;
    if ((count > 0 && !per_item3) || !launches) return fail(LSQ_EINVAL, "%s: NULL output", what);
    for (int32_t i = 0; i < count; ++i) {
        per_item3[3 * i] = -1;
        per_item3[3 * i + 1] = 0;
        per_item3[3 * i + 2] = 0;
    }
    int32_t n_launch = 0;
    lsq::for_each_launch(io_vec(dtype), items, count, [&](const lsq::GrpLaunch& l) {
        for (int k = 0; k < l.count; ++k) {
            int32_t* o = per_item3 + 3 * l.index[k];
            o[0] = n_launch;
            o[1] = l.plan[k].fwd_grid;
            o[2] = l.plan[k].bwd_grid;
        }
        ++n_launch;
    });
    *launches = n_launch;
    return LSQ_OK;
}

}  // extern "C"
