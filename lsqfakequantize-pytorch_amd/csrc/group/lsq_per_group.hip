// lsq_per_group.hip -- group-wise LSQ on gfx950 (include/lsq_hip_group.h): one scale / shift per run of G consecutive
// elements, the per-channel arithmetic of lsq_math.hpp on the [1, n / G, G] view.  The single-tensor kernels and the C ABI
// of the whole library; the fused calls' kernels are in lsq_per_group_multi.hip.
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
#include "lsq_grp_body.hpp"
#include "../lsq_companion_abi.hpp"

namespace lsq {

// the kernels: the bodies of lsq_grp_fwd_body.inc / lsq_grp_bwd_body.inc over the whole grid
#define LSQ_GRP_BLOCK static_cast<int64_t>(blockIdx.x)
#define LSQ_GRP_GRID static_cast<int64_t>(gridDim.x)
template <typename IO, bool INIT, bool LEVELS, bool PACKET>
__global__ __launch_bounds__(kBlock) void fwd_grp_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                         int8_t* __restrict__ levels, int level_bias, int aux_kind,
                                                         int64_t n, int64_t G, int pg_shift, DivU64 per_group,
                                                         const typename IO::arith* __restrict__ scale,
                                                         const typename IO::arith* __restrict__ shift,
                                                         Range<typename IO::arith> r) {
#include "lsq_grp_fwd_body.inc"
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
#include "lsq_grp_bwd_body.inc"
}
#undef LSQ_GRP_BLOCK
#undef LSQ_GRP_GRID

// ------------------------------------------------------------------------------------------------
// host side: the launchers (the plan is plan_group, the kernel arguments grp_fwd_item / grp_bwd_item: lsq_grp_body.hpp)
// ------------------------------------------------------------------------------------------------
template <typename IO, bool INIT, bool LEVELS>
static void launch_fwd_grp(const GrpPlan& pl, const GrpFwdItem<typename IO::arith>& it, int8_t* levels, int bias,
                           int aux_kind, const Range<typename IO::arith>& r, hipStream_t stream) {
#define LSQ_LAUNCH_FWD_GRP(P)                                                                                              \
    hipLaunchKernelGGL((fwd_grp_kernel<IO, INIT, LEVELS, P>), dim3(pl.fwd_grid), dim3(kBlock), 0, stream, it.x, it.y, levels, \
                       bias, aux_kind, it.n, it.G, it.pg_shift, it.per_group, it.scale, it.shift, r)
    if (pl.packet) LSQ_LAUNCH_FWD_GRP(true);
    else LSQ_LAUNCH_FWD_GRP(false);
#undef LSQ_LAUNCH_FWD_GRP
}

template <typename IO>
static hipError_t forward_per_group(const lsq_group_item& item, const lsq_params& p, const lsq_fwd_extras* ex,
                                    hipStream_t stream) {
    using T = typename IO::arith;
    const Range<T> r = make_range<T>(p);
    int8_t* levels = ex ? static_cast<int8_t*>(ex->levels) : nullptr;
    const int bias = ex ? ex->level_bias : 0;
    const int aux_kind = ex ? ex->aux_kind : 0;
    GrpPlan pl = plan_group(IO::VEC, item.n, item.group_size);
    // the VEC level bytes of a packet are stored as one word: a levels buffer without that alignment takes the element form
    if (pl.packet && levels && (reinterpret_cast<uintptr_t>(levels) & (IO::VEC - 1)) != 0) {
        pl.packet = false;
        pl.fwd_grid = grp_elem_fwd_grid(item.n);
    }
    const GrpFwdItem<T> it = grp_fwd_item<T>(pl, item);
    if (p.init_mode) {
        if (levels) launch_fwd_grp<IO, true, true>(pl, it, levels, bias, aux_kind, r, stream);
        else launch_fwd_grp<IO, true, false>(pl, it, levels, bias, aux_kind, r, stream);
    } else {
        if (levels) launch_fwd_grp<IO, false, true>(pl, it, levels, bias, aux_kind, r, stream);
        else launch_fwd_grp<IO, false, false>(pl, it, levels, bias, aux_kind, r, stream);
    }
    return hipGetLastError();
}

template <typename IO, bool SYM, bool INIT, bool EVAL>
static void launch_bwd_grp(const GrpPlan& pl, const GrpBwdItem<typename IO::arith>& it, const Range<typename IO::arith>& r,
                           hipStream_t stream) {
#define LSQ_LAUNCH_BWD_GRP(M)                                                                                             \
    hipLaunchKernelGGL((bwd_grp_kernel<IO, SYM, INIT, EVAL, M>), dim3(pl.bwd_grid), dim3(kBlock), 0, stream, it.grad, it.x, \
                       it.dx, it.ds, it.db, it.n, it.G, it.pg_shift, it.per_group, it.groups_per_wave, it.scale, it.shift, r, \
                       it.gs, it.sym_term)
    if (pl.mode == kP2) LSQ_LAUNCH_BWD_GRP(kP2);
    else if (pl.mode == kScanPacket) LSQ_LAUNCH_BWD_GRP(kScanPacket);
    else LSQ_LAUNCH_BWD_GRP(kScanElem);
#undef LSQ_LAUNCH_BWD_GRP
}

template <typename IO>
static hipError_t backward_per_group(const lsq_group_item& item, const lsq_params& p, hipStream_t stream) {
    using T = typename IO::arith;
    const Range<T> r = make_range<T>(p);
    const GrpPlan pl = plan_group(IO::VEC, item.n, item.group_size);
    const GrpBwdItem<T> it = grp_bwd_item<T>(pl, item, p);
#define LSQ_BWD_GRP_CASE(S, I, E) launch_bwd_grp<IO, S, I, E>(pl, it, r, stream)
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
// the C ABI of include/lsq_hip_group.h, all eight entry points: validation, dtype dispatch, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// LSQ_EINVAL, "what: message" for a single call (item < 0), "what: item <i>: message" for an item of a fused call
int fail_item(const char* what, int item, const char* fmt, ...) {
    char msg[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    if (item < 0) return fail(LSQ_EINVAL, "%s: %s", what, msg);
    return fail(LSQ_EINVAL, "%s: item %d: %s", what, item, msg);
}

int check_dtype(int dtype, const char* what) {
    if (dtype < LSQ_F32 || dtype > LSQ_F16) return fail(LSQ_EINVAL, "%s: unknown dtype code %d", what, dtype);
    return LSQ_OK;
}

// a fused call has no numel_for_scaler: its items are whole tensors
int check_params(const lsq_params* p, bool fused, const char* what) {
    if (!p) return fail(LSQ_EINVAL, "%s: lsq_params pointer is NULL", what);
    if (p->quant_min > p->quant_max) return fail(LSQ_EINVAL, "%s: quant_min %d > quant_max %d", what, p->quant_min, p->quant_max);
    if (p->type_min > p->type_max) return fail(LSQ_EINVAL, "%s: type_min %d > type_max %d", what, p->type_min, p->type_max);
    if (fused && p->numel_for_scaler != 0)
        return fail(LSQ_EINVAL, "%s: numel_for_scaler must be 0 (there is no sharded group op), got %lld", what,
                    static_cast<long long>(p->numel_for_scaler));
    return LSQ_OK;
}

enum Use { kSizes, kForward, kBackward };

// one tensor's sizes and, for a launch (kForward / kBackward), the buffers that direction uses; y_optional: a single
// forward with a levels output, whose y may be NULL
int check_item(int dtype, const lsq_group_item& it, Use use, const char* what, int item, bool y_optional = false) {
    const long long n = it.n, G = it.group_size;
    if (G <= 0) return fail_item(what, item, "group_size must be positive, got %lld", G);
    if (n < 0) return fail_item(what, item, "negative element count %lld", n);
    if (n % G != 0) return fail_item(what, item, "element count %lld is not a multiple of group_size %lld", n, G);
    if (use == kSizes) return LSQ_OK;
    const uintptr_t eb = elem_bytes(dtype), pb = param_bytes(dtype);
    if (use == kForward) {
        if (!it.x || !it.scale || !it.shift || (!it.y && !y_optional)) return fail_item(what, item, "NULL buffer");
        if (!aligned_to(it.x, eb) || (it.y && !aligned_to(it.y, eb)))
            return fail_item(what, item, "x and y must be element-aligned");
    } else {
        if (!it.grad || !it.x || !it.dx || !it.ds || !it.db || !it.scale || !it.shift) return fail_item(what, item, "NULL buffer");
        if (!aligned_to(it.grad, eb) || !aligned_to(it.x, eb) || !aligned_to(it.dx, eb))
            return fail_item(what, item, "grad, x and dx must be element-aligned");
        if (!aligned_to(it.ds, pb) || !aligned_to(it.db, pb)) return fail_item(what, item, "ds and db must be element-aligned");
    }
    if (!aligned_to(it.scale, pb) || !aligned_to(it.shift, pb))
        return fail_item(what, item, "scale and shift must be element-aligned");
    return LSQ_OK;
}

// a fused call's dtype, lsq_params (unless use == kSizes) and list, every item before anything is enqueued; the buffers of
// an item with n == 0 are not read
int check_items(int dtype, const lsq_group_item* items, int32_t count, const lsq_params* p, Use use, const char* what) {
    if (int rc = check_dtype(dtype, what)) return rc;
    if (count < 0) return fail(LSQ_EINVAL, "%s: negative item count %d", what, count);
    if (count > 0 && !items) return fail(LSQ_EINVAL, "%s: items is NULL", what);
    if (use != kSizes)
        if (int rc = check_params(p, true, what)) return rc;
    for (int32_t i = 0; i < count; ++i)
        if (int rc = check_item(dtype, items[i], items[i].n == 0 ? kSizes : use, what, i)) return rc;
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

const char* lsq_group_last_error(void) { return g_last_error; }

int lsq_group_forward(int dtype, const void* x, void* y, int64_t n, int64_t group_size, const void* scale, const void* shift,
                      const lsq_params* p, const lsq_fwd_extras* extras, void* stream) {
    const char* what = "lsq_group_forward";
    const void* levels = extras ? extras->levels : nullptr;
    const lsq_group_item it{x, nullptr, y, nullptr, scale, shift, nullptr, nullptr, n, group_size};
    if (int rc = check_dtype(dtype, what)) return rc;
    if (int rc = check_params(p, false, what)) return rc;
    if (int rc = check_item(dtype, it, kForward, what, -1, levels != nullptr)) return rc;
    if (levels && extras->aux_kind == 0) {
        const int lo = p->quant_min - extras->level_bias, hi = p->quant_max - extras->level_bias;
        if (!((lo >= -128 && hi <= 127) || (lo >= 0 && hi <= 255)))
            return fail(LSQ_EINVAL, "%s: levels: [quant_min, quant_max] - level_bias = [%d, %d] fits neither int8 nor uint8", what,
                        lo, hi);
    }
    if (n == 0) return LSQ_OK;
    hipError_t e = hipSuccess;
    LSQ_GRP_DISPATCH_IO(dtype, e = lsq::forward_per_group<IO>(it, *p, extras, static_cast<hipStream_t>(stream)));
    return hip_status(e, what);
}

int lsq_group_backward(int dtype, const void* grad, const void* x, void* dx, void* ds, void* db, int64_t n, int64_t group_size,
                       const void* scale, const void* shift, const lsq_params* p, void* stream) {
    const char* what = "lsq_group_backward";
    const lsq_group_item it{x, grad, nullptr, dx, scale, shift, ds, db, n, group_size};
    if (int rc = check_dtype(dtype, what)) return rc;
    if (int rc = check_params(p, false, what)) return rc;
    if (int rc = check_item(dtype, it, kBackward, what, -1)) return rc;
    if (n == 0) return LSQ_OK;
    hipError_t e = hipSuccess;
    LSQ_GRP_DISPATCH_IO(dtype, e = lsq::backward_per_group<IO>(it, *p, static_cast<hipStream_t>(stream)));
    return hip_status(e, what);
}

int lsq_group_plan(int dtype, int64_t n, int64_t group_size, int32_t* out8) {
    const char* what = "lsq_group_plan";
    const lsq_group_item it{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n, group_size};
    if (int rc = check_dtype(dtype, what)) return rc;
    if (int rc = check_item(dtype, it, kSizes, what, -1)) return rc;
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

int lsq_group_multi_forward(int dtype, const lsq_group_item* items, int32_t count, const lsq_params* p, void* stream) {
    const char* what = "lsq_group_multi_forward";
    if (int rc = check_items(dtype, items, count, p, kForward, what)) return rc;
    return hip_status(lsq::forward_per_group_multi(dtype, items, count, *p, static_cast<hipStream_t>(stream)), what);
}

int lsq_group_multi_backward(int dtype, const lsq_group_item* items, int32_t count, const lsq_params* p, void* stream) {
    const char* what = "lsq_group_multi_backward";
    if (int rc = check_items(dtype, items, count, p, kBackward, what)) return rc;
    return hip_status(lsq::backward_per_group_multi(dtype, items, count, *p, static_cast<hipStream_t>(stream)), what);
}

int lsq_group_multi_plan(int dtype, const lsq_group_item* items, int32_t count, int32_t* per_item3, int32_t* launches) {
    const char* what = "lsq_group_multi_plan";
    if (int rc = check_items(dtype, items, count, nullptr, kSizes, what)) return rc;
    if ((count > 0 && !per_item3) || !launches) return fail(LSQ_EINVAL, "%s: NULL output", what);
    for (int32_t i = 0; i < count; ++i) {
        per_item3[3 * i] = -1;
        per_item3[3 * i + 1] = 0;
        per_item3[3 * i + 2] = 0;
    }
    *launches = lsq::plan_group_multi(io_vec(dtype), items, count, per_item3);
    return LSQ_OK;
}

}  // extern "C"
