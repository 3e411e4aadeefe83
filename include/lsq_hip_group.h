/* include/lsq_hip_group.h -- group-wise LSQ fake quantization on gfx950: one learned scale and shift per run of
 * `group_size` (G) consecutive elements, one tensor per call or many tensors in one launch each way.
 *
 * Exported by `liblsq_hip_group.so` (built from lsqfakequantize-pytorch_amd/csrc/group/ for gfx950), a companion of
 * `liblsq_hip.so`: the main library's ABI (include/lsq_hip.h, version 6) is unchanged, this header only borrows its
 * structs (lsq_params, lsq_fwd_extras), dtype codes and status codes.  Same contract as lsq_hip.h: caller-owned device
 * buffers, kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no
 * synchronisation, no environment variables, no mutable global state, 0 / negative LSQ_E* / positive hipError_t returns,
 * never throws; lsq_group_last_error() describes the calling thread's last failure, whichever entry point it came from.
 *
 * Layout: x, y, grad, dx are `n` dense elements; group j is elements [j*G, (j+1)*G), so n must be a multiple of G.
 * scale, shift, ds, db hold n / G values (float for F32 | BF16 | F16 storage, double for F64).  Every op is, value for
 * value, the per-channel op of lsq_hip.h on the [outer = 1, C = n / G, inner = G] view -- the same per-group constants
 * (fmax(eps, |s|), correctly rounded 1 / s, the clamped zero point) and the per-channel gradient scaler
 * grad_scaler / sqrt(numel * quant_max / (n / G)) -- with d_scale / d_shift summed in fp64 in a fixed order: no
 * workspace, bit-identical from launch to launch.  Pointers must be element-aligned (16-byte alignment is not needed).
 *
 * The fused calls (lsq_group_multi_*) take a list of items, each one tensor of this layout; G may differ from item to
 * item.  Results are, bit for bit, those of one lsq_group_forward / lsq_group_backward call per item with the same
 * lsq_params: each item is walked by exactly the workgroups its own call would launch, so its d_scale / d_shift are
 * summed in the same order.  The gradient scaler is per item: grad_scaler / sqrt(n * quant_max / (n / G)).  The items
 * of one call are launched in classes of one backward reduction each (the `reduction` of lsq_group_plan: 16-byte packets
 * with a power-of-two or another packet count per group, or one element per lane), at most LSQ_GROUP_MULTI_ITEMS items
 * per launch: one launch each way when every G is the same multiple of the packet width.  Every item is validated before
 * anything is enqueued: a bad item fails the whole call with LSQ_EINVAL and its index in the message.  Items with
 * n == 0 take no part (their pointers are not read).  p->numel_for_scaler must be 0 (there is no sharded group op).  The
 * inside-mask and levels outputs of lsq_group_forward are not offered there.
 */
#ifndef LSQ_HIP_GROUP_H_
#define LSQ_HIP_GROUP_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_GROUP_ABI_VERSION 2
#define LSQ_GROUP_MULTI_ITEMS 28   /* items per fused launch */

/* One tensor of a fused call.  Forward reads x, scale, shift and writes y; backward reads grad, x, scale, shift and writes
 * dx, ds, db.  Pointers the direction does not use are ignored. */
typedef struct {
    const void* x;
    const void* grad;
    void* y;
    void* dx;
    const void* scale;
    const void* shift;
    void* ds;
    void* db;
    int64_t n;
    int64_t group_size;
} lsq_group_item;

/* LSQ_GROUP_ABI_VERSION the library was built with. */
int lsq_group_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_group_last_error(void);

/* Forward (lsq_hip_forward_per_channel on [1, n / G, G]).  `extras` as in lsq_hip.h: optional one byte per element
 * (aux_kind 0 = integer levels minus level_bias, 1 = inside mask); with extras->levels set `y` may be NULL. */
int lsq_group_forward(int dtype, const void* x, void* y, int64_t n, int64_t group_size, const void* scale,
                      const void* shift, const lsq_params* p, const lsq_fwd_extras* extras, void* stream);

/* Fused backward: dx and the n / G values of d_scale / d_shift, in ONE launch (a wave owns whole groups and finishes
 * their sums in registers: no workspace argument, because none is needed).  eval_mode: ds = db = 0. */
int lsq_group_backward(int dtype, const void* grad, const void* x, void* dx, void* ds, void* db, int64_t n,
                       int64_t group_size, const void* scale, const void* shift, const lsq_params* p, void* stream);

/* Host only, nothing is launched: the launches the two ops make for (dtype, n, group_size) on the current device with
 * element-aligned buffers.  out8 = [forward grid, backward grid, workgroup size, form (1 = 16-byte packets, one group per
 * packet; 0 = per element), lanes per group (packets resp. elements of one group), backward reduction (1 = power-of-two
 * butterfly, 2 = keyed segmented scan), elements per packet, 0]. */
int lsq_group_plan(int dtype, int64_t n, int64_t group_size, int32_t* out8);

/* y_i = lsq_group_forward(x_i) for every item. */
int lsq_group_multi_forward(int dtype, const lsq_group_item* items, int32_t count, const lsq_params* p, void* stream);

/* (dx_i, ds_i, db_i) = lsq_group_backward(grad_i, x_i) for every item.  eval_mode: ds = db = 0. */
int lsq_group_multi_backward(int dtype, const lsq_group_item* items, int32_t count, const lsq_params* p, void* stream);

/* Host only, nothing is launched: how the two fused calls launch `items` on the current device.  per_item3 (3 * count
 * values): per item its launch index (the same in both directions; -1 for an item with n == 0), its forward and its
 * backward workgroup count (those of lsq_group_plan for its (dtype, n, G)); *launches: the launches per direction. */
int lsq_group_multi_plan(int dtype, const lsq_group_item* items, int32_t count, int32_t* per_item3, int32_t* launches);

#ifdef __cplusplus
}
#endif
#endif
