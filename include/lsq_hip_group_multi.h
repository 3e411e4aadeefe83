/* include/lsq_hip_group_multi.h -- many group-wise LSQ quantizers in one launch each way, on gfx950.
 *
 * Exported by `liblsq_hip_group_multi.so` (built from lsqfakequantize-pytorch_amd/csrc/group/ for gfx950), a companion of
 * `liblsq_hip.so` and `liblsq_hip_group.so`, whose ABIs (include/lsq_hip.h, include/lsq_hip_group.h) are unchanged.  This
 * header only borrows lsq_hip.h's lsq_params, dtype codes and status codes.  Same contract as lsq_hip_group.h:
 * caller-owned device buffers, kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no
 * allocation, no synchronisation, no environment variables, no mutable global state, 0 / negative LSQ_E* / positive
 * hipError_t returns, never throws; lsq_group_multi_last_error() describes the calling thread's last failure.
 *
 * Every item is one tensor of lsq_hip_group.h's layout: `n` dense elements in groups of `group_size` (G) consecutive
 * elements, n / G values of scale / shift / ds / db (float for F32 | BF16 | F16 storage, double for F64).  G may differ
 * from item to item.  Results are, bit for bit, those of one lsq_group_forward / lsq_group_backward call per item with
 * the same lsq_params: each item is walked by exactly the workgroups its own call would launch, so its d_scale / d_shift
 * are summed in the same order.  The gradient scaler is per item: grad_scaler / sqrt(n * quant_max / (n / G)).
 *
 * The items of one call are launched in classes of one backward reduction each (the `reduction` of lsq_group_plan:
 * 16-byte packets with a power-of-two or another packet count per group, or one element per lane), at most
 * LSQ_GROUP_MULTI_ITEMS items per launch: one launch each way when every G is the same multiple of the packet width.
 * Every item is validated before anything is enqueued: a bad item fails the whole call with LSQ_EINVAL and its index in
 * the message.  Items with n == 0 take no part (their pointers are not read).  Pointers must be element-aligned.
 * p->numel_for_scaler must be 0 (there is no sharded group op).  The inside-mask and levels outputs of
 * lsq_group_forward are not offered here.
 */
#ifndef LSQ_HIP_GROUP_MULTI_H_
#define LSQ_HIP_GROUP_MULTI_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_GROUP_MULTI_ABI_VERSION 1
#define LSQ_GROUP_MULTI_ITEMS 28   /* items per launch */

/* One tensor of a call.  Forward reads x, scale, shift and writes y; backward reads grad, x, scale, shift and writes dx,
 * ds, db.  Pointers the direction does not use are ignored. */
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

/* LSQ_GROUP_MULTI_ABI_VERSION the library was built with. */
int lsq_group_multi_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_group_multi_last_error(void);

/* y_i = lsq_group_forward(x_i) for every item. */
int lsq_group_multi_forward(int dtype, const lsq_group_item* items, int32_t count, const lsq_params* p, void* stream);

/* (dx_i, ds_i, db_i) = lsq_group_backward(grad_i, x_i) for every item.  eval_mode: ds = db = 0. */
int lsq_group_multi_backward(int dtype, const lsq_group_item* items, int32_t count, const lsq_params* p, void* stream);

/* Host only, nothing is launched: how the two calls launch `items` on the current device.  per_item3 (3 * count values):
 * per item its launch index (the same in both directions; -1 for an item with n == 0), its forward and its backward
 * workgroup count (those of lsq_group_plan for its (dtype, n, G)); *launches: the launches per direction. */
int lsq_group_multi_plan(int dtype, const lsq_group_item* items, int32_t count, int32_t* per_item3, int32_t* launches);

#ifdef __cplusplus
}
#endif
#endif
