/* include/lsq_hip_linmid_w4.h -- the W4A8 / W2A8 linears with an 8-bit output on gfx950 for 17 to 64 ROWS of activation levels
 * on packed 4- / 2-bit group-wise weight codes (THE FORMAT of include/lsq_hip_pack.h), levels out, with an optional residual given
 * as levels: ONE launch that streams the weight ONCE.  It continues lsq_hip_lindec_w4.h (1 to 16 rows, one MFMA tile) into the
 * batches a decoder is served at: a workgroup keeps 2, 3 or 4 sub-tiles of 16 rows against every weight fragment it unpacks.
 *
 * Exported by `liblsq_hip_linmid_w4.so` (built from lsqfakequantize-pytorch_amd/csrc/linmid_w4/ for gfx950), the thirty-second
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows what lsq_hip_lindec_w4.h borrows,
 * and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device buffers, kernels enqueued on
 * `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation, no environment variables, 0 /
 * negative LSQ_E* / positive hipError_t returns, never throws, everything is validated before anything is enqueued;
 * lsq_linmid_w4_last_error() describes the calling thread's last failure.
 *
 * THE OP.  NOTHING NEW IS DEFINED: it is lsq_hip_lindec_w4.h's, word for word.  v is the float-output decode kernel's fp32 value
 * (the exact integer I per group, ONE conversion, acc + qscale * float(I) as a rounded multiply then a rounded add; span s of a
 * chunk of 4096 k belongs to wave slot s % 16; a slot's groups ascend and its accumulator carries across the chunks; the 16 slots
 * are summed in slot order; then * s_x; then + bias), the byte is lsq_hip_requant_w8.h's steps after v, with a residual
 * lsq_hip_resadd_w8.h's.  CONSEQUENCES.  Every byte equals the composition of the existing ops on the same device, and so the
 * bytes of lsq_lindec_w4_linear_levels on any 16 of the rows.  Row m does not depend on M.  No atomics; launches repeat bit for bit.
 *
 * WHAT IS SERVED: 17 <= M <= 64; bits 4 or 2; group_size a multiple of the 128 / bits elements of one 16-byte code packet with
 * lcm(group_size, 4 packets) <= 4096 elements; K > 0; `codes` and `x_levels` 16-byte aligned.  y and the residual may lie at any
 * byte offset.  Everything else is refused with a message (the package's host layer takes lsq_hip_lindec_w4.h up to 16 rows and
 * composes the existing ops otherwise).
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): those of lsq_hip_lindec_w4.h, with M < 17 or M > 64 in place of M > 16.
 */
#ifndef LSQ_HIP_LINMID_W4_H_
#define LSQ_HIP_LINMID_W4_H_

#include "lsq_hip.h"
#include "lsq_hip_requant_w8.h"
#include "lsq_hip_resadd_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINMID_W4_ABI_VERSION 1
#define LSQ_LINMID_W4_MIN_ROWS 17
#define LSQ_LINMID_W4_MAX_ROWS 64
/* out8[6] and out8[7] of the plan */
#define LSQ_LINMID_W4_BYTES 0
#define LSQ_LINMID_W4_PACKETS 1

/* LSQ_LINMID_W4_ABI_VERSION the library was built with. */
int lsq_linmid_w4_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_linmid_w4_last_error(void);

/* The arguments of lsq_lindec_w4_linear_levels (lsq_hip_lindec_w4.h), for 17 <= M <= 64. */
int lsq_linmid_w4_linear_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, const void* codes,
                                int64_t N, int64_t K, int64_t group_size, int bits, const void* qscale, const void* qzero,
                                const void* bias, int bias_dtype, const lsq_requant_w8_out* out, const lsq_resadd_w8_res* res,
                                const lsq_resadd_w8_pre* pre, void* y, void* stream);

/* Host only, nothing is launched: the launch for (M, N, K, group_size, bits) on the current device (256 compute units are assumed
 * when there is none).  `aligned`: whether codes AND x_levels are 16-byte aligned; `y_aligned` / `res_aligned`: whether y / the
 * residual is.  out8 = [served (0: refused -- the other seven are 0), grid, workgroup size, bytes of LDS (at most 160 KB), subs
 * (sub-tiles of 16 rows a wave keeps: ceil(M / 16)), stages (windows of x a full chunk of K is staged in: 1 when the rows of a
 * whole chunk fit in LDS), store (LSQ_LINMID_W4_PACKETS: N % 16 == 0 and `y_aligned`, one 16-byte packet per row and tile; else
 * _BYTES), res_load (the same for the residual)].
 * The grid is persistent: min(ceil(N / 16), compute units) workgroups of 8 waves (512 threads), each wave owning two of the 16 wave
 * slots, each workgroup walking tiles of 16 output columns. */
int lsq_linmid_w4_plan(int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int aligned, int y_aligned, int res_aligned,
                       int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
