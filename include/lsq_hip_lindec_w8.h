/* include/lsq_hip_lindec_w8.h -- the DECODE SHAPE of the W8A8 linears with an 8-bit output on gfx950: up to 16 rows of
 * activation levels on a [N, K] matrix of 8-bit weight levels, levels out, with an optional residual given as levels.  The four
 * linears of a decoder layer's decode step (qkv, o + residual, gate_up, down + residual) stream nearly all of the step's bytes;
 * this library streams them with the 16-wave weight-streaming work split of lsq_hip_qlinear_w8.h's decode kernel and writes one
 * byte per output.
 *
 * Exported by `liblsq_hip_lindec_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/lindec_w8/ for gfx950), the twenty-sixth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h, the output quantizer struct and level codes of lsq_hip_requant_w8.h and the residual and pre-quantizer structs of
 * lsq_hip_resadd_w8.h, and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device
 * buffers, kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation,
 * no environment variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is validated before
 * anything is enqueued; lsq_lindec_w8_last_error() describes the calling thread's last failure.
 *
 * THE OP.  NOTHING NEW IS DEFINED.  With the exact integer I of lsq_hip_qlinear_w8.h every output byte equals, bit for bit,
 *     lsq_requant_w8_linear_levels' (lsq_hip_requant_w8.h: v, u, the ReLU select, level())           when `res` is NULL,
 *     lsq_resadd_w8_linear_levels'  (lsq_hip_resadd_w8.h: u, the optional p, d, t, the select, level()) when it is given:
 * the device functions that form the byte are those libraries', compiled into this one.  No atomics; launches repeat bit for
 * bit; a row's bytes depend on that row, its residual bytes, the weight and the constants alone.
 *
 * WHAT IS SERVED: 1 <= M <= 16, K % 16 == 0, 0 < K <= 65536, w_levels and x_levels 16-byte aligned.  Every other legal call of
 * the two libraries above is NOT served here and is refused with a message (the package's host layer sends it to them before
 * calling in).  y and the residual may lie at any byte offset.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): everything lsq_hip_requant_w8.h refuses, with a residual everything
 * lsq_hip_resadd_w8.h refuses (a residual whose M * N bytes overlap y's included), a `pre` without a residual, M > 16, a K
 * or an alignment outside the list above, a NULL out8.
 */
#ifndef LSQ_HIP_LINDEC_W8_H_
#define LSQ_HIP_LINDEC_W8_H_

#include "lsq_hip.h"
#include "lsq_hip_requant_w8.h"
#include "lsq_hip_resadd_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINDEC_W8_ABI_VERSION 1
#define LSQ_LINDEC_W8_MAX_ROWS 16
/* out8[6] and out8[7] of the plan */
#define LSQ_LINDEC_W8_BYTES 0
#define LSQ_LINDEC_W8_PACKETS 1

/* LSQ_LINDEC_W8_ABI_VERSION the library was built with. */
int lsq_lindec_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_lindec_w8_last_error(void);

/* lsq_requant_w8_linear_levels' arguments, the residual `res` (NULL: none -- the op is lsq_requant_w8_linear_levels') and the
 * layer's own output fake-quantizer `pre` (NULL: none; only with a residual).  `x_levels` is [M, K] bytes of `level_dtype`,
 * y and res->levels are [M, N] bytes at any byte offset. */
int lsq_lindec_w8_linear_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx,
                                int w_level_dtype, const void* w_levels, int64_t N, int64_t K, const void* w_scale,
                                const void* w_zero, const void* bias, int bias_dtype, const lsq_requant_w8_out* out,
                                const lsq_resadd_w8_res* res, const lsq_resadd_w8_pre* pre, void* y, void* stream);

/* Host only, nothing is launched: the launch for (M, N, K) on the current device (256 compute units are assumed when there is
 * none).  `aligned`: whether w_levels AND x_levels are 16-byte aligned; `y_aligned` / `res_aligned`: whether y / the residual is.
 * out8 = [served (0: refused -- the other seven are 0), grid, workgroup size, bytes of LDS, chunks of K (of at most 4096),
 * x_resident (one chunk holds all of K: x is staged once per workgroup and stays in LDS across its tiles), store
 * (LSQ_LINDEC_W8_PACKETS: N % 16 == 0 and `y_aligned`, one 16-byte packet per row and tile; else _BYTES), res_load (the same
 * for the residual: N % 16 == 0 and `res_aligned`)].
 * The grid is persistent: min(ceil(N / 16), compute units) workgroups of 16 waves, each walking tiles of 16 output columns;
 * a weight of fewer than 16 * compute units rows leaves compute units idle. */
int lsq_lindec_w8_plan(int64_t M, int64_t N, int64_t K, int aligned, int y_aligned, int res_aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
