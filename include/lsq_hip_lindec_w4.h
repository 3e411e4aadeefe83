/* include/lsq_hip_lindec_w4.h -- the DECODE SHAPE of the W4A8 / W2A8 linears with an 8-bit output on gfx950: up to 16 rows of
 * activation levels on packed 4- / 2-bit group-wise weight codes (THE FORMAT of include/lsq_hip_pack.h), levels out, with an
 * optional residual given as levels, in ONE launch.  It is for the packed weights what lsq_hip_lindec_w8.h is for 8-bit weight
 * levels: the weight bytes are nearly all of a decode step's bytes, and the packed format is (bits / 8 + 8 / G) of them.
 *
 * Exported by `liblsq_hip_lindec_w4.so` (built from lsqfakequantize-pytorch_amd/csrc/lindec_w4/ for gfx950), the twenty-ninth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h, the level codes of lsq_hip_qlinear_a8.h (LSQ_A8_U8 / LSQ_A8_I8, the values of LSQ_REQUANT_W8_U8 / _I8), the output
 * quantizer struct of lsq_hip_requant_w8.h and the residual and pre-quantizer structs of lsq_hip_resadd_w8.h, and the library
 * imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device buffers, kernels enqueued on `stream` (a
 * hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation, no environment variables, 0 / negative
 * LSQ_E* / positive hipError_t returns, never throws, everything is validated before anything is enqueued;
 * lsq_lindec_w4_last_error() describes the calling thread's last failure.
 *
 * THE OP.  NOTHING NEW IS DEFINED.  Let v be the fp32 value that lsq_qlinear_a8_forward_levels (lsq_hip_qlinear_a8.h) rounds to
 * its y on the same operands: the exact integer I per group, ONE conversion per group, acc + qscale * float(I), the fp32 sum over
 * the groups in THAT KERNEL'S ORDER (matrix-core form) --
 *     span s (lcm(G, 4 code packets) elements) of a chunk of x belongs to wave s % 16; a wave's groups run in ascending order
 *     and its accumulator carries across the chunks; the 16 waves' sums are added in wave order; then * s_x; then + bias
 * -- each step one rounded fp32 operation, never an fma.  The output byte is
 *     res == NULL:  lsq_hip_requant_w8.h's steps after v: u = float(round_to(mid_dtype, v)), the ReLU select, level();
 *     res given:    lsq_hip_resadd_w8.h's steps after v: u, the optional p (`pre`), d, t, the select, level().
 * CONSEQUENCES.  Every byte equals the composition of existing ops on the same device: lsq_qlinear_a8_forward_levels writing a
 * `mid_dtype` y (the op lsq_linear_packed_q8(..., out_dtype=mid_dtype)), the `pre` fake-quantize forward, the add in mid_dtype of
 * the dequantized residual, the select, the per-tensor levels forward (lsq_levels_per_tensor).  Row m does not depend on M.  No
 * atomics; launches repeat bit for bit.  The int8 GEMM of liblsq_hip_qgemm_a8.so keeps the same order of the sum, so rows beyond
 * 16 served by that composition have the same bits: whether a caller takes this library is a matter of speed alone.
 *
 * WHAT IS SERVED: 1 <= M <= 16; bits 4 or 2; the formats of lsq_hip_qlinear_a8.h's matrix-core form -- group_size a multiple of
 * the 128 / bits elements of one 16-byte code packet and lcm(group_size, 4 packets) <= 4096 elements --; K > 0; `codes` and
 * `x_levels` 16-byte aligned.  y and the residual may lie at any byte offset.  Every other legal call of
 * lsq_qlinear_a8_forward_levels is NOT served here and is refused with a message (the package's host layer composes it from the
 * existing ops before calling in).
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): an illegal format (bits, group_size, K % group_size), everything
 * lsq_hip_requant_w8.h refuses of the output quantizer, with a residual everything lsq_hip_resadd_w8.h refuses (a residual whose
 * M * N bytes overlap y's included), a `pre` without a residual, a bias that is neither float32 nor of mid_dtype, M > 16, a
 * format or an alignment outside the list above.
 */
#ifndef LSQ_HIP_LINDEC_W4_H_
#define LSQ_HIP_LINDEC_W4_H_

#include "lsq_hip.h"
#include "lsq_hip_requant_w8.h"
#include "lsq_hip_resadd_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINDEC_W4_ABI_VERSION 1
#define LSQ_LINDEC_W4_MAX_ROWS 16
/* out8[6] and out8[7] of the plan */
#define LSQ_LINDEC_W4_BYTES 0
#define LSQ_LINDEC_W4_PACKETS 1

/* LSQ_LINDEC_W4_ABI_VERSION the library was built with. */
int lsq_lindec_w4_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_lindec_w4_last_error(void);

/* `x_levels` is [M, K] bytes of `level_dtype` (0: 0..255, 1: -128..127), `s_x` one float32 and `zx` one int32 on the device; the
 * weight is `codes` [N, K * bits / 8] bytes with `qscale` float32 and `qzero` int32 of [N, K / group_size]; `bias` is NULL or N
 * values of LSQ_F32 or of out->mid_dtype; `res` (NULL: none) and `pre` (NULL: none; only with a residual) as in
 * lsq_hip_resadd_w8.h; y and res->levels are [M, N] bytes at any byte offset. */
int lsq_lindec_w4_linear_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, const void* codes,
                                int64_t N, int64_t K, int64_t group_size, int bits, const void* qscale, const void* qzero,
                                const void* bias, int bias_dtype, const lsq_requant_w8_out* out, const lsq_resadd_w8_res* res,
                                const lsq_resadd_w8_pre* pre, void* y, void* stream);

/* Host only, nothing is launched: the launch for (M, N, K, group_size, bits) on the current device (256 compute units are assumed
 * when there is none).  `aligned`: whether codes AND x_levels are 16-byte aligned; `y_aligned` / `res_aligned`: whether y / the
 * residual is.  out8 = [served (0: refused -- the other seven are 0), grid, workgroup size, bytes of LDS, chunks of K (of at most
 * 4096 elements, whole spans), x_resident (one chunk holds all of K: x is staged once per workgroup and stays in LDS across its
 * tiles), store (LSQ_LINDEC_W4_PACKETS: N % 16 == 0 and `y_aligned`, one 16-byte packet per row and tile; else _BYTES), res_load
 * (the same for the residual: N % 16 == 0 and `res_aligned`)].
 * The grid is persistent: min(ceil(N / 16), compute units) workgroups of 16 waves, each walking tiles of 16 output columns. */
int lsq_lindec_w4_plan(int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int aligned, int y_aligned, int res_aligned,
                       int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
