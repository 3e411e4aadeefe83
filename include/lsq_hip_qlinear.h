/* include/lsq_hip_qlinear.h -- a linear layer that reads packed 4- / 2-bit group-wise weights in place (decode GEMV) on gfx950.
 *
 * Exported by `liblsq_hip_qlinear.so` (built from lsqfakequantize-pytorch_amd/csrc/qlinear/ for gfx950), the fourth companion
 * of `liblsq_hip.so`: the ABIs of include/lsq_hip.h, include/lsq_hip_group.h and include/lsq_hip_pack.h are unchanged, this
 * header only borrows the dtype codes and the status codes of lsq_hip.h, and the library imports no lsq_hip_* / lsq_group_* /
 * lsq_pack_* symbol.  Same contract as lsq_hip.h: caller-owned device buffers, kernels enqueued on `stream` (a hipStream_t
 * as void*, NULL = the default stream), no allocation, no synchronisation, no environment variables, 0 / negative LSQ_E* /
 * positive hipError_t returns, never throws, everything is validated before anything is enqueued;
 * lsq_qlinear_last_error() describes the calling thread's last failure.
 *
 * THE OP
 *     y[m, n] = sum_k x[m, k] * w[n, k]  (+ bias[n]),      w[n, k] = (code[n, k] - qzero[n, k / G]) * qscale[n, k / G]
 * with the weight in THE FORMAT of include/lsq_hip_pack.h: `bits` is 4 or 2, K % G == 0, G % (8 / bits) == 0, codes row-major
 * and little-endian inside the byte (N * K * bits / 8 bytes, any byte offset), qscale float32 and qzero int32 of [N, K / G].
 * x is [M, K] dense in LSQ_BF16, LSQ_F16 or LSQ_F32 (element-aligned; LSQ_F64 is refused), y is [M, N] of the same type,
 * bias is NULL or N values of LSQ_F32 or of x's type.  1 <= M <= LSQ_QLINEAR_MAX_ROWS: the kernel streams the weight once for
 * all rows of x; larger M is the caller's business (dequantize and call a GEMM).
 *
 * THE ARITHMETIC
 *  - code - qzero is an exact integer; the sum runs in fp32; qscale may be factored out of a partial sum that lies within
 *    one group; the bias is added in fp32 before the one rounding to the type of y.
 *  - No formulation that cancels: the integer code - qzero itself is an operand, for every qzero within the format's
 *    +-2^23 (an integer beyond the exact range of a 16-bit matrix operand is split into exact pieces of 8 bits).
 *  - Deterministic: no atomics; the order of the sum depends on (K, G, bits, dtype, the form) alone, never on M or on the
 *    data of x.  Repeated launches are bit-identical, and row m of an M-row call is bit for bit the 1-row call on x[m].
 *  - Exact when the arithmetic is: if every product and partial sum is representable in fp32, y is the exact result
 *    rounded once.
 */
#ifndef LSQ_HIP_QLINEAR_H_
#define LSQ_HIP_QLINEAR_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_QLINEAR_ABI_VERSION 1
#define LSQ_QLINEAR_MAX_ROWS 16

/* LSQ_QLINEAR_ABI_VERSION the library was built with. */
int lsq_qlinear_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_qlinear_last_error(void);

/* One launch: y = x @ w^T (+ bias).  `bias` may be NULL (bias_dtype is then ignored); otherwise bias_dtype is LSQ_F32 or
 * `dtype`.  x, y, qscale, qzero and bias must be element-aligned.  A `codes` pointer that is not 16-byte aligned takes the
 * generic form (see lsq_qlinear_plan). */
int lsq_qlinear_forward(int dtype, const void* x, int64_t M, const void* codes, int64_t N, int64_t K, int64_t group_size,
                        int bits, const void* qscale, const void* qzero, const void* bias, int bias_dtype, void* y,
                        void* stream);

/* Host only, nothing is launched: the launch of lsq_qlinear_forward for (dtype, M, N, K, group_size, bits) on the current
 * device (256 compute units are assumed when there is none) with a 16-byte aligned `codes`.  out8 = [form, grid, workgroup
 * size, rows of x served natively (LSQ_QLINEAR_MAX_ROWS), bytes of LDS, elements of K per LDS chunk of x (0 in the generic
 * form), waves that share one output tile, output columns per tile].
 * form 1 = matrix cores: bf16 / fp16 x, G a multiple of the 128 / bits elements of one 16-byte code packet; a 16 x 16 output
 *          tile per workgroup, K split over its waves, 16-byte code loads, x in LDS, mfma_f32_16x16x32 on the integer
 *          code - qzero, one fp32 multiply by qscale per 16-byte packet's partial tile.
 * form 0 = generic: one wave per output column, one code byte per lane and step, fp32 multiply-add, a butterfly sum over
 *          the wave (fp32 x, small or odd G, misaligned codes). */
int lsq_qlinear_plan(int dtype, int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
