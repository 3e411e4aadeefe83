/* include/lsq_hip_qgemm.h -- the linear layer on packed 4- / 2-bit group-wise weights for MORE rows of x than the decode
 * kernel of include/lsq_hip_qlinear.h serves (prefill, batches of sequences): a matrix-core GEMM that reads the codes in
 * place on gfx950.
 *
 * Exported by `liblsq_hip_qgemm.so` (built from lsqfakequantize-pytorch_amd/csrc/qgemm/ for gfx950), the sixth companion of
 * `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header only borrows the dtype codes and the status
 * codes of lsq_hip.h, and the library imports no lsq_hip_* / lsq_group_* / lsq_pack_* / lsq_qlinear* symbol.  Same contract
 * as lsq_hip.h: caller-owned device buffers, kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default
 * stream), no allocation, no synchronisation, no environment variables, no atomics, 0 / negative LSQ_E* / positive
 * hipError_t returns, never throws, everything is validated before anything is enqueued; lsq_qgemm_last_error() describes
 * the calling thread's last failure.
 *
 * THE OP  (that of lsq_hip_qlinear.h)
 *     y[m, n] = sum_k x[m, k] * w[n, k]  (+ bias[n]),      w[n, k] = (code[n, k] - qzero[n, k / G]) * qscale[n, k / G]
 * with the weight in THE FORMAT of include/lsq_hip_pack.h: `bits` is 4 or 2, K % G == 0, G % (8 / bits) == 0, codes
 * row-major and little-endian inside the byte, qscale float32 and qzero int32 of [N, K / G].  x is [M, K] dense, y is [M, N]
 * of the same type, bias is NULL or N values of LSQ_F32 or of x's type.  M >= 1, and as large as fits: offsets into x and y
 * are 64-bit, the number of output tiles (lsq_qgemm_plan) must fit a 31-bit grid.
 *
 * WHAT IS SERVED.  LSQ_BF16 / LSQ_F16 x, G a multiple of the 128 / bits elements of one 16-byte code packet, `codes` 16-byte
 * aligned -- the eligibility of the decode kernel's matrix-core form.  Everything else (LSQ_F32 x, small or odd G, 2 bits
 * at G = 32, misaligned codes) is NOT served: lsq_qgemm_plan reports form 0 and lsq_qgemm_forward returns LSQ_EINVAL with a
 * message that says why, and launches nothing; the caller dequantizes and calls a GEMM.  There is no cap on M.
 *
 * THE ARITHMETIC
 *  - code - qzero enters v_mfma_f32_16x16x32_{bf16,f16} as an exact integer operand, for every qzero within the format's
 *    +-2^23: an integer beyond +-128 is split into three exact pieces of 8 bits (three MFMAs); whether a group takes that
 *    path is decided from the qzero of the weight alone, never from x or M.  The weight is never rounded to 16 bits with
 *    its scale folded in.
 *  - The sum runs in fp32.  qscale multiplies, in fp32, the partial tile of one whole group (one fused multiply-add per
 *    group and output, the product unrounded); the bias is added in fp32 before the one rounding to the type of y.
 *  - The order of each output's sum depends on (K, G, bits, dtype) alone: one accumulator chain per output in ascending k,
 *    the same MFMA and the same k-to-operand-slot map in every tile shape, K never split.  Not on M, not on where the row
 *    sits in its tile, not on the tile shape the plan picked, not on the data.  So launches repeat bit for bit, and row m of
 *    an M-row call equals, bit for bit, that row in any other call of this library, wherever it sits.
 *  - NOT promised: equality with the bits of lsq_qlinear_forward.  The decode kernel splits K over 16 waves and folds
 *    qscale per packet; that is another order of the same sum.  Both meet the same bound.
 *  - Exact when the arithmetic is: if every product and partial sum is representable in fp32, y is the exact result
 *    rounded once.
 */
#ifndef LSQ_HIP_QGEMM_H_
#define LSQ_HIP_QGEMM_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_QGEMM_ABI_VERSION 1

/* LSQ_QGEMM_ABI_VERSION the library was built with. */
int lsq_qgemm_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_qgemm_last_error(void);

/* One launch: y = x @ w^T (+ bias).  `bias` may be NULL (bias_dtype is then ignored); otherwise bias_dtype is LSQ_F32 or
 * `dtype`.  x, y, qscale, qzero and bias must be element-aligned.  A format that is not served, or a `codes` pointer that
 * is not 16-byte aligned, returns LSQ_EINVAL. */
int lsq_qgemm_forward(int dtype, const void* x, int64_t M, const void* codes, int64_t N, int64_t K, int64_t group_size,
                      int bits, const void* qscale, const void* qzero, const void* bias, int bias_dtype, void* y,
                      void* stream);

/* Host only, nothing is launched: the launch of lsq_qgemm_forward for (dtype, M, N, K, group_size, bits) on the current
 * device (256 compute units are assumed when there is none) with a 16-byte aligned `codes`.  out8 = [form, grid, workgroup
 * size, rows per tile, columns per tile, bytes of LDS, elements of K per main-loop step, 0].
 * form 1 = matrix cores.  A workgroup owns one tile of 128 rows by 64 columns (4 waves), or by 16 columns (1 wave) while
 *          64-column tiles would not give every compute unit one; each wave owns 16 columns, loads their code packets
 *          with 16-byte loads and reuses one unpacked B fragment over the 16-row sub-tiles of x, which is staged in LDS.
 * form 0 = not served (see above); the other fields are 0. */
int lsq_qgemm_plan(int dtype, int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
