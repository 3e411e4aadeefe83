/* include/lsq_hip_qgemm_a8.h -- the W4A8 / W2A8 linear of include/lsq_hip_qlinear_a8.h for MORE rows than its decode kernel
 * serves (prefill, batches of sequences): an int8 matrix-core GEMM on gfx950 that reads the packed codes in place and gives,
 * row for row, THE BITS OF THE DECODE KERNEL.
 *
 * Exported by `liblsq_hip_qgemm_a8.so` (built from lsqfakequantize-pytorch_amd/csrc/qgemm_a8/ for gfx950), the seventh
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header only borrows the dtype codes and
 * the status codes of lsq_hip.h and the level codes LSQ_A8_U8 / LSQ_A8_I8 of lsq_hip_qlinear_a8.h, and the library imports no
 * lsq_hip_* / lsq_group_* / lsq_pack_* / lsq_qlinear* / lsq_qgemm_forward symbol.  Same contract as lsq_hip.h: caller-owned
 * device buffers, kernels enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no
 * synchronisation, no environment variables, no atomics, 0 / negative LSQ_E* / positive hipError_t returns, never throws,
 * everything is validated before anything is enqueued; lsq_qgemm_a8_last_error() describes the calling thread's last failure.
 *
 * THE OP  (that of lsq_hip_qlinear_a8.h)
 *     I[m, n, g] = sum_{k in group g} (lx[m, k] - zx) * (code[n, k] - qzero[n, g])          an exact integer
 *     y[m, n]    = s_x * sum_g qscale[n, g] * float(I[m, n, g])  (+ bias[n])
 * with the weight in THE FORMAT of include/lsq_hip_pack.h and levels, zx, s_x, y and bias as in lsq_hip_qlinear_a8.h.
 * M >= 1, and as large as fits: offsets into x and y are 64-bit, the number of output tiles (lsq_qgemm_a8_plan) must fit a
 * 31-bit grid.
 *
 * WHAT IS SERVED.  Exactly the eligibility of the decode kernel's matrix-core form (lsq_qlinear_a8_plan's form 1): G a
 * multiple of the 128 / bits elements of one 16-byte code packet, lcm(G, 4 packets) <= 4096 elements, `codes` 16-byte
 * aligned; every level type, every type of x (float32 included: the operand is bytes) and of y.  Everything the decode
 * plan calls generic (small or odd G, 2 bits at G = 32, very large G, misaligned codes) is NOT served: lsq_qgemm_a8_plan
 * reports form 0, the forwards return LSQ_EINVAL with a message that says why and launch nothing; the caller keeps such
 * calls on the decode kernel, LSQ_QLINEAR_A8_MAX_ROWS rows at a time.
 *
 * THE ARITHMETIC -- the order of the floating-point sum is the contract
 *  - I is exact (32-bit integers when every |qzero| of a wave's 16 columns is at most 256, else 64-bit) and is converted to
 *    fp32 with one rounding: an integer has no order, so which tile or MFMA formed it does not matter.
 *  - K is cut as lsq_qlinear_a8_plan cuts it: spans of lcm(G, 4 packets) elements, chunks of floor(4096 / span) spans.
 *    Output (m, n) has 16 chains w = 0..15, each starting at +0.0f.  Chain w walks the chunks in ascending order, within a
 *    chunk the spans s = w, w + 16, ... in ascending order, within a span the groups in ascending order, and does
 *        acc_w = acc_w + qscale[n, g] * float(I[m, n, g])
 *    as ONE fp32 MULTIPLY (rounded) FOLLOWED BY ONE fp32 ADD (rounded) -- not a fused multiply-add; the decode library is
 *    built with -ffp-contract=off and its code has v_mul_f32 / v_add_f32 there; this library says __fmul_rn / __fadd_rn.
 *    Then sum = +0.0f; sum = sum + acc_0; ...; sum = sum + acc_15 -- every chain, the empty ones too -- and
 *        y = round(sum * s_x + bias),  again a rounded multiply followed by a rounded add, the bias in fp32.
 *    That is the decode kernel's order (its 16 waves are the 16 chains, its ordered LDS reduction the last sum), so row m of
 *    an M-row call is, bit for bit, lsq_qlinear_a8_forward* on that row alone -- whatever M is, wherever the row sits,
 *    whichever tile shape the plan picked -- and repeated launches are bit-identical.
 *
 * TWO ENTRY FORMS OVER ONE KERNEL
 *  - lsq_qgemm_a8_forward_levels: the levels as bytes, s_x and zx on the device, as in lsq_qlinear_a8_forward_levels.
 *  - lsq_qgemm_a8_forward (fused): floating x.  A pre-pass of this library writes the byte operand level(x) - off (off = 128
 *    for a range within 0..255, else 0), formed with lsq_math.hpp's make_qparams / level() exactly as the decode kernel
 *    forms it, ONCE into `levels_ws`, a caller-owned device buffer of M * K bytes, 16-byte aligned; the GEMM then runs on
 *    those bytes and derives s_x and the zero point in the kernel from `scale` and `shift` -- nothing is read back, and no
 *    level is formed twice.  `levels_ws` may be reused as soon as the call's kernels have run.
 */
#ifndef LSQ_HIP_QGEMM_A8_H_
#define LSQ_HIP_QGEMM_A8_H_

#include "lsq_hip.h"
#include "lsq_hip_qlinear_a8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_QGEMM_A8_ABI_VERSION 1

/* LSQ_QGEMM_A8_ABI_VERSION the library was built with. */
int lsq_qgemm_a8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_qgemm_a8_last_error(void);

/* Levels in: the arguments of lsq_qlinear_a8_forward_levels with M >= 1.  A format that is not served, or a `codes` pointer
 * that is not 16-byte aligned, returns LSQ_EINVAL. */
int lsq_qgemm_a8_forward_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx,
                                const void* codes, int64_t N, int64_t K, int64_t group_size, int bits, const void* qscale,
                                const void* qzero, const void* bias, int bias_dtype, void* y, int y_dtype, void* stream);

/* Floating x in (fused): the arguments of lsq_qlinear_a8_forward with M >= 1, and `levels_ws`: M * K bytes on the device,
 * 16-byte aligned, written by this call. */
int lsq_qgemm_a8_forward(int dtype, const void* x, int64_t M, const void* scale, const void* shift, int64_t quant_min,
                         int64_t quant_max, int64_t type_min, int64_t type_max, const void* codes, int64_t N, int64_t K,
                         int64_t group_size, int bits, const void* qscale, const void* qzero, const void* bias,
                         int bias_dtype, void* y, void* levels_ws, void* stream);

/* Host only, nothing is launched: the launch of either entry form for (M, N, K, group_size, bits) on the current device
 * (256 compute units are assumed when there is none) with a 16-byte aligned `codes`.  out8 = [form, grid, workgroup size,
 * rows per tile, columns per tile, bytes of LDS, elements of K per main-loop step, 16-row sub-tiles per workgroup (SUBS)].
 * form 1 = matrix cores.  A workgroup owns one tile of 16 * SUBS rows by 64 columns (4 waves), or by 16 columns (1 wave)
 *          while 64-column tiles would not give every compute unit one; SUBS is 8, or 4 / 2 when all of M is at most 64 /
 *          32 rows.  Each wave owns 16 columns and walks K chain by chain (see THE ARITHMETIC).
 * form 0 = not served (see above); the other fields are 0. */
int lsq_qgemm_a8_plan(int64_t M, int64_t N, int64_t K, int64_t group_size, int bits, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
