/* include/lsq_hip_linrope_w4.h -- the qkv projection of an attention block's DECODE STEP on packed 4- / 2-bit group-wise weight codes
 * (THE FORMAT of include/lsq_hip_pack.h) with the rotary embedding and the KV-cache append in its epilogue, on gfx950: up to 16 rows of
 * activation levels on the codes of a qkv weight [(H + 2 Hkv) D, K * bits / 8], and in ONE launch the rotated q levels out, the
 * rotated k levels at their token of a dense [B, Hkv, Tmax, D] cache or of a paged pool, and the v levels beside them.  The qkv
 * bytes that lsq_hip_lindec_w4.h writes only for lsq_hip_rope_w8.h and lsq_hip_attn_paged_w8.h's append to read them straight back
 * never reach memory.  It is for the packed weights what lsq_hip_linrope_w8.h is for 8-bit weight levels.
 *
 * Exported by `liblsq_hip_linrope_w4.so` (built from lsqfakequantize-pytorch_amd/csrc/linrope_w4/ for gfx950), the thirty-first
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h, the level codes of lsq_hip_qlinear_a8.h, the projection struct of lsq_hip_linglu_w4.h, the geometry struct of
 * lsq_hip_linrope_w8.h (reused, not redefined), the two sides of lsq_hip_rope_w8.h and the pages struct of
 * lsq_hip_attn_paged_w8.h, and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device
 * buffers, the kernel enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation,
 * no atomics, no environment variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is validated
 * before anything is enqueued; lsq_linrope_w4_last_error() describes the calling thread's last failure.
 *
 * THE OP.  NOTHING NEW IS DEFINED.  With qkv = lsq_lindec_w4_linear_levels(x, codes ..., proj->out) viewed as [B, T, H + 2 Hkv, D]
 * -- q its first H heads, k the next Hkv, v the last Hkv -- every byte written equals, bit for bit, the ops of
 * lsq_hip_linrope_w8.h's list run on that qkv: rq as lsq_rope_w8 HALF with scatter = 0, dense k as HALF with scatter = 1, dense v as
 * COPY with scatter = 1, paged k and v as lsq_kv_append_paged_w8 of the rotated k and of v.  WHERE A ROW GOES is that header's rule
 * row by row, its one stated exception included: a paged k at p >= P is not written.  Per column v is lsq_hip_lindec_w4.h's fp32
 * value -- span s (lcm(G, 4 code packets) elements) of a chunk of x belongs to wave s % 16; a wave's groups run in ascending order
 * and its accumulator carries across the chunks; the 16 waves' sums are added in wave order; then * s_x; then + bias; each step
 * one rounded fp32 operation, never an fma --, the qkv byte is lsq_hip_requant_w8.h's steps after v, the rotation
 * lsq_hip_rope_w8.h's on two of those bytes, its level the shared output side's.  Row m does not depend on M.  No atomics;
 * launches repeat bit for bit.  Whether a caller takes this library is a matter of speed alone.
 *
 * WHAT IS SERVED: 1 <= B T <= 16; bits 4 or 2; group_size a multiple of the 128 / bits elements of one 16-byte code packet with
 * lcm(group_size, 4 packets) <= 4096 elements; 0 < K <= 2^30, K % group_size == 0; the HALF pairing; D % 32 == 0 and R % 32 == 0,
 * 32 <= R <= D; levels out on every side; x_levels, codes, cos, sin and the three destinations 16-byte aligned, every destination
 * stride a multiple of 16 bytes; paged: any ps >= 1.  Everything else is refused with a message (the package's host layer runs the
 * ops above for it before calling in).
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): a NULL geometry, projection, side, table or buffer; an illegal format
 * (bits, group_size, K % group_size); for the projection everything lsq_hip_requant_w8.h refuses of the output quantizer, `relu`
 * set, a bias that is neither float32 nor of mid_dtype; for the geometry, the tables, the output side and the pages everything
 * lsq_hip_linrope_w8.h refuses; B T > 16; N != (H + 2 Hkv) D; a format, D, R, style, alignment or stride outside the list above;
 * rows of a destination that overlap each other; a destination overlapping another destination, x, the codes, the tables,
 * positions or the block table; a NULL out9.
 */
#ifndef LSQ_HIP_LINROPE_W4_H_
#define LSQ_HIP_LINROPE_W4_H_

#include "lsq_hip.h"
#include "lsq_hip_linglu_w4.h"
#include "lsq_hip_linrope_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINROPE_W4_ABI_VERSION 1
#define LSQ_LINROPE_W4_MAX_ROWS 16

/* The projection is lsq_linglu_w4_proj: `codes` [N, K * bits / 8] bytes, 16-byte aligned, N = (H + 2 Hkv) D; `qscale` float32 and
 * `qzero` int32 of [N, K / group_size]; `bias` NULL or [N] of `bias_dtype`; `out`: the quantizer of the qkv levels, `relu` 0. */
typedef lsq_linglu_w4_proj lsq_linrope_w4_proj;

/* LSQ_LINROPE_W4_ABI_VERSION the library was built with. */
int lsq_linrope_w4_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_linrope_w4_last_error(void);

/* As lsq_linrope_w8 with the packed projection and its format: `x_levels` [B T, K] bytes of `level_dtype` with `s_x` and `zx` on
 * the device; `geom`, `qkv`, `rot`, `cos`, `sin`, `positions`, `block_table` and the three destinations as there. */
int lsq_linrope_w4(int level_dtype, const void* x_levels, const void* s_x, const void* zx, const lsq_linrope_w4_proj* proj, int64_t N,
                   int64_t K, int64_t group_size, int bits, const lsq_linrope_w8_geom* geom, const lsq_rope_w8_in* qkv,
                   const lsq_rope_w8_out* rot, const void* cos, const void* sin, const void* positions, const void* block_table, void* rq,
                   void* k, void* v, void* stream);

/* Host only, nothing is launched: the launch for the geometry, K and the format on the current device (256 compute units are
 * assumed when there is none).  `aligned`: whether x_levels, codes, the tables and the three destinations are 16-byte aligned.
 * out9 = [served (0: refused by lsq_linrope_w4 as not served -- the other eight are 0), grid, workgroup size, bytes of LDS (exact),
 * chunks of K (of at most 4096 elements, whole spans), x_resident (one chunk holds all of K: x and the per-group sums are staged
 * once per workgroup and stay in LDS across its items), ROTATE items, PASS items, COPY items] -- the items of lsq_linrope_w8_plan.
 * The grid is persistent: min(items, compute units) workgroups of 16 waves. */
int lsq_linrope_w4_plan(const lsq_linrope_w8_geom* geom, int64_t K, int64_t group_size, int bits, int aligned, int32_t* out9);

#ifdef __cplusplus
}
#endif
#endif
