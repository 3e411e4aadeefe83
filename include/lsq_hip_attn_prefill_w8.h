/* include/lsq_hip_attn_prefill_w8.h -- PREFILL attention on 8-bit LEVELS on gfx950: causal and key-length masked, grouped-query, any
 * number of query rows, in ONE launch; the scores and the probabilities stay in LDS and nothing above the diagonal is computed.
 *
 * Exported by `liblsq_hip_attn_prefill_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/attn_prefill_w8/ for gfx950), the
 * twenty-first companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the structs
 * `lsq_attn_decode_w8_geom` and `lsq_attn_decode_w8_consts` of lsq_hip_attn_decode_w8.h and, through it, `lsq_attn_w8_strides` and
 * `lsq_attn_w8_out` of lsq_hip_attn_w8.h, and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned
 * device buffers, the kernel enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no workspace,
 * no synchronisation, no atomics, no environment variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws,
 * everything is validated before anything is enqueued; lsq_attn_prefill_w8_last_error() describes the calling thread's last
 * failure.  Launches repeat bit for bit.
 *
 * THE DEFINITION is lsq_hip_attn_decode_w8.h's, word for word: q [B, H, Tq, D], k and v [B, Hkv, Tk, D] with H = G Hkv, query head
 * h reads kv head h / G; the operands' dtypes, constants and strides, the softmax `table`, the three output sides with their one
 * mid_dtype, `causal` with `causal_offset` >= 0 and `key_lengths` (int32 [B] on the device, or NULL; read in the kernel); the key
 * count
 *     n(b, t) = min(Tk,  t + 1 + causal_offset  where causal,  max(key_lengths[b], 0)  where given)
 * and the bytes s_j, p_j (j < n), the exact integer I over the keys j < n and y = level(u) of the context's side.  KEYS j >= n TAKE
 * NO PART and are never read -- slots at or beyond the workgroup's largest n included --; n = 0 gives the context quantizer's level
 * of 0.0; bytes outside the logical y are never written.
 *
 * SERVED (plan family LSQ_ATTN_PREFILL_W8_PREFILL): any Tq >= 1 and any G >= 1; D % 16 == 0 and 16 <= D <= 128; the bases of q, k
 * and v 16-byte aligned and every stride of theirs a multiple of 16; and Tk_eff <= 2048, where
 *     Tk_eff = min(Tk, Tq + causal_offset)  where causal,  else Tk
 * is the largest key count any row can have as the host knows it (key_lengths lives on the device and does not enter): a long cache
 * is served in place, Tk = 8192 with a prompt of 2048 tokens is served.  One workgroup of 256 threads per (b, h, 64-row tile); wave
 * w owns rows 16 w .. 16 w + 15 in all three phases and its key loops end at its last live row's n (the G heads of a kv head are
 * separate workgroups, adjacent in the grid: k and v are shared through L2).  Its LDS holds 64 score rows of `ld` bytes (ld = 16 n
 * with n = ceil(Tk_eff / 16) made odd), the table (1024 bytes) and one staging tile of 80 D bytes (v's 64-key step transposed; then
 * the level tile):
 *     LDS bytes = 64 ld + 1024 + 80 D   <= 64 * 2064 + 1024 + 10240 = 143360 of the CU's 163840.
 * Every other legal call has the plan family LSQ_ATTN_PREFILL_W8_COMPOSITION: lsq_attn_prefill_w8 REFUSES it (LSQ_EINVAL, a
 * message, nothing enqueued) and the caller composes lsq_hip_attn_w8.h and lsq_hip_attn_mask_w8.h (or, with G Tq <= 16, calls
 * lsq_attn_decode_w8).
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): those of lsq_hip_attn_decode_w8.h -- a NULL geometry, constants, output
 * side, table or buffer; NULL or misaligned scales, zero points, out_scale, out_shift, table; an output side without a quantizer
 * (levels out only); mid_dtypes that differ; a level dtype that is not U8 / I8; a mid_dtype that is not LSQ_F32 / LSQ_BF16 /
 * LSQ_F16; an extent < 1; D or Tk > 65536; Tq, B, H or B * H > 2^20; H not a multiple of Hkv; a negative causal_offset; key_lengths
 * NULL where the geometry says has_lengths, given where it does not, or not 4-byte aligned; a grid beyond 2^24 - 1 workgroups; a
 * row stride smaller than the row; a negative batch stride; a y whose rows or batches overlap each other, or that overlaps q, k, v,
 * the table or key_lengths; an output range that is empty or lies neither within 0..255 nor within -128..127; a NULL out8; and,
 * for lsq_attn_prefill_w8 alone, a geometry the prefill kernel does not serve.
 */
#ifndef LSQ_HIP_ATTN_PREFILL_W8_H_
#define LSQ_HIP_ATTN_PREFILL_W8_H_

#include "lsq_hip_attn_decode_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_ATTN_PREFILL_W8_ABI_VERSION 1
/* out8[0] of the plan */
#define LSQ_ATTN_PREFILL_W8_COMPOSITION 0       /* legal, not served by the prefill kernel: the caller composes the existing ops */
#define LSQ_ATTN_PREFILL_W8_PREFILL 1           /* one launch, one workgroup per (b, h, 64-row tile) */
#define LSQ_ATTN_PREFILL_W8_ROWS 64
#define LSQ_ATTN_PREFILL_W8_MAX_TK_EFF 2048
#define LSQ_ATTN_PREFILL_W8_MAX_D 128
#define LSQ_ATTN_PREFILL_W8_MAX_LDS 163840

/* LSQ_ATTN_PREFILL_W8_ABI_VERSION the library was built with. */
int lsq_attn_prefill_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_attn_prefill_w8_last_error(void);

/* y = the context's levels as defined in lsq_hip_attn_decode_w8.h; the arguments are lsq_attn_decode_w8's. */
int lsq_attn_prefill_w8(const lsq_attn_decode_w8_geom* geom, const lsq_attn_decode_w8_consts* consts, const lsq_attn_w8_out* scores_out,
                        const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out, const void* table, const void* key_lengths,
                        const void* q_levels, const void* k_levels, const void* v_levels, void* y, void* stream);

/* Host only, nothing is launched.  `qkv_aligned`: the bases of q, k and v are 16-byte aligned; `y_aligned`: y's is.
 * out8[0] = the family (LSQ_ATTN_PREFILL_W8_*); for COMPOSITION the other slots are 0;
 * out8[1] = workgroups = B H ceil(Tq / 64); out8[2] = threads per workgroup (256); out8[3] = query rows per workgroup (64);
 * out8[4] = ld, the bytes between score rows in LDS (16 n, n = ceil(Tk_eff / 16) made odd);
 * out8[5] = LDS bytes = 64 ld + 1024 + 80 D (<= 143360);
 * out8[6] = 1 where those exceed the 65536 a kernel gets unasked and the launch asks for more (said once per device);
 * out8[7] = the store kind (LSQ_ATTN_W8_STORE_*): PACKETS with `y_aligned` and y's strides multiples of 16. */
int lsq_attn_prefill_w8_plan(const lsq_attn_decode_w8_geom* geom, int qkv_aligned, int y_aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
