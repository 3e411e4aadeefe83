/* include/lsq_hip_attn_decode_w8.h -- DECODE attention on 8-bit LEVELS on gfx950 against a grouped-query KV cache, in ONE launch:
 * a few query rows per kv head, the keys of a row bounded by its key count n, nothing beyond n is read.
 *
 * Exported by `liblsq_hip_attn_decode_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/attn_decode_w8/ for gfx950), the twentieth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h and the structs `lsq_attn_w8_strides` and `lsq_attn_w8_out` of lsq_hip_attn_w8.h, and the library imports no symbol of
 * the others.  Same contract as lsq_hip.h: caller-owned device buffers, the kernel enqueued on `stream` (a hipStream_t as void*,
 * NULL = the default stream), no allocation, no workspace, no synchronisation, no atomics, no environment variables, 0 / negative
 * LSQ_E* / positive hipError_t returns, never throws, everything is validated before anything is enqueued;
 * lsq_attn_decode_w8_last_error() describes the calling thread's last failure.  Launches repeat bit for bit.
 *
 * THE DEFINITION.  q is levels [B, H, Tq, D]; k and v are levels [B, Hkv, Tk, D] with H = G Hkv, G >= 1: query head h reads kv head
 * h / G (repeat_interleave(G, dim 1), HF's repeat_kv).  Each operand is uint8 or int8 on its own with one (scale float32, zero point
 * int32) ON THE DEVICE; q, k, v and y [B, H, Tq, D] are strided as in lsq_bmm_w8 (innermost stride 1, a row stride and two batch
 * strides, in elements): a cache is read in place and q may be a view of a qkv buffer.  The softmax `table` (int32 [256] on the
 * device), the three output sides (every one a quantizer: levels out only) and their one mid_dtype are lsq_attn_fused_w8's.
 * `causal` with `causal_offset` >= 0 and `key_lengths` (int32 [B] on the device, or NULL; read in the kernel) give the key count
 * of lsq_softmax_mask_w8:
 *     n(b, t) = min(Tk,  t + 1 + causal_offset  where causal,  max(key_lengths[b], 0)  where given)
 * For every (b, h, t), with the bytes of lsq_hip_attn_w8.h / lsq_hip_attn_mask_w8.h:
 *     s_j  for j < n: the byte lsq_bmm_w8 (NT) gives for q[b, h, t] . k[b, h / G, j] with the scores' side
 *     p_j  for j < n: the byte lsq_softmax_mask_w8 gives for that prefix (byte max, E = table[m - s], the exact integer S,
 *                     float(E) * (1.0f / float(S)), mid, level())
 *     I = sum_{j < n} (p_j - z_p) (lv_j - z_v), an exact integer: KEYS j >= n TAKE NO PART
 *     u = round_to(mid, (s_v * float(I)) * s_p)  (two rounded multiplies, no fma);  y = level(u) of the context's side
 * n = 0 gives I = 0 and y = the context quantizer's level of 0.0.  (s_p, z_p): the probabilities' quantizer as an operand
 * (torchlsq.functional._act_constants), ON THE DEVICE.
 *
 * AGAINST THE THREE LAUNCHES of the masked core (lsq_bmm_w8, lsq_softmax_mask_w8, lsq_bmm_w8 on k and v repeated G times): the
 * masked softmax writes the probabilities quantizer's level of 0.0 beyond n and the second matmul sums over all Tk keys.  Where that
 * level equals z_p (every quantizer with shift 0) a masked key contributes exactly 0 and the two results are equal BIT FOR BIT.
 * Where it differs, each masked key contributes (l0 - z_p)(lv - z_v) there -- the three launches then depend on cache slots nobody
 * wrote -- and, by the definition above, nothing here.
 * Bytes of k and v at slots >= max_t n(b, t) are never read; bytes outside the logical y are never written.
 *
 * SERVED (plan family LSQ_ATTN_DECODE_W8_DECODE): R = G Tq <= 16 (the query rows that share a kv head fill at most one 16-row tile
 * of the matrix core); D % 16 == 0 and 16 <= D <= 128; Tk <= 8192; the bases of q, k and v 16-byte aligned and every stride of
 * theirs a multiple of 16.  One workgroup per (b, kv head), of 256 threads up to Tk = 256 and of 512 above; its LDS holds 16 score
 * rows of `ld` bytes (ld = 16 n with n = ceil(Tk / 16) made odd), the table (1024 bytes) and two staging tiles of 80 D bytes (v's
 * 64-key step transposed, double buffered; then the level tile):
 *     LDS bytes = 16 ld + 1024 + 160 D   <= 16 * 8208 + 1024 + 20480 = 152832 of the CU's 163840.
 * Every other legal call has the plan family LSQ_ATTN_DECODE_W8_COMPOSITION: lsq_attn_decode_w8 REFUSES it (LSQ_EINVAL, a message,
 * nothing enqueued) and the caller composes lsq_hip_attn_w8.h and lsq_hip_attn_mask_w8.h.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): a NULL geometry, constants, output side, table or buffer; NULL or
 * misaligned scales, zero points, out_scale, out_shift, table; an output side without a quantizer (levels out only); mid_dtypes
 * that differ; a level dtype that is not U8 / I8; a mid_dtype that is not LSQ_F32 / LSQ_BF16 / LSQ_F16; an extent < 1; D or Tk
 * > 65536; Tq, B, H or B * H > 2^20; H not a multiple of Hkv; a negative causal_offset; key_lengths NULL where the geometry says
 * has_lengths, given where it does not, or not 4-byte aligned; a grid beyond 2^24 - 1 workgroups; a row stride smaller than the
 * row; a negative batch stride; a y whose rows or batches overlap each other, or that overlaps q, k, v, the table or key_lengths;
 * an output range that is empty or lies neither within 0..255 nor within -128..127; a NULL out8; and, for lsq_attn_decode_w8
 * alone, a geometry the decode kernel does not serve.
 */
#ifndef LSQ_HIP_ATTN_DECODE_W8_H_
#define LSQ_HIP_ATTN_DECODE_W8_H_

#include "lsq_hip_attn_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_ATTN_DECODE_W8_ABI_VERSION 1
/* out8[0] of the plan */
#define LSQ_ATTN_DECODE_W8_COMPOSITION 0        /* legal, not served by the decode kernel: the caller composes the existing ops */
#define LSQ_ATTN_DECODE_W8_DECODE 1             /* one launch, one workgroup per (b, kv head) */
#define LSQ_ATTN_DECODE_W8_MAX_ROWS 16
#define LSQ_ATTN_DECODE_W8_MAX_TK 8192
#define LSQ_ATTN_DECODE_W8_MAX_D 128
#define LSQ_ATTN_DECODE_W8_MAX_LDS 163840

typedef struct lsq_attn_decode_w8_geom {
    int64_t B, H, Hkv, Tq, Tk, D;
    int64_t q_dtype, k_dtype, v_dtype;      /* LSQ_ATTN_W8_U8 / LSQ_ATTN_W8_I8 */
    int64_t causal, causal_offset;          /* causal != 0: row t sees t + 1 + causal_offset keys */
    int64_t has_lengths;                    /* != 0: key_lengths is given */
    lsq_attn_w8_strides q, k, v, y;         /* q, y: [B, H, Tq, D]; k, v: [B, Hkv, Tk, D] */
} lsq_attn_decode_w8_geom;

/* The operands' constants, one float32 and one int32 each ON THE DEVICE; (s_p, z_p): the probabilities as the context's sum reads them. */
typedef struct lsq_attn_decode_w8_consts {
    const void* s_q;
    const void* z_q;
    const void* s_k;
    const void* z_k;
    const void* s_v;
    const void* z_v;
    const void* s_p;
    const void* z_p;
} lsq_attn_decode_w8_consts;

/* LSQ_ATTN_DECODE_W8_ABI_VERSION the library was built with. */
int lsq_attn_decode_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_attn_decode_w8_last_error(void);

/* y = the context's levels as defined above; the three sides carry one mid_dtype; the scores' and the probabilities' ranges say
 * whether those bytes are uint8 or int8.  `key_lengths`: int32 [B] on the device where geom->has_lengths, else NULL. */
int lsq_attn_decode_w8(const lsq_attn_decode_w8_geom* geom, const lsq_attn_decode_w8_consts* consts, const lsq_attn_w8_out* scores_out,
                       const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out, const void* table, const void* key_lengths,
                       const void* q_levels, const void* k_levels, const void* v_levels, void* y, void* stream);

/* Host only, nothing is launched.  `qkv_aligned`: the bases of q, k and v are 16-byte aligned; `y_aligned`: y's is.
 * out8[0] = the family (LSQ_ATTN_DECODE_W8_*); for COMPOSITION the other slots are 0;
 * out8[1] = workgroups = B Hkv; out8[2] = threads per workgroup (256 up to Tk = 256, 512 above);
 * out8[3] = R = G Tq, the query rows of a workgroup (row g Tq + t is q[b, hkv G + g, t]);
 * out8[4] = ld, the bytes between score rows in LDS; out8[5] = LDS bytes = 16 ld + 1024 + 160 D (<= 163840);
 * out8[6] = 1 where those exceed the 65536 a kernel gets unasked and the launch asks for more (said once per device);
 * out8[7] = the store kind (LSQ_ATTN_W8_STORE_*): PACKETS with `y_aligned` and y's strides multiples of 16. */
int lsq_attn_decode_w8_plan(const lsq_attn_decode_w8_geom* geom, int qkv_aligned, int y_aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
