/* include/lsq_hip_attn_fused_w8.h -- the attention core softmax(q k^T) v on 8-bit LEVELS on gfx950 in ONE launch: the scores and the
 * probabilities are bytes in LDS and never reach memory.
 *
 * Exported by `liblsq_hip_attn_fused_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/attn_fused_w8/ for gfx950), the seventeenth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h and the structs `lsq_attn_w8_strides` and `lsq_attn_w8_out` of lsq_hip_attn_w8.h, and the library imports no symbol of
 * the others.  Same contract as lsq_hip.h: caller-owned device buffers, the kernel enqueued on `stream` (a hipStream_t as void*,
 * NULL = the default stream), no allocation, no workspace, no synchronisation, no atomics, no environment variables, 0 / negative
 * LSQ_E* / positive hipError_t returns, never throws, everything is validated before anything is enqueued;
 * lsq_attn_fused_w8_last_error() describes the calling thread's last failure.  Launches repeat bit for bit.
 *
 * THE DEFINITION has no arithmetic of its own.  q is levels [B, H, Tq, D], k and v are levels [B, H, Tk, D], each uint8 or int8 on
 * its own with one (scale float32, zero point int32) ON THE DEVICE; all three and y [B, H, Tq, D] are strided as in lsq_bmm_w8
 * (innermost stride 1, a row stride and two batch strides, in elements).  With the three output sides (every one a quantizer: levels
 * out only) and the softmax `table` (int32 [256] on the device), y holds byte for byte what lsq_hip_attn_w8.h's three calls give:
 *     s = lsq_bmm_w8(NT: q, k; the scores' side)             a level of the scores' quantizer per (row, key)
 *     p = lsq_softmax_w8(s, table; the probabilities' side)  a level of the probabilities' quantizer per (row, key)
 *     y = lsq_bmm_w8(NN: p, v; the context's side)           p read with (s_p, z_p), the constants of the probabilities' quantizer
 *                                                            as an operand (torchlsq.functional._act_constants), ON THE DEVICE
 * all three with one mid_dtype.  Every intermediate is a defined byte, so there is no tolerance and no rescaling of a running
 * softmax: a (b, h, row) of y depends on that row of q, on k[b, h], on v[b, h] and on the constants alone.  Bytes outside the
 * logical y are never written.
 *
 * SERVED (plan family LSQ_ATTN_FUSED_W8_FUSED): the bases of q, k and v 16-byte aligned and every stride of theirs a multiple of
 * 16; D % 16 == 0 and 16 <= D <= 128; 1 <= Tk <= 2048; any Tq >= 1.  A workgroup of four waves takes one (b, h) and 64 query rows;
 * its LDS holds 64 score rows of `ld` bytes (ld = 16 n with n = ceil(Tk / 16) made odd: the 16-byte reads of 16 rows start on
 * different banks), the table (1024 bytes) and a staging area of 80 D bytes (v's 64-key step transposed; then the level tile):
 *     LDS bytes = 64 ld + 1024 + 80 D   <= 64 * 2064 + 1024 + 10240 = 143360 of the CU's 163840.
 * Every other legal call has the plan family LSQ_ATTN_FUSED_W8_THREE_LAUNCHES: lsq_attn_fused_w8 REFUSES it (LSQ_EINVAL, a message,
 * nothing enqueued) and the caller runs the three launches of lsq_hip_attn_w8.h.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): a NULL geometry, constants, output side, table or buffer; NULL or
 * misaligned scales, zero points, out_scale, out_shift, table; an output side without a quantizer (levels out only); mid_dtypes
 * that differ; a level dtype that is not U8 / I8; a mid_dtype that is not LSQ_F32 / LSQ_BF16 / LSQ_F16; an extent < 1; D or Tk
 * > 65536; Tq, Tk, D or B * H > 2^20; a grid beyond 2^24 - 1 workgroups; a row stride smaller than the row; a negative batch stride;
 * a y whose rows or batches overlap each other, or that overlaps an operand or the table; an output range that is empty or lies
 * neither within 0..255 nor within -128..127; a NULL out8; and, for lsq_attn_fused_w8 alone, a geometry the fused kernel does not
 * serve.
 */
#ifndef LSQ_HIP_ATTN_FUSED_W8_H_
#define LSQ_HIP_ATTN_FUSED_W8_H_

#include "lsq_hip_attn_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_ATTN_FUSED_W8_ABI_VERSION 1
/* out8[0] of the plan */
#define LSQ_ATTN_FUSED_W8_THREE_LAUNCHES 0      /* legal, not served by the fused kernel: the caller composes lsq_hip_attn_w8.h */
#define LSQ_ATTN_FUSED_W8_FUSED 1               /* one launch, scores and probabilities in LDS */
#define LSQ_ATTN_FUSED_W8_MAX_TK 2048
#define LSQ_ATTN_FUSED_W8_MAX_D 128
#define LSQ_ATTN_FUSED_W8_MAX_LDS 163840

typedef struct lsq_attn_fused_w8_geom {
    int64_t B, H, Tq, Tk, D;
    int64_t q_dtype, k_dtype, v_dtype;      /* LSQ_ATTN_W8_U8 / LSQ_ATTN_W8_I8 */
    lsq_attn_w8_strides q, k, v, y;         /* q, y: [B, H, Tq, D]; k, v: [B, H, Tk, D] */
} lsq_attn_fused_w8_geom;

/* The operands' constants, one float32 and one int32 each ON THE DEVICE; (s_p, z_p): the probabilities as the second matmul reads them. */
typedef struct lsq_attn_fused_w8_consts {
    const void* s_q;
    const void* z_q;
    const void* s_k;
    const void* z_k;
    const void* s_v;
    const void* z_v;
    const void* s_p;
    const void* z_p;
} lsq_attn_fused_w8_consts;

/* LSQ_ATTN_FUSED_W8_ABI_VERSION the library was built with. */
int lsq_attn_fused_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_attn_fused_w8_last_error(void);

/* y = levels of softmax(q k^T) v as defined above; the three sides carry one mid_dtype; the scores' and the probabilities' ranges
 * say whether those bytes are uint8 or int8. */
int lsq_attn_fused_w8(const lsq_attn_fused_w8_geom* geom, const lsq_attn_fused_w8_consts* consts, const lsq_attn_w8_out* scores_out,
                      const lsq_attn_w8_out* probs_out, const lsq_attn_w8_out* ctx_out, const void* table, const void* q_levels,
                      const void* k_levels, const void* v_levels, void* y, void* stream);

/* Host only, nothing is launched.  `qkv_aligned`: the bases of q, k and v are 16-byte aligned; `y_aligned`: y's is.
 * out8[0] = the family (LSQ_ATTN_FUSED_W8_*); for THREE_LAUNCHES the other slots are 0;
 * out8[1] = workgroups = B H ceil(Tq / 64); out8[2] = threads per workgroup (256);
 * out8[3] = query rows per workgroup (64: four waves of 16, each wave owns its rows in all three phases);
 * out8[4] = ld, the bytes between score rows in LDS; out8[5] = LDS bytes = 64 ld + 1024 + 80 D (<= 163840);
 * out8[6] = 1 where those exceed the 65536 a kernel gets unasked and the launch asks for more (said once per device);
 * out8[7] = the store kind (LSQ_ATTN_W8_STORE_*): PACKETS with `y_aligned` and y's strides multiples of 16. */
int lsq_attn_fused_w8_plan(const lsq_attn_fused_w8_geom* geom, int qkv_aligned, int y_aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
