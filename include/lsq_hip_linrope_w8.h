/* include/lsq_hip_linrope_w8.h -- the qkv projection of an attention block's DECODE STEP with the rotary embedding and the KV-cache
 * append in its epilogue, on gfx950: up to 16 rows of activation levels on a qkv weight [(H + 2 Hkv) D, K] of 8-bit levels, and in
 * ONE launch the rotated q levels out, the rotated k levels at their token of a dense [B, Hkv, Tmax, D] cache or of a paged pool,
 * and the v levels beside them.  The qkv bytes that lsq_hip_lindec_w8.h writes only for lsq_hip_rope_w8.h and
 * lsq_hip_attn_paged_w8.h's append to read them straight back never reach memory.
 *
 * Exported by `liblsq_hip_linrope_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/linrope_w8/ for gfx950), the twenty-eighth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h, the output quantizer struct and level codes of lsq_hip_requant_w8.h, the output side of lsq_hip_rope_w8.h and the
 * pages struct of lsq_hip_attn_paged_w8.h, and the library imports no symbol of the others.  Same contract as lsq_hip.h:
 * caller-owned device buffers, the kernel enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation,
 * no synchronisation, no atomics, no environment variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws,
 * everything is validated before anything is enqueued; lsq_linrope_w8_last_error() describes the calling thread's last failure.
 *
 * THE OP.  NOTHING NEW IS DEFINED.  With qkv = lsq_requant_w8_linear_levels(x, w ..., proj->out) viewed as [B, T, H + 2 Hkv, D] --
 * q its first H heads, k the next Hkv, v the last Hkv -- and s_q, z_q (`qkv_scale`, `qkv_zero`) the constants of ITS levels, every
 * byte written equals, bit for bit,
 *     rq            lsq_rope_w8(q; HALF, scatter = 0) through the three strides q_sb, q_st, q_sh;
 *     k, dense      lsq_rope_w8(k; HALF, scatter = 1, Tout = Tmax) into the cache, strides (batch, token, head);
 *     v, dense      lsq_rope_w8(v; LSQ_ROPE_W8_COPY, scatter = 1, Tout = Tmax);
 *     k, v, paged   lsq_kv_append_paged_w8(lsq_rope_w8(k; HALF, scatter = 0), v) into the pools, strides (page, slot, head),
 * formed by the same device functions, compiled into this library.  Token (b, t), row m = b T + t of x, has the position
 * p = positions[b] + t; `positions` is int32 [B] on the device or NULL for zeros and is READ in the kernel by every workgroup,
 * never written (the caller advances it after the launch).  WHERE A ROW GOES, decided once per row:
 *     rq       not written where p < 0 or p >= P;
 *     dense    k not written where p < 0, p >= P or p >= Tmax;  v not written where p < 0 or p >= Tmax;
 *     paged    k and v not written where p < 0, p >= Mp ps, or block_table[b, p / ps] lies outside [0, Np);  AND k IS NOT WRITTEN
 *              WHERE p >= P: there the composition above appends a row of its temporary that the rotation left as allocated, which
 *              is undefined; everywhere the composition is defined the bytes are equal.
 * No byte of a destination changes for a row that is not written.  No atomics; launches repeat bit for bit; a row's bytes depend
 * on that row, the weight, the tables and the constants alone.
 *
 * WHAT IS SERVED: 1 <= B T <= 16; K % 16 == 0, 0 < K <= 65536; the HALF pairing; D % 32 == 0 and R % 32 == 0, 32 <= R <= D; levels
 * out on every side; x_levels, w_levels, cos, sin and the three destinations 16-byte aligned, every destination stride a multiple
 * of 16 bytes; paged: any ps >= 1.  Everything else is refused with a message (the package's host layer runs the ops above for
 * it before calling in).
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): a NULL geometry, projection, side, table or buffer; for the projection
 * everything lsq_hip_requant_w8.h refuses, and `relu` set; for the tables and the output side everything lsq_hip_rope_w8.h refuses
 * (P below 1 or beyond 29 bits, an odd R, R above D, misaligned constants or positions, a range outside a byte type), and a
 * floating output (NULL out_scale); for the pages everything lsq_hip_attn_paged_w8.h's append refuses (an extent below 1, bt_ld <
 * Mp, Mp ps or Np beyond 2^29, a NULL or misaligned block table); an extent below 1; B T > 16; N != (H + 2 Hkv) D; a K, D, R,
 * style, alignment or stride outside the list above; a negative stride or one that takes an offset beyond 2^58; rows of a
 * destination that overlap each other; a destination overlapping another destination, x, the weight, the tables, positions or
 * the block table; a NULL out9.
 */
#ifndef LSQ_HIP_LINROPE_W8_H_
#define LSQ_HIP_LINROPE_W8_H_

#include "lsq_hip.h"
#include "lsq_hip_requant_w8.h"
#include "lsq_hip_rope_w8.h"
#include "lsq_hip_attn_paged_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINROPE_W8_ABI_VERSION 1
#define LSQ_LINROPE_W8_MAX_ROWS 16

/* The projection: `w_levels` [N, K] bytes of `w_level_dtype` (LSQ_REQUANT_W8_U8 / _I8), 16-byte aligned, rows K bytes apart,
 * N = (H + 2 Hkv) D; `w_scale` float32 [N], `w_zero` int32 [N], `bias` NULL or [N] of `bias_dtype` (float32 or out->mid_dtype);
 * `out`: the quantizer of the qkv levels, `relu` 0. */
typedef struct lsq_linrope_w8_proj {
    const void* w_levels;
    const void* w_scale;
    const void* w_zero;
    const void* bias;
    const lsq_requant_w8_out* out;
    int64_t w_level_dtype, bias_dtype;
} lsq_linrope_w8_proj;

/* Shapes, strides (in bytes = elements) and where k and v go.  dense (`paged` 0): the caches hold Tmax tokens, k_so / v_so is the
 * batch stride and k_st / v_st the token stride; `pages` is not read.  paged: the pools hold pages.Np pages of pages.ps slots,
 * k_so / v_so is the page stride and k_st / v_st the slot stride; Tmax is not read.  k_sh / v_sh: the head stride. */
typedef struct lsq_linrope_w8_geom {
    int64_t B, T, H, Hkv, D, R, P;
    int64_t style;                  /* LSQ_ROPE_W8_HALF; LSQ_ROPE_W8_INTERLEAVED is refused (not served) */
    int64_t q_sb, q_st, q_sh;       /* rq's batch, token and head strides */
    int64_t paged, Tmax;
    int64_t k_so, k_st, k_sh;
    int64_t v_so, v_st, v_sh;
    lsq_attn_paged_w8_pages pages;
} lsq_linrope_w8_geom;

/* LSQ_LINROPE_W8_ABI_VERSION the library was built with. */
int lsq_linrope_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_linrope_w8_last_error(void);

/* `x_levels` [B T, K] bytes of `level_dtype` with its constants `s_x` (one float32) and `zx` (one int32) on the device; the
 * projection; `qkv` the constants of the qkv levels as lsq_rope_w8 takes them (s_x float32 [1], zx int32 [1]); `rot` the output
 * side of the rotation (levels); `cos` / `sin` float32 [P, R / 2]; `positions` int32 [B] or NULL; `block_table` int32
 * [B, pages.Mp] with rows pages.bt_ld apart (paged) or NULL (dense); the destinations: `rq` [B, T, H, D] levels of `rot`, `k`
 * levels of `rot` and `v` levels of the projection's quantizer in the caches or pools. */
int lsq_linrope_w8(int level_dtype, const void* x_levels, const void* s_x, const void* zx, const lsq_linrope_w8_proj* proj, int64_t N,
                   int64_t K, const lsq_linrope_w8_geom* geom, const lsq_rope_w8_in* qkv, const lsq_rope_w8_out* rot, const void* cos,
                   const void* sin, const void* positions, const void* block_table, void* rq, void* k, void* v, void* stream);

/* Host only, nothing is launched: the launch for the geometry and K on the current device (256 compute units are assumed when
 * there is none).  `aligned`: whether x_levels, w_levels, the tables and the three destinations are 16-byte aligned.
 * out9 = [served (0: refused by lsq_linrope_w8 as not served -- the other eight are 0), grid, workgroup size, bytes of LDS, chunks
 * of K (of at most 4096), x_resident (one chunk holds all of K: x is staged once per workgroup and stays in LDS across its items),
 * ROTATE items, PASS items, COPY items].  An item is two 16-column strips of the weight: ROTATE the features f0 .. f0 + 15
 * (f0 < R / 2) and f0 + R / 2 .. of a q or k head -- (H + Hkv) R / 32 items --, PASS two adjacent strips beyond R of a q or k
 * head -- (H + Hkv) (D - R) / 32 --, COPY two adjacent strips of a v head -- Hkv D / 32.  The grid is persistent:
 * min(items, compute units) workgroups of 16 waves. */
int lsq_linrope_w8_plan(const lsq_linrope_w8_geom* geom, int64_t K, int aligned, int32_t* out9);

#ifdef __cplusplus
}
#endif
#endif
