/* include/lsq_hip_linglu_w8.h -- the gate and up projections of a gated MLP's DECODE STEP with the gated product in their
 * epilogue, on gfx950: up to 16 rows of activation levels on a gate weight [C, K] and an up weight [C, K] of 8-bit levels, and
 * the levels of act(gate) * up out, [M, C] bytes, in ONE launch.  The [M, 2 C] bytes that lsq_hip_lindec_w8.h writes only for
 * lsq_hip_glu_w8.h to read them straight back never reach memory.
 *
 * Exported by `liblsq_hip_linglu_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/linglu_w8/ for gfx950), the twenty-seventh
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h, the output quantizer struct and level codes of lsq_hip_requant_w8.h and the constants struct of lsq_hip_glu_w8.h,
 * and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device buffers, the kernel enqueued
 * on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation, no environment variables,
 * 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is validated before anything is enqueued;
 * lsq_linglu_w8_last_error() describes the calling thread's last failure.
 *
 * THE OP.  NOTHING NEW IS DEFINED.  Every output byte equals, bit for bit,
 *     lsq_glu_w8(g, u, table, consts)   with   g = lsq_requant_w8_linear_levels(x, gate->..., gate->out)
 *                                              u = lsq_requant_w8_linear_levels(x, up->..., up->out):
 * the gate byte and the up byte are formed by lsq_hip_requant_w8.h's device functions on the exact integer of
 * lsq_hip_qlinear_w8.h, the product by lsq_hip_glu_w8.h's on table[gate byte] and the dequantized up byte, compiled into this
 * library.  The level type of g and u follows the range of its quantizer (within 0..255: uint8, within -128..127: int8), as it
 * does there; consts->s_u and consts->z_u are the constants of u's levels as lsq_glu_w8 takes them.  The two projections may be
 * the halves of one fused [2 C, K] weight (two views, one quantizer) or two tensors with two quantizers.  No atomics; launches
 * repeat bit for bit; a row's bytes depend on that row, the weights, the table and the constants alone.
 *
 * WHAT IS SERVED: 1 <= M <= 16, K % 16 == 0, 0 < K <= 65536, x_levels and both w_levels 16-byte aligned, levels out.  y may lie
 * at any byte offset.  Everything else is refused with a message (the package's host layer sends it to the libraries above
 * before calling in).
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): a NULL projection, constants, table or buffer; for either projection
 * everything lsq_hip_requant_w8.h refuses, and `relu` set; for the product everything lsq_hip_glu_w8.h refuses of its constants
 * and table, and a floating y (NULL out_scale); M > 16, a K or an alignment outside the list above; C < 0; a NULL out8.
 */
#ifndef LSQ_HIP_LINGLU_W8_H_
#define LSQ_HIP_LINGLU_W8_H_

#include "lsq_hip.h"
#include "lsq_hip_requant_w8.h"
#include "lsq_hip_glu_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINGLU_W8_ABI_VERSION 1
#define LSQ_LINGLU_W8_MAX_ROWS 16
/* out8[6] of the plan */
#define LSQ_LINGLU_W8_BYTES 0
#define LSQ_LINGLU_W8_PACKETS 1

/* One projection: `w_levels` [C, K] bytes of `w_level_dtype` (LSQ_REQUANT_W8_U8 / _I8), 16-byte aligned, rows K bytes apart;
 * `w_scale` float32 [C], `w_zero` int32 [C], `bias` NULL or [C] of `bias_dtype` (float32 or out->mid_dtype); `out`: the
 * quantizer of the projection's output, `relu` 0. */
typedef struct lsq_linglu_w8_proj {
    const void* w_levels;
    const void* w_scale;
    const void* w_zero;
    const void* bias;
    const lsq_requant_w8_out* out;
    int64_t w_level_dtype, bias_dtype;
} lsq_linglu_w8_proj;

/* LSQ_LINGLU_W8_ABI_VERSION the library was built with. */
int lsq_linglu_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_linglu_w8_last_error(void);

/* `x_levels` [M, K] bytes of `level_dtype` with its constants `s_x` (one float32) and `zx` (one int32) on the device; the two
 * projections; `table` the 256 float32 values of lsq_glu_w8; `consts` as lsq_glu_w8 takes them, with an output quantizer;
 * y [M, C] bytes (uint8 for an output range in 0..255, int8 for one in -128..127) at any byte offset. */
int lsq_linglu_w8(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, const lsq_linglu_w8_proj* gate,
                  const lsq_linglu_w8_proj* up, int64_t C, int64_t K, const void* table, const lsq_glu_w8_consts* consts, void* y,
                  void* stream);

/* Host only, nothing is launched: the launch for (M, C, K) on the current device (256 compute units are assumed when there is
 * none).  `aligned`: whether x_levels AND both w_levels are 16-byte aligned; `y_aligned`: whether y is.
 * out8 = [served (0: refused -- the other seven are 0), grid, workgroup size, bytes of LDS, chunks of K (of at most 4096),
 * x_resident (one chunk holds all of K: x is staged once per workgroup and stays in LDS across its tiles), store
 * (LSQ_LINGLU_W8_PACKETS: C % 16 == 0 and `y_aligned`, one 16-byte packet per row and tile; else _BYTES), 0].
 * The grid is persistent: min(ceil(C / 16), compute units) workgroups of 16 waves, each walking tiles of 16 product columns
 * with the 16 gate rows and the 16 up rows that make them. */
int lsq_linglu_w8_plan(int64_t M, int64_t C, int64_t K, int aligned, int y_aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
