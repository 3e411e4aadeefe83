/* include/lsq_hip_linglu_w4.h -- the gate and up projections of a gated MLP's DECODE STEP on packed 4- / 2-bit group-wise weight
 * codes (THE FORMAT of include/lsq_hip_pack.h) with the gated product in their epilogue, on gfx950: up to 16 rows of activation
 * levels on a gate strip [C, K * bits / 8] and an up strip [C, K * bits / 8] of codes, and the levels of act(gate) * up out, [M, C]
 * bytes, in ONE launch.  The [M, 2 C] bytes that lsq_hip_lindec_w4.h writes only for lsq_hip_glu_w8.h to read them straight back
 * never reach memory.  It is for the packed weights what lsq_hip_linglu_w8.h is for 8-bit weight levels.
 *
 * Exported by `liblsq_hip_linglu_w4.so` (built from lsqfakequantize-pytorch_amd/csrc/linglu_w4/ for gfx950), the thirtieth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h, the level codes of lsq_hip_qlinear_a8.h (LSQ_A8_U8 / LSQ_A8_I8, the values of LSQ_REQUANT_W8_U8 / _I8), the output
 * quantizer struct of lsq_hip_requant_w8.h and the constants struct of lsq_hip_glu_w8.h, and the library imports no symbol of the
 * others.  Same contract as lsq_hip.h: caller-owned device buffers, the kernel enqueued on `stream` (a hipStream_t as void*,
 * NULL = the default stream), no allocation, no synchronisation, no environment variables, 0 / negative LSQ_E* / positive
 * hipError_t returns, never throws, everything is validated before anything is enqueued; lsq_linglu_w4_last_error() describes the
 * calling thread's last failure.
 *
 * THE OP.  NOTHING NEW IS DEFINED.  Every output byte equals, bit for bit,
 *     lsq_glu_w8(g, u, table, consts)   with   g = lsq_lindec_w4_linear_levels(x, gate->..., gate->out)
 *                                              u = lsq_lindec_w4_linear_levels(x, up->..., up->out):
 * for each strip v is the fp32 value of lsq_qlinear_a8_forward_levels in that kernel's order of the sum, as lsq_hip_lindec_w4.h
 * states it -- span s (lcm(G, 4 code packets) elements) of a chunk of x belongs to wave s % 16; a wave's groups run in ascending
 * order and its accumulator carries across the chunks; the 16 waves' sums are added in wave order; then * s_x; then + bias; each
 * step one rounded fp32 operation, never an fma --, the gate byte and the up byte are lsq_hip_requant_w8.h's steps after v, the
 * product is lsq_hip_glu_w8.h's on table[gate byte] and the dequantized up byte, its level the shared output side's.  The level
 * type of g and u follows the range of its quantizer (within 0..255: uint8, within -128..127: int8); consts->s_u and consts->z_u
 * are the constants of u's levels as lsq_glu_w8 takes them.  The two strips may be the row halves of one fused [2 C, K] packed
 * weight (two views, one quantizer) or two tensors with two quantizers.  Row m does not depend on M.  No atomics; launches repeat
 * bit for bit.  Whether a caller takes this library is a matter of speed alone.
 *
 * WHAT IS SERVED: 1 <= M <= 16; bits 4 or 2; both strips of one `bits` and one `group_size`, a format of lsq_hip_qlinear_a8.h's
 * matrix-core form -- group_size a multiple of the 128 / bits elements of one 16-byte code packet and lcm(group_size, 4 packets)
 * <= 4096 elements --; 0 < K <= 2^30; C <= 2^30; x_levels and both `codes` 16-byte aligned; levels out.  y may lie at any byte
 * offset.  Everything else is refused with a message (the package's host layer composes it from the existing ops before calling in).
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): a NULL projection, constants, table or buffer; an illegal format (bits,
 * group_size, K % group_size); for either projection everything lsq_hip_requant_w8.h refuses of the output quantizer, `relu` set,
 * a bias that is neither float32 nor of mid_dtype; for the product everything lsq_hip_glu_w8.h refuses of its constants and table,
 * and a floating y (NULL out_scale); M > 16, a format or an alignment outside the list above; a NULL out8.
 */
#ifndef LSQ_HIP_LINGLU_W4_H_
#define LSQ_HIP_LINGLU_W4_H_

#include "lsq_hip.h"
#include "lsq_hip_requant_w8.h"
#include "lsq_hip_glu_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINGLU_W4_ABI_VERSION 1
#define LSQ_LINGLU_W4_MAX_ROWS 16
/* out8[6] of the plan */
#define LSQ_LINGLU_W4_BYTES 0
#define LSQ_LINGLU_W4_PACKETS 1

/* One projection: `codes` [C, K * bits / 8] bytes, 16-byte aligned, rows K * bits / 8 bytes apart; `qscale` float32 and `qzero`
 * int32 of [C, K / group_size]; `bias` NULL or [C] of `bias_dtype` (float32 or out->mid_dtype); `out`: the quantizer of the
 * projection's output, `relu` 0. */
typedef struct lsq_linglu_w4_proj {
    const void* codes;
    const void* qscale;
    const void* qzero;
    const void* bias;
    const lsq_requant_w8_out* out;
    int64_t bias_dtype;
} lsq_linglu_w4_proj;

/* LSQ_LINGLU_W4_ABI_VERSION the library was built with. */
int lsq_linglu_w4_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_linglu_w4_last_error(void);

/* `x_levels` [M, K] bytes of `level_dtype` (0: 0..255, 1: -128..127) with its constants `s_x` (one float32) and `zx` (one int32) on
 * the device; the two projections, both of `group_size` and `bits`; `table` the 256 float32 values of lsq_glu_w8; `consts` as
 * lsq_glu_w8 takes them, with an output quantizer; y [M, C] bytes (uint8 for an output range in 0..255, int8 for one in
 * -128..127) at any byte offset. */
int lsq_linglu_w4(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, const lsq_linglu_w4_proj* gate,
                  const lsq_linglu_w4_proj* up, int64_t C, int64_t K, int64_t group_size, int bits, const void* table,
                  const lsq_glu_w8_consts* consts, void* y, void* stream);

/* Host only, nothing is launched: the launch for (M, C, K, group_size, bits) on the current device (256 compute units are assumed
 * when there is none).  `aligned`: whether x_levels AND both `codes` are 16-byte aligned; `y_aligned`: whether y is.
 * out8 = [served (0: refused -- the other seven are 0), grid, workgroup size, bytes of LDS, chunks of K (of at most 4096 elements,
 * whole spans), x_resident (one chunk holds all of K: x and the per-group sums are staged once per workgroup and stay in LDS
 * across its tiles), store (LSQ_LINGLU_W4_PACKETS: C % 16 == 0 and `y_aligned`, one 16-byte packet per row and tile; else _BYTES),
 * 0].  The grid is persistent: min(ceil(C / 16), compute units) workgroups of 16 waves, each walking tiles of 16 product columns
 * with the 16 gate rows and the 16 up rows that make them. */
int lsq_linglu_w4_plan(int64_t M, int64_t C, int64_t K, int64_t group_size, int bits, int aligned, int y_aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
