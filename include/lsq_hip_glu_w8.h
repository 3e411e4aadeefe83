/* include/lsq_hip_glu_w8.h -- the gated product of a gated MLP (SwiGLU / GeGLU / classic GLU) on 8-bit LEVELS on gfx950:
 * y = act(gate) * up in ONE launch, the activation read from a 256-entry FLOAT table indexed by the gate byte, both operands
 * read in place through a row stride -- so the two halves of a fused gate_up linear's [M, 2 C] output need no copy -- and the
 * next quantizer's levels (or floats) out.  What makes a converted Llama / Mistral / Qwen / Gemma MLP stay in levels between its
 * gate_up linear and its down linear.
 *
 * Exported by `liblsq_hip_glu_w8.so` (built from lsqfakequantize-pytorch_amd/csrc/glu_w8/ for gfx950), the twenty-fifth
 * companion of `liblsq_hip.so`: the ABIs of the other headers are unchanged, this header borrows the dtype and status codes of
 * lsq_hip.h, and the library imports no symbol of the others.  Same contract as lsq_hip.h: caller-owned device buffers, kernels
 * enqueued on `stream` (a hipStream_t as void*, NULL = the default stream), no allocation, no synchronisation, no environment
 * variables, 0 / negative LSQ_E* / positive hipError_t returns, never throws, everything is validated before anything is
 * enqueued; lsq_glu_w8_last_error() describes the calling thread's last failure.
 *
 * THE OP.  gate and up are [rows, C] bytes of gate_dtype / up_dtype (LSQ_GLU_W8_U8: 0..255, LSQ_GLU_W8_I8: -128..127, the two
 * independent) at any byte offset, element (r, c) of each at r * its row stride + c; y is a DENSE [rows, C] tensor (a floating y:
 * element-aligned).  `table` is 256 float32 values on the device, 4-byte aligned, indexed by the gate BYTE as stored (an int8
 * level l reads entry l & 0xff) and holding values of mid_dtype (an entry that is not one is rounded to mid_dtype first).  With
 * s_u, z_u ONE float32 / int32 each on the device, read in the kernel as they are, and `mid` = consts->mid_dtype (LSQ_F32:
 * identity, LSQ_BF16, LSQ_F16):
 *     a = float(round_to(mid, table[gate byte]))                       the identity on a value of mid
 *     d = float(round_to(mid, (float(l_u) - float(z_u)) * s_u))        fp32 subtract, one rounded fp32 multiply, one rounding
 *     t = float(round_to(mid, a * d))                                  one rounded fp32 multiply, never contracted
 *     with out_scale:  q = level(t; out),  y = q mod 256               lsq_math.hpp's level() with make_qparams(
 *                                                                      sanitize_scale_per_tensor(out_scale[0]), out_shift[0],
 *                                                                      range); a NaN goes to quant_min
 *     without:         y = round_to(mid, a * d), stored as mid
 * The kernel knows no activation function and no constants of the gate: the package builds the table from existing ops
 * (dequantize the 256 bytes, apply the function -- and, where the model has a quantizer after the activation, take its levels
 * and dequantize them again).  No atomics; launches repeat bit for bit; an output depends on its own two bytes, the table and
 * the constants alone; bytes outside the logical y, and the bytes between the rows of gate and up, are never written; the GPU
 * result equals the package's CPU path (the existing ops composed) bit for bit for the same table.
 *
 * REFUSALS (LSQ_EINVAL, a message, nothing is enqueued): a NULL shape, constants, gate, up, table or y; NULL or misaligned s_u,
 * z_u, out_scale, out_shift (out_scale and out_shift come together); a table that is not 4-byte aligned; a level dtype that is
 * not LSQ_GLU_W8_U8 / _I8; a mid_dtype that is not LSQ_F32 / LSQ_BF16 / LSQ_F16; a floating y that is not element-aligned; rows
 * or C < 1; a row stride < C; shapes beyond 64-bit offsets; an output range that is empty or lies neither within 0..255 nor
 * within -128..127; y overlapping the span of gate, of up or the table; more workgroups than a 31-bit grid; a NULL out8.
 */
#ifndef LSQ_HIP_GLU_W8_H_
#define LSQ_HIP_GLU_W8_H_

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_GLU_W8_ABI_VERSION 1
#define LSQ_GLU_W8_U8 0
#define LSQ_GLU_W8_I8 1
/* out8[0] of the plan */
#define LSQ_GLU_W8_GENERIC 0             /* one lane per element */
#define LSQ_GLU_W8_PACKETS 1             /* 16-byte packets */

/* The shape of one call: gate, up and y [rows, C]; the row strides of gate and up in bytes (y is dense). */
typedef struct lsq_glu_w8_shape {
    int64_t rows, C, gate_row_stride, up_row_stride;
} lsq_glu_w8_shape;

/* The constants: `s_u` one float32 and `z_u` one int32 ON THE DEVICE, read in the kernel as they are; `out_scale` and
 * `out_shift` one float32 each on the device, or both NULL for a floating y of mid_dtype. */
typedef struct lsq_glu_w8_consts {
    const void* s_u;
    const void* z_u;
    const void* out_scale;
    const void* out_shift;
    int64_t quant_min, quant_max, type_min, type_max, mid_dtype;
} lsq_glu_w8_consts;

/* LSQ_GLU_W8_ABI_VERSION the library was built with. */
int lsq_glu_w8_abi_version(void);

/* Message for the last non-zero status returned to the calling thread ("" if none). */
const char* lsq_glu_w8_last_error(void);

/* The gated product: y [rows, C] bytes (uint8 for an output range in 0..255, int8 for one in -128..127) or mid_dtype floats. */
int lsq_glu_w8(int gate_dtype, const void* gate_levels, int up_dtype, const void* up_levels, const void* table,
               const lsq_glu_w8_shape* shape, const lsq_glu_w8_consts* consts, void* y, void* stream);

/* Host only, nothing is launched.  `aligned`: gate, up and y are 16-byte aligned.
 * out8[0] = the kernel family (LSQ_GLU_W8_*): PACKETS needs `aligned`, C % 16 == 0 and both row strides % 16 == 0, every other
 * legal call is GENERIC; out8[1] = workgroups, out8[2] = threads per workgroup, out8[3] = 16-byte packets of gate (and of up) per
 * lane P (PACKETS: 2, halved while the grid holds fewer than two workgroups per compute unit; GENERIC: 1, an element),
 * out8[4] = LDS bytes (PACKETS: the table, 1024), out8[5] = packets (rows * C / 16; GENERIC: 0; at most 2^31 - 1 is reported),
 * out8[6] = out8[7] = 0. */
int lsq_glu_w8_plan(const lsq_glu_w8_shape* shape, int aligned, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
