"""Op loader and registration for the MI355X build of torchlsq.

This module replaces two pieces of the reference:
  * torchlsq/extension.py (reference :12-56), which located `_C.so` and `torch.ops.load_library`-ed
    it: here the native part is `liblsq_hip.so`, a C-ABI HIP library (include/lsq_hip.h) opened
    with ctypes;
  * the registration blocks of the C++ extension -- the schemas (csrc/ops/lsq.cpp:137-146,
    csrc/torchlsq.cpp:35-39), the composite front op `lsq` (lsq.cpp:104-134), the autograd-key
    kernels (csrc/ops/autograd/lsq_autograd.cpp) and the backend kernels' argument checks
    (lsq_cpu.cpp:28-29,72-78,159-163,214-223) -- which are restated with `torch.library`.

Dispatch keys: HIP tensors carry PyTorch's "CUDA" dispatch key on ROCm builds, so the gfx950
kernels are registered under "CUDA".  CPU tensors are served, like in the reference
(TORCH_LIBRARY_IMPL(torchlsq, CPU), lsq_cpu.cpp:298-311), by kernels for host memory: `liblsq_cpu.so`
(include/lsq_cpu.h, csrc/cpu/lsq_cpu_twin.cpp), registered under "CPU".  The two never substitute for
each other: a GPU tensor is only ever handled by the HIP library, and when `liblsq_hip.so` is missing
the package refuses to work at all (`_assert_has_ops`), CPU tensors included.
"""
import torch

from . import _abi
from ._abi import *  # noqa: F401,F403  (structures, C_ABI tables, loaders: the names tests and tools import from here)
from ._abi import (ABI_VERSION, C_ABI, C_ABI_CPU, _assert_has_ops, _check_hip_version, _has_ops, host_binding,  # noqa: F401
                   library, native_lsq, set_host_binding, set_library)
from ._hip_host import *  # noqa: F401,F403
from ._hip_host import (_SINGLE_LAUNCH_BWD, _TICKET_SLABS, _TICKETS, _WS_BYTES_PC, _WS_BYTES_PT, _check, _dense,  # noqa: F401
                        _wants_ticket,
                        _like_layout, _ocl, _param_dtype, _params, _physical_order, _ROW_MAJOR, _transposition, hip_backward_from_mask,
                        hip_backward_per_channel, hip_backward_per_channel_multi, hip_backward_per_tensor,
                        hip_forward_per_channel, hip_forward_per_channel_multi, hip_forward_per_tensor, hip_meanstd,
                        hip_minmax, hip_multi_eligible, hip_observer_update, hip_plan_backward_per_channel, hip_sharded_finish, HipComm, LSQ_COMM_ID_BYTES,
                        LSQ_COMM_MAX, LSQ_COMM_MIN, LSQ_COMM_SUM,
                        saves_mask, set_single_launch_backward)
from ._cpu_host import _cpu_meanstd, _cpu_minmax, cpu_backward, cpu_forward, cpu_levels, cpu_sharded_finish  # noqa: F401
from ._group_host import (check_group_args, group_backward, group_backward_multi, group_forward,  # noqa: F401
                          group_forward_multi, group_multi_plan, group_plan)
from ._pack_host import pack_dequantize, pack_plan, pack_quantize, pack_unpack  # noqa: F401
from ._qlinear_host import qlinear_forward, qlinear_plan  # noqa: F401
from ._qlinear_a8_host import qlinear_a8_forward, qlinear_a8_forward_levels, qlinear_a8_plan  # noqa: F401
from ._qgemm_host import qgemm_forward, qgemm_plan  # noqa: F401
from ._qgemm_a8_host import qgemm_a8_forward, qgemm_a8_forward_levels, qgemm_a8_min_rows, qgemm_a8_plan  # noqa: F401
from ._qlinear_w8_host import qlinear_w8_forward, qlinear_w8_forward_levels, qlinear_w8_plan  # noqa: F401
from ._qconv_w8_host import qconv_w8_forward, qconv_w8_forward_levels, qconv_w8_plan  # noqa: F401
from ._requant_w8_host import (requant_w8_conv, requant_w8_conv_levels, requant_w8_linear, requant_w8_linear_levels,  # noqa: F401
                               requant_w8_plan_conv, requant_w8_plan_linear)
from ._resadd_w8_host import resadd_w8_conv_levels, resadd_w8_linear_levels, resadd_w8_plan_conv, resadd_w8_plan_linear  # noqa: F401
from ._pool_w8_host import (pool_w8_adaptive_kernel, pool_w8_avg, pool_w8_avg_q, pool_w8_max, pool_w8_plan_avg,  # noqa: F401
                            pool_w8_plan_max)
from ._dwconv_w8_host import dwconv_w8_levels, dwconv_w8_levels_q, dwconv_w8_plan  # noqa: F401
from ._eltwise_w8_host import (eltwise_w8_lut, eltwise_w8_mul_gate, eltwise_w8_mul_gate_q, eltwise_w8_plan_lut,  # noqa: F401
                               eltwise_w8_plan_mul)
from ._norm_w8_host import norm_w8_layer, norm_w8_layer_q, norm_w8_plan, norm_w8_rms, norm_w8_rms_q  # noqa: F401
from ._attn_w8_host import (attn_w8_bmm, attn_w8_bmm_q, attn_w8_plan_bmm, attn_w8_plan_softmax, attn_w8_softmax,  # noqa: F401
                            attn_w8_softmax_q)
from ._attn_fused_w8_host import attn_fused_w8_plan, attn_fused_w8_q  # noqa: F401
from ._attn_mask_w8_host import attn_mask_w8_plan_softmax, attn_mask_w8_softmax, attn_mask_w8_softmax_q  # noqa: F401
from ._rope_w8_host import rope_w8, rope_w8_kv_copy, rope_w8_plan, rope_w8_q  # noqa: F401
from ._attn_decode_w8_host import attn_decode_w8_plan, attn_decode_w8_q  # noqa: F401
from ._attn_prefill_w8_host import attn_prefill_w8_plan, attn_prefill_w8_q  # noqa: F401
from ._attn_decode_split_w8_host import attn_decode_split_w8_plan, attn_decode_split_w8_q  # noqa: F401
from ._attn_paged_w8_host import (attn_paged_w8_plan, attn_paged_w8_q, kv_append_paged_w8, kv_append_paged_w8_plan,  # noqa: F401
                                  kv_gather_paged_w8)
from ._attn_chunk_w8_host import attn_chunk_paged_w8_plan, attn_chunk_paged_w8_q, attn_chunk_w8_plan, attn_chunk_w8_q  # noqa: F401
from ._glu_w8_host import glu_w8, glu_w8_plan, glu_w8_q  # noqa: F401


def __getattr__(name):
    # loader state lives in _abi (it changes at run time: set_host_binding, set_library); read it through this module too
    if name in ("_LIB", "_HAS_OPS", "_CPU_LIB", "_GROUP_LIB", "_PACK_LIB", "_QLINEAR_LIB", "_QLINEAR_A8_LIB", "_QGEMM_LIB", "_QGEMM_A8_LIB", "_QLINEAR_W8_LIB", "_QCONV_W8_LIB", "_REQUANT_W8_LIB", "_RESADD_W8_LIB", "_POOL_W8_LIB", "_DWCONV_W8_LIB", "_ELTWISE_W8_LIB", "_NORM_W8_LIB", "_ATTN_W8_LIB", "_ATTN_FUSED_W8_LIB", "_ATTN_MASK_W8_LIB", "_ROPE_W8_LIB", "_ATTN_DECODE_W8_LIB", "_ATTN_PREFILL_W8_LIB", "_ATTN_DECODE_SPLIT_W8_LIB", "_ATTN_PAGED_W8_LIB", "_ATTN_CHUNK_W8_LIB", "_GLU_W8_LIB", "_NATIVE_LSQ", "error_str",
                "cpu_error_str", "group_error_str", "pack_error_str", "qlinear_error_str", "qlinear_a8_error_str", "qgemm_error_str", "qgemm_a8_error_str", "qlinear_w8_error_str", "qconv_w8_error_str", "requant_w8_error_str", "resadd_w8_error_str", "pool_w8_error_str", "dwconv_w8_error_str", "eltwise_w8_error_str", "norm_w8_error_str", "attn_w8_error_str", "attn_fused_w8_error_str", "attn_mask_w8_error_str", "rope_w8_error_str", "attn_decode_w8_error_str", "attn_prefill_w8_error_str", "attn_decode_split_w8_error_str", "attn_paged_w8_error_str", "attn_chunk_w8_error_str", "glu_w8_error_str",
                "native_error_str"):
        return getattr(_abi, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


# -------------------------------------------------------------------------------------------------
# schemas -- namespace and signatures of the reference (lsq.cpp:138-145, torchlsq.cpp:36-37)
# -------------------------------------------------------------------------------------------------
_TAIL = ("int quant_min, int quant_max, int type_min, int type_max, bool use_grad_scaling, float grad_scaler, "
         "bool sym, bool eval_mode, bool init_mode")
_lib_def = torch.library.Library("torchlsq", "DEF")
_lib_def.define("_cuda_version() -> int")
_lib_def.define("lsq(Tensor x, Tensor scale, Tensor shift, int quant_min, int quant_max, int type_min, int type_max, "
                "int axis, bool use_grad_scaling, float grad_scale, bool is_affine, bool is_perchannel, "
                "bool eval_mode, bool init_mode) -> Tensor")
_lib_def.define("lsq_forward_per_tensor(Tensor x, Tensor scale, Tensor shift, " + _TAIL + ") -> Tensor")
_lib_def.define("lsq_backward_per_tensor(Tensor grad, Tensor x, Tensor scale, Tensor shift, " + _TAIL +
                ") -> (Tensor, Tensor, Tensor)")
_lib_def.define("lsq_forward_per_channel(Tensor x, Tensor scale, Tensor shift, int axis, " + _TAIL + ") -> Tensor")
_lib_def.define("lsq_backward_per_channel(Tensor grad, Tensor x, Tensor scale, Tensor shift, int axis, " + _TAIL +
                ") -> (Tensor, Tensor, Tensor)")
# Additions of this build (not in the reference):
#  * `*_wide`: backward that also takes the element count for the gradient scaler and returns the
#    un-rounded fp64 reductions ([2] or [2, C]) -- what the batch-sharded path all-reduces;
#  * `lsq_quantize_*`: forward that also emits the int8 integer levels (q - level_bias).
_lib_def.define("lsq_backward_per_tensor_wide(Tensor grad, Tensor x, Tensor scale, Tensor shift, " + _TAIL +
                ", int numel_for_scaler) -> (Tensor, Tensor)")
_lib_def.define("lsq_backward_per_channel_wide(Tensor grad, Tensor x, Tensor scale, Tensor shift, int axis, " + _TAIL +
                ", int numel_for_scaler) -> (Tensor, Tensor)")
#  * `lsq_minmax*`: one-pass running min/max (torch.aminmax semantics) for the observer init phase.
#  * `lsq_backward_from_mask`: eval-mode backward from the forward's one-byte inside mask (dx = grad * mask).
_lib_def.define("lsq_backward_from_mask(Tensor grad, Tensor mask) -> Tensor")
_lib_def.define("lsq_minmax_per_tensor(Tensor x) -> (Tensor, Tensor)")
_lib_def.define("lsq_minmax_per_channel(Tensor x, int axis) -> (Tensor, Tensor)")
#  * `lsq_meanstd*`: one-pass mean and unbiased standard deviation (torch.mean / torch.std semantics) for the
#    3-sigma initialisation of weight quantizers.
_lib_def.define("lsq_meanstd_per_tensor(Tensor x) -> (Tensor, Tensor)")
_lib_def.define("lsq_meanstd_per_channel(Tensor x, int axis) -> (Tensor, Tensor)")
_lib_def.define("lsq_quantize_per_tensor(Tensor x, Tensor scale, Tensor shift, int quant_min, int quant_max, "
                "int type_min, int type_max, int level_bias) -> (Tensor, Tensor)")
_lib_def.define("lsq_quantize_per_channel(Tensor x, Tensor scale, Tensor shift, int axis, int quant_min, "
                "int quant_max, int type_min, int type_max, int level_bias) -> (Tensor, Tensor)")
#  * `lsq_levels_*`: ONLY the int8 levels (y is not written: 5 instead of 9 bytes of traffic per fp32 element) -- the
#    conversion-time pass behind `torchlsq.functional.lsq_quantize` / `LSQFakeQuantizer.quantize`, which wraps them into real
#    torch.quint8 / torch.qint8 tensors.  The byte is (q - level_bias) mod 256 (include/lsq_hip.h, lsq_fwd_extras).
_lib_def.define("lsq_levels_per_tensor(Tensor x, Tensor scale, Tensor shift, int quant_min, int quant_max, "
                "int type_min, int type_max, int level_bias) -> Tensor")
_lib_def.define("lsq_levels_per_channel(Tensor x, Tensor scale, Tensor shift, int axis, int quant_min, "
                "int quant_max, int type_min, int type_max, int level_bias) -> Tensor")
#  * `*_per_group`: one scale / shift per run of `group_size` consecutive elements of the last dim (liblsq_hip_group.so,
#    include/lsq_hip_group.h): by definition the per-channel op on the [x.numel() // G, G] view, axis 0.
_lib_def.define("lsq_forward_per_group(Tensor x, Tensor scale, Tensor shift, int group_size, " + _TAIL + ") -> Tensor")
_lib_def.define("lsq_backward_per_group(Tensor grad, Tensor x, Tensor scale, Tensor shift, int group_size, " + _TAIL +
                ") -> (Tensor, Tensor, Tensor)")
_lib_def.define("lsq_levels_per_group(Tensor x, Tensor scale, Tensor shift, int group_size, int quant_min, int quant_max, "
                "int type_min, int type_max, int level_bias) -> Tensor")
#  * packed export of group-wise weights (liblsq_hip_pack.so, include/lsq_hip_pack.h, which defines the format): the 4- / 2-bit
#    codes of `lsq_forward_per_group`'s levels with one (scale, zero point) per group, and the two ways back -- the
#    fake-quantized values, bit for bit those of the forward, and the one-byte levels of `lsq_levels_per_group`.
_lib_def.define("lsq_pack_per_group(Tensor x, Tensor scale, Tensor shift, int group_size, int bits, int quant_min, "
                "int quant_max, int type_min, int type_max) -> (Tensor, Tensor, Tensor)")
_lib_def.define("lsq_unpack_per_group(Tensor codes, int bits, int quant_min, int level_bias) -> Tensor")
_lib_def.define("lsq_dequantize_per_group(Tensor codes, Tensor scale, Tensor zero_point, int group_size, int bits, "
                "ScalarType dtype) -> Tensor")
#  * a linear layer on the packed weight (liblsq_hip_qlinear.so, include/lsq_hip_qlinear.h): y = x @ w^T (+ bias) read from the
#    codes, for x of [..., K] and codes of [N, K * bits / 8].  Inference only.
_lib_def.define("lsq_linear_packed(Tensor x, Tensor codes, Tensor scale, Tensor zero_point, Tensor? bias, int group_size, "
                "int bits) -> Tensor")
#  * the same layer on 8-bit activation LEVELS, summed in integers (liblsq_hip_qlinear_a8.so, include/lsq_hip_qlinear_a8.h):
#    _q8 takes the levels as uint8 / int8 bytes with s_x (float32) and zx (int32) as one-element tensors; _a8 takes a floating
#    x and a per-tensor quantizer's scale, shift and range and forms the levels on the way.  Inference only.
_lib_def.define("lsq_linear_packed_q8(Tensor x_levels, Tensor s_x, Tensor zx, Tensor codes, Tensor scale, Tensor zero_point, "
                "Tensor? bias, int group_size, int bits, ScalarType out_dtype) -> Tensor")
_lib_def.define("lsq_linear_packed_a8(Tensor x, Tensor act_scale, Tensor act_shift, int quant_min, int quant_max, int type_min, "
                "int type_max, Tensor codes, Tensor scale, Tensor zero_point, Tensor? bias, int group_size, int bits) -> Tensor")
#  * W8A8: 8-bit activation levels times 8-bit weight LEVELS [N, K] (int8 / uint8) with one scale (float32) and zero point
#    (int32) per output row, summed in integers over all of K (liblsq_hip_qlinear_w8.so, include/lsq_hip_qlinear_w8.h): _q8
#    takes the activation levels, _a8 a floating x and the per-tensor quantizer's constants.  Inference only.
_lib_def.define("lsq_linear_w8_q8(Tensor x_levels, Tensor s_x, Tensor zx, Tensor w_levels, Tensor w_scale, Tensor w_zero, "
                "Tensor? bias, ScalarType out_dtype) -> Tensor")
_lib_def.define("lsq_linear_w8_a8(Tensor x, Tensor act_scale, Tensor act_shift, int quant_min, int quant_max, int type_min, "
                "int type_max, Tensor w_levels, Tensor w_scale, Tensor w_zero, Tensor? bias) -> Tensor")
#  * W8A8 conv2d: the same arithmetic over every tap and input channel of a 2-D convolution (groups == 1, zero padding) on
#    activation levels / a floating x [B, Cin, H, W] and weight LEVELS [Cout, Cin, kh, kw], both read channels-last
#    (liblsq_hip_qconv_w8.so, include/lsq_hip_qconv_w8.h); y is [B, Cout, OH, OW] in channels-last memory.  Inference only.
_lib_def.define("lsq_conv2d_w8_q8(Tensor x_levels, Tensor s_x, Tensor zx, Tensor w_levels, Tensor w_scale, Tensor w_zero, "
                "Tensor? bias, int[2] stride, int[2] padding, int[2] dilation, ScalarType out_dtype) -> Tensor")
_lib_def.define("lsq_conv2d_w8_a8(Tensor x, Tensor act_scale, Tensor act_shift, int quant_min, int quant_max, int type_min, "
                "int type_max, Tensor w_levels, Tensor w_scale, Tensor w_zero, Tensor? bias, int[2] stride, int[2] padding, "
                "int[2] dilation) -> Tensor")
#  * the four W8A8 ops with an 8-bit OUTPUT: the same sums and fp32 steps, a rounding to `mid_dtype`, an optional ReLU and the
#    next layer's per-tensor quantizer (out_scale, out_shift, its range) in the epilogue; the result is the level tensor (uint8
#    for a range in 0..255, int8 for one in -128..127) (liblsq_hip_requant_w8.so, include/lsq_hip_requant_w8.h).  Inference only.
_OUT_Q = "Tensor out_scale, Tensor out_shift, int out_quant_min, int out_quant_max, int out_type_min, int out_type_max, bool relu"
_lib_def.define("lsq_linear_w8_q8_q(Tensor x_levels, Tensor s_x, Tensor zx, Tensor w_levels, Tensor w_scale, Tensor w_zero, "
                "Tensor? bias, %s, ScalarType mid_dtype) -> Tensor" % _OUT_Q)
_lib_def.define("lsq_linear_w8_a8_q(Tensor x, Tensor act_scale, Tensor act_shift, int quant_min, int quant_max, int type_min, "
                "int type_max, Tensor w_levels, Tensor w_scale, Tensor w_zero, Tensor? bias, %s) -> Tensor" % _OUT_Q)
_lib_def.define("lsq_conv2d_w8_q8_q(Tensor x_levels, Tensor s_x, Tensor zx, Tensor w_levels, Tensor w_scale, Tensor w_zero, "
                "Tensor? bias, int[2] stride, int[2] padding, int[2] dilation, %s, ScalarType mid_dtype) -> Tensor" % _OUT_Q)
_lib_def.define("lsq_conv2d_w8_a8_q(Tensor x, Tensor act_scale, Tensor act_shift, int quant_min, int quant_max, int type_min, "
                "int type_max, Tensor w_levels, Tensor w_scale, Tensor w_zero, Tensor? bias, int[2] stride, int[2] padding, "
                "int[2] dilation, %s) -> Tensor" % _OUT_Q)
#  * the two levels-in ops of those four with a RESIDUAL given as 8-bit levels (res_levels in the output's shape, res_scale
#    float32 [1], res_zero int32 [1]) added between the rounding to `mid_dtype` and the ReLU, after the layer's own optional
#    per-tensor output fake-quantizer (pre_scale, pre_shift, its range): the end of a residual block in one launch
#    (liblsq_hip_resadd_w8.so, include/lsq_hip_resadd_w8.h).  Inference only.
_RES_Q = ("Tensor res_levels, Tensor res_scale, Tensor res_zero, Tensor? pre_scale, Tensor? pre_shift, int pre_quant_min, "
          "int pre_quant_max, int pre_type_min, int pre_type_max")
_lib_def.define("lsq_linear_w8_q8_add_q(Tensor x_levels, Tensor s_x, Tensor zx, Tensor w_levels, Tensor w_scale, Tensor w_zero, "
                "Tensor? bias, %s, ScalarType mid_dtype, %s) -> Tensor" % (_OUT_Q, _RES_Q))
_lib_def.define("lsq_conv2d_w8_q8_add_q(Tensor x_levels, Tensor s_x, Tensor zx, Tensor w_levels, Tensor w_scale, Tensor w_zero, "
                "Tensor? bias, int[2] stride, int[2] padding, int[2] dilation, %s, ScalarType mid_dtype, %s) -> Tensor" % (_OUT_Q, _RES_Q))
#  * 2-D pooling on 8-bit LEVELS [B, C, H, W], read channels-last (liblsq_hip_pool_w8.so, include/lsq_hip_pool_w8.h): the max pool
#    gives levels of the same quantizer; the average pool sums (level - x_zero) exactly, takes (float(S) * x_scale) / float(D)
#    in fp32 with ATen's divisor D, rounds to `mid_dtype` and gives the levels of the output quantizer (_q) or the floats
#    themselves.  The results are [B, C, OH, OW] in channels-last memory.  Inference only.
_lib_def.define("lsq_max_pool2d_q8(Tensor levels, int[2] kernel_size, int[2] stride, int[2] padding, int[2] dilation, "
                "bool ceil_mode) -> Tensor")
_AVG_POOL = ("Tensor levels, Tensor x_scale, Tensor x_zero, int[2] kernel_size, int[2] stride, int[2] padding, bool ceil_mode, "
             "bool count_include_pad, int? divisor_override")
_lib_def.define("lsq_avg_pool2d_q8_q(%s, Tensor out_scale, Tensor out_shift, int out_quant_min, int out_quant_max, int out_type_min, "
                "int out_type_max, ScalarType mid_dtype) -> Tensor" % _AVG_POOL)
_lib_def.define("lsq_avg_pool2d_q8(%s, ScalarType out_dtype) -> Tensor" % _AVG_POOL)
#  * W8A8 DEPTHWISE conv2d (groups == C, channel multiplier 1) on 8-bit LEVELS [B, C, H, W], read channels-last, and weight LEVELS
#    given TAP-MAJOR, [kh, kw, C], with one scale (float32) and zero point (int32) per channel (liblsq_hip_dwconv_w8.so,
#    include/lsq_hip_dwconv_w8.h): the exact integer sum over the taps of one channel, the fp32 steps of the W8A8 ops, a rounding
#    to `mid_dtype`, act (0 none, 1 ReLU, 2 ReLU6) and the levels of the output quantizer (_q) or the floats themselves.  The
#    results are [B, C, OH, OW] in channels-last memory.  Inference only.
_DWCONV = ("Tensor x_levels, Tensor s_x, Tensor zx, Tensor w_levels, Tensor w_scale, Tensor w_zero, Tensor? bias, int[2] stride, "
           "int[2] padding, int[2] dilation")
_lib_def.define("lsq_dwconv2d_w8_q8_q(%s, Tensor out_scale, Tensor out_shift, int out_quant_min, int out_quant_max, int out_type_min, "
                "int out_type_max, int act, ScalarType mid_dtype) -> Tensor" % _DWCONV)
_lib_def.define("lsq_dwconv2d_w8_q8(%s, int act, ScalarType out_dtype) -> Tensor" % _DWCONV)
#  * elementwise ops on 8-bit LEVELS (liblsq_hip_eltwise_w8.so, include/lsq_hip_eltwise_w8.h).  The TABLE op: y = table[x], the
#    index being the byte as stored (an int8 level l reads entry l & 0xff), in x's shape and memory layout, as `out_dtype` (uint8 /
#    int8: the same bytes); a 256-entry table holds any elementwise function between two per-tensor 8-bit quantizers
#    (`torchlsq.functional.lsq_act_table` builds it from existing ops).  The GATE MULTIPLY: x levels [B, C, H, W] (read
#    channels-last) or [B, C] times gate levels [B, C] or [B, C, 1, 1], each dequantized to `mid_dtype`, one rounded product, and
#    the levels of the output quantizer (_q) or the floats themselves.  Inference only.
_lib_def.define("lsq_lut_w8(Tensor x_levels, Tensor table, ScalarType out_dtype) -> Tensor")
_MUL_GATE = "Tensor x_levels, Tensor x_scale, Tensor x_zero, Tensor g_levels, Tensor g_scale, Tensor g_zero"
_lib_def.define("lsq_mul_gate_w8_q8_q(%s, Tensor out_scale, Tensor out_shift, int out_quant_min, int out_quant_max, int out_type_min, "
                "int out_type_max, ScalarType mid_dtype) -> Tensor" % _MUL_GATE)
_lib_def.define("lsq_mul_gate_w8_q8(%s, ScalarType out_dtype) -> Tensor" % _MUL_GATE)
#  * LayerNorm and RMSNorm on 8-bit LEVELS (liblsq_hip_norm_w8.so, include/lsq_hip_norm_w8.h): the last axis of a level tensor of
#    any shape is normalised with EXACT integer row statistics (LayerNorm does not use the zero point at all), then
#    (t * weight) + bias in float32, one rounding to `mid_dtype`, and the levels of the output quantizer (_q) or the floats
#    themselves, in x's shape.  Not ATen's layer_norm: a small share of the levels differs by one.  Inference only.
_NORM = "Tensor x_levels, Tensor x_scale, Tensor x_zero, Tensor? weight, Tensor? bias, float eps"
for _norm_name in ("lsq_layer_norm_w8_q8", "lsq_rms_norm_w8_q8"):
    _lib_def.define("%s_q(%s, Tensor out_scale, Tensor out_shift, int out_quant_min, int out_quant_max, int out_type_min, "
                    "int out_type_max, ScalarType mid_dtype) -> Tensor" % (_norm_name, _NORM))
    _lib_def.define("%s(%s, ScalarType out_dtype) -> Tensor" % (_norm_name, _NORM))
del _norm_name
#  * the attention core on 8-bit LEVELS (liblsq_hip_attn_w8.so, include/lsq_hip_attn_w8.h).  The BATCHED MATMUL: a [.., M, K] times
#    b [.., K, N] (`transpose_b`: [.., N, K]) per batch, 2 to 4 axes, the same batch axes, each operand uint8 / int8 with one scale
#    and zero point; the exact integer sum, (b_scale * float(I)) * a_scale, one rounding to `mid_dtype`, and the levels of the output
#    quantizer (_q) or the floats themselves, [.., M, N] dense.  Operands whose innermost stride is 1 are read in place.  The
#    SOFTMAX over the last axis: E = table[max - level] with `table` int32 [256] (`torchlsq.functional.lsq_softmax_table`), the
#    exact integer sum S, float(E) * (1 / float(S)), then as above; `row_pad` pads the rows of the result's memory to a multiple of
#    that many bytes and returns the [.., :C] view.  Not ATen's softmax: at most one level differs.  Inference only.
_BMM = "Tensor a_levels, Tensor a_scale, Tensor a_zero, Tensor b_levels, Tensor b_scale, Tensor b_zero, bool transpose_b"
_ATTN_OUT_Q = "Tensor out_scale, Tensor out_shift, int out_quant_min, int out_quant_max, int out_type_min, int out_type_max, ScalarType mid_dtype"
_lib_def.define("lsq_bmm_w8_q8_q(%s, %s) -> Tensor" % (_BMM, _ATTN_OUT_Q))
_lib_def.define("lsq_bmm_w8_q8(%s, ScalarType out_dtype) -> Tensor" % _BMM)
_lib_def.define("lsq_softmax_w8_q8_q(Tensor x_levels, Tensor table, %s, int row_pad=1) -> Tensor" % _ATTN_OUT_Q)
_lib_def.define("lsq_softmax_w8_q8(Tensor x_levels, Tensor table, ScalarType out_dtype) -> Tensor")
#  * the same attention core in ONE launch (liblsq_hip_attn_fused_w8.so, include/lsq_hip_attn_fused_w8.h): q [B, H, Tq, D], k and v
#    [B, H, Tk, D] levels with one scale and zero point each, the softmax's `table`, and the three output quantizers (the scores', the
#    probabilities', the context's) -> the context's levels [B, Tq, H D].  Byte for byte lsq_bmm_w8_q8_q (q k^T), lsq_softmax_w8_q8_q,
#    lsq_bmm_w8_q8_q (p v) composed; the scores and probabilities stay in LDS where the fused kernel serves the shape, every other
#    legal input runs the three launches.  Inference only.
_ATTN_SIDE = "Tensor %s_scale, Tensor %s_shift, int %s_quant_min, int %s_quant_max, int %s_type_min, int %s_type_max"
_lib_def.define("lsq_attention_w8_q8_q(Tensor q_levels, Tensor q_scale, Tensor q_zero, Tensor k_levels, Tensor k_scale, Tensor k_zero, "
                "Tensor v_levels, Tensor v_scale, Tensor v_zero, Tensor table, %s, %s, %s, ScalarType mid_dtype) -> Tensor"
                % tuple(_ATTN_SIDE % ((n,) * 6) for n in ("scores", "probs", "out")))
#  * the MASKED softmax on 8-bit LEVELS (liblsq_hip_attn_mask_w8.so, include/lsq_hip_attn_mask_w8.h): lsq_softmax_w8_q8(_q) over the
#    first n keys of every row of x [.., Tq, Tk] -- `causal`: row t of a matrix sees t + 1 + `causal_offset` keys; `key_lengths`:
#    int32 [x.shape[0]] on x's device, read in the kernel --, the output side's level of 0 (+0.0) beyond n; a row with n = 0 is all
#    zeros (ATen: NaN).  A row's prefix equals lsq_softmax_w8_q8(_q) of that prefix bit for bit.  Inference only.
_MASK = "bool causal=False, int causal_offset=0, Tensor? key_lengths=None"
_lib_def.define("lsq_softmax_mask_w8_q8_q(Tensor x_levels, Tensor table, %s, %s, int row_pad=1) -> Tensor" % (_ATTN_OUT_Q, _MASK))
_lib_def.define("lsq_softmax_mask_w8_q8(Tensor x_levels, Tensor table, ScalarType out_dtype, %s) -> Tensor" % _MASK)
#  * ROTARY POSITION EMBEDDING and the KV-CACHE APPEND on 8-bit LEVELS (liblsq_hip_rope_w8.so, include/lsq_hip_rope_w8.h): x
#    [B, T, H, D] levels with one scale and zero point, `cos` and `sin` float32 [P, R / 2] holding values of `mid_dtype`, `positions`
#    int32 [B] on x's device, read in the kernel: token (b, t) is rotated at the position positions[b] + t, every step rounded to
#    `mid_dtype` -> levels or floats [B, T, H, D].  `lsq_kv_copy_w8` moves x's bytes into `out` [B, Tout, H, D] at those positions (or
#    at t); a token outside `out` is not written.  Inference only.
_ROPE = "Tensor x_levels, Tensor x_scale, Tensor x_zero, Tensor cos, Tensor sin"
_ROPE_POS = "Tensor? positions=None, bool interleaved=False"
_lib_def.define("lsq_rope_w8_q8_q(%s, %s, %s) -> Tensor" % (_ROPE, _ATTN_OUT_Q, _ROPE_POS))
_lib_def.define("lsq_rope_w8_q8(%s, ScalarType out_dtype, %s) -> Tensor" % (_ROPE, _ROPE_POS))
_lib_def.define("lsq_kv_copy_w8(Tensor x_levels, Tensor(a!) out, Tensor? positions=None, bool scatter=True) -> ()")
#  * DECODE ATTENTION on 8-bit LEVELS against a grouped-query KV cache (liblsq_hip_attn_decode_w8.so, include/lsq_hip_attn_decode_w8.h):
#    q [B, H, Tq, D] against k, v [B, Hkv, Tk, D] with Hkv dividing H (query head h reads kv head h // G), the operands and sides of
#    lsq_attention_w8_q8_q and the mask of lsq_softmax_mask_w8_q8_q (`key_lengths`: int32 [B]) -> the context's levels [B, Tq, H D].
#    Keys at or beyond a row's count n take no part and are never read.  One launch where G Tq <= 16, D % 16 == 0, D <= 128,
#    Tk <= 8192 and q, k, v are 16-byte aligned with strides that are multiples of 16; the existing ops composed elsewhere, with
#    the same bytes.  Inference only.
_lib_def.define("lsq_attention_decode_w8_q8_q(Tensor q_levels, Tensor q_scale, Tensor q_zero, Tensor k_levels, Tensor k_scale, "
                "Tensor k_zero, Tensor v_levels, Tensor v_scale, Tensor v_zero, Tensor table, %s, %s, %s, ScalarType mid_dtype, %s) -> Tensor"
                % (tuple(_ATTN_SIDE % ((n,) * 6) for n in ("scores", "probs", "out")) + (_MASK,)))
#  * PREFILL ATTENTION on 8-bit LEVELS (liblsq_hip_attn_prefill_w8.so, include/lsq_hip_attn_prefill_w8.h): the arguments, the definition
#    and the result of lsq_attention_decode_w8_q8_q for ANY number of query rows.  One launch of the decode kernel where G Tq <= 16; one
#    launch of the prefill kernel -- a workgroup per (b, h, 64 rows), nothing above the diagonal computed -- where D % 16 == 0, D <= 128,
#    min(Tk, Tq + causal_offset) (causal; else Tk) <= 2048 and q, k, v are 16-byte aligned with strides that are multiples of 16; the
#    existing ops composed elsewhere, with the same bytes.  Inference only.
_lib_def.define("lsq_attention_prefill_w8_q8_q(Tensor q_levels, Tensor q_scale, Tensor q_zero, Tensor k_levels, Tensor k_scale, "
                "Tensor k_zero, Tensor v_levels, Tensor v_scale, Tensor v_zero, Tensor table, %s, %s, %s, ScalarType mid_dtype, %s) -> Tensor"
                % (tuple(_ATTN_SIDE % ((n,) * 6) for n in ("scores", "probs", "out")) + (_MASK,)))
#  * SPLIT-KEY DECODE ATTENTION on 8-bit LEVELS (liblsq_hip_attn_decode_split_w8.so, include/lsq_hip_attn_decode_split_w8.h): the arguments,
#    the definition and the result of lsq_attention_decode_w8_q8_q plus `splits` -- 0: the library's choice; s >= 1: at most s splits --:
#    one kv head's keys dealt to several workgroups, three launches and a workspace allocated per call, the SAME BYTES for every
#    `splits`.  Served where G Tq <= 16, D % 16 == 0, D <= 128, Tk <= 65536 and q, k, v are 16-byte aligned with strides that are
#    multiples of 16; the existing ops composed elsewhere.  Inference only.
_lib_def.define("lsq_attention_decode_split_w8_q8_q(Tensor q_levels, Tensor q_scale, Tensor q_zero, Tensor k_levels, Tensor k_scale, "
                "Tensor k_zero, Tensor v_levels, Tensor v_scale, Tensor v_zero, Tensor table, %s, %s, %s, ScalarType mid_dtype, %s, "
                "int splits=0) -> Tensor" % (tuple(_ATTN_SIDE % ((n,) * 6) for n in ("scores", "probs", "out")) + (_MASK,)))
#  * The PAGED KV CACHE on 8-bit LEVELS (liblsq_hip_attn_paged_w8.so, include/lsq_hip_attn_paged_w8.h): the arguments and the result of
#    lsq_attention_decode_split_w8_q8_q with the POOLS [Np, Hkv, ps, D] in place of k and v and `block_table` int32 [B, Mp] on their
#    device: key j of batch entry b lies in page clamp(block_table[b, j // ps], 0, Np - 1) at slot j % ps, and the result is
#    lsq_attention_decode_w8_q8_q's on the caches so gathered -- without gathering them where R = G Tq <= 16, D % 16 == 0, D <= 128, ps is
#    a power of two >= 16, Mp ps <= 65536 and q and the pools are 16-byte aligned with strides that are multiples of 16; the gather
#    and the existing ops composed elsewhere, with the same bytes.  `lsq_kv_append_paged_w8` writes a step's k and v [B, T, Hkv, D]
#    into the pools at positions[b] + t in one launch; a token outside the table's capacity or with an entry outside [0, Np) is not
#    written.  Inference only.
_lib_def.define("lsq_attention_decode_paged_w8_q8_q(Tensor q_levels, Tensor q_scale, Tensor q_zero, Tensor k_pool, Tensor k_scale, "
                "Tensor k_zero, Tensor v_pool, Tensor v_scale, Tensor v_zero, Tensor block_table, Tensor table, %s, %s, %s, "
                "ScalarType mid_dtype, %s, int splits=0) -> Tensor"
                % (tuple(_ATTN_SIDE % ((n,) * 6) for n in ("scores", "probs", "out")) + (_MASK,)))
_lib_def.define("lsq_kv_append_paged_w8(Tensor k_levels, Tensor v_levels, Tensor(a!) k_pool, Tensor(b!) v_pool, Tensor block_table, "
                "Tensor? positions=None) -> ()")
#  * CHUNKED PREFILL ATTENTION on 8-bit LEVELS (liblsq_hip_attn_chunk_w8.so, include/lsq_hip_attn_chunk_w8.h): the arguments, the
#    definition and the result of lsq_attention_decode_split_w8_q8_q (and of lsq_attention_decode_paged_w8_q8_q: pools and a block table)
#    for ANY number of query rows, with `causal` an int MODE: 0 off, 1 row t sees t + 1 + causal_offset keys, 2 every row's keys counted
#    back from key_lengths on the device -- n(b, t) = max(0, min(Tk, max(key_lengths[b], 0)) - (Tq - 1 - t)); needs key_lengths and
#    causal_offset 0.  Three launches with the rows of a kv head dealt to row tiles of 16 and a workspace allocated per call where
#    D % 16 == 0, D <= 128, Tk <= 65536 (ps a power of two >= 16) and q, k, v are 16-byte aligned with strides that are multiples of 16;
#    the existing ops composed elsewhere, with the same bytes.  Inference only.
_MASK_MODE = "int causal=0, int causal_offset=0, Tensor? key_lengths=None"
_lib_def.define("lsq_attention_chunk_w8_q8_q(Tensor q_levels, Tensor q_scale, Tensor q_zero, Tensor k_levels, Tensor k_scale, "
                "Tensor k_zero, Tensor v_levels, Tensor v_scale, Tensor v_zero, Tensor table, %s, %s, %s, ScalarType mid_dtype, %s, "
                "int splits=0) -> Tensor" % (tuple(_ATTN_SIDE % ((n,) * 6) for n in ("scores", "probs", "out")) + (_MASK_MODE,)))
_lib_def.define("lsq_attention_chunk_paged_w8_q8_q(Tensor q_levels, Tensor q_scale, Tensor q_zero, Tensor k_pool, Tensor k_scale, "
                "Tensor k_zero, Tensor v_pool, Tensor v_scale, Tensor v_zero, Tensor block_table, Tensor table, %s, %s, %s, "
                "ScalarType mid_dtype, %s, int splits=0) -> Tensor"
                % (tuple(_ATTN_SIDE % ((n,) * 6) for n in ("scores", "probs", "out")) + (_MASK_MODE,)))
#  * THE GATED PRODUCT of a gated MLP on 8-bit LEVELS (liblsq_hip_glu_w8.so, include/lsq_hip_glu_w8.h): gate and up levels of the same
#    shape [.., C], each with innermost stride 1 and one row stride over its leading axes (the halves of a fused linear's [.., 2 C]
#    output are read in place; anything else is made dense first).  `table`: 256 float32 values holding values of `mid_dtype`,
#    indexed by the gate byte as stored (`torchlsq.functional.lsq_glu_table` builds it from existing ops).  a = table[gate byte],
#    d = up dequantized to `mid_dtype`, one rounded product, and the levels of the output quantizer (_q) or the floats themselves,
#    as a new dense [.., C] tensor.  Inference only.
_GLU = "Tensor gate_levels, Tensor up_levels, Tensor up_scale, Tensor up_zero, Tensor table"
_lib_def.define("lsq_glu_w8_q8_q(%s, Tensor out_scale, Tensor out_shift, int out_quant_min, int out_quant_max, int out_type_min, "
                "int out_type_max, ScalarType mid_dtype) -> Tensor" % _GLU)
_lib_def.define("lsq_glu_w8_q8(%s, ScalarType out_dtype) -> Tensor" % _GLU)


# -------------------------------------------------------------------------------------------------
# the HIP backend ("CUDA" dispatch key on ROCm): _hip_host.py
# -------------------------------------------------------------------------------------------------
def _impl_minmax_pt(x):
    return hip_minmax(x, None)


def _impl_minmax_pc(x, axis):
    return hip_minmax(x, axis)


def _impl_meanstd_pt(x):
    return hip_meanstd(x, None)


def _impl_meanstd_pc(x, axis):
    return hip_meanstd(x, axis)


def _impl_fwd_pt(x, scale, shift, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode):
    return hip_forward_per_tensor(x, scale, shift, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode)


def _impl_bwd_pt(grad, x, scale, shift, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode):
    return hip_backward_per_tensor(grad, x, scale, shift, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode,
                                   init_mode)


def _impl_fwd_pc(x, scale, shift, axis, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode):
    return hip_forward_per_channel(x, scale, shift, axis, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode,
                                   init_mode)


def _impl_bwd_pc(grad, x, scale, shift, axis, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode):
    return hip_backward_per_channel(grad, x, scale, shift, axis, qmin, qmax, tmin, tmax, use_gs, gs, sym,
                                    eval_mode, init_mode)


def _impl_bwd_pt_wide(grad, x, scale, shift, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode, n4s):
    return hip_backward_per_tensor(grad, x, scale, shift, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode,
                                   init_mode, numel_for_scaler=n4s, want_wide=True)


def _impl_bwd_pc_wide(grad, x, scale, shift, axis, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode,
                      n4s):
    return hip_backward_per_channel(grad, x, scale, shift, axis, qmin, qmax, tmin, tmax, use_gs, gs, sym,
                                    eval_mode, init_mode, numel_for_scaler=n4s, want_wide=True)


def _impl_quantize_pt(x, scale, shift, qmin, qmax, tmin, tmax, level_bias):
    return hip_forward_per_tensor(x, scale, shift, qmin, qmax, tmin, tmax, True, 1.0, False, False, False,
                                  levels_bias=level_bias)


def _impl_quantize_pc(x, scale, shift, axis, qmin, qmax, tmin, tmax, level_bias):
    return hip_forward_per_channel(x, scale, shift, axis, qmin, qmax, tmin, tmax, True, 1.0, False, False, False,
                                   levels_bias=level_bias)


def _impl_levels_pt(x, scale, shift, qmin, qmax, tmin, tmax, level_bias):
    return hip_forward_per_tensor(x, scale, shift, qmin, qmax, tmin, tmax, True, 1.0, False, False, False,
                                  levels_bias=level_bias, levels_only=True)


def _impl_levels_pc(x, scale, shift, axis, qmin, qmax, tmin, tmax, level_bias):
    return hip_forward_per_channel(x, scale, shift, axis, qmin, qmax, tmin, tmax, True, 1.0, False, False, False,
                                   levels_bias=level_bias, levels_only=True)


_lib_hip = torch.library.Library("torchlsq", "IMPL", "CUDA")
_lib_hip.impl("lsq_levels_per_tensor", _impl_levels_pt)
_lib_hip.impl("lsq_levels_per_channel", _impl_levels_pc)
_lib_hip.impl("lsq_forward_per_tensor", _impl_fwd_pt)
_lib_hip.impl("lsq_backward_per_tensor", _impl_bwd_pt)
_lib_hip.impl("lsq_forward_per_channel", _impl_fwd_pc)
_lib_hip.impl("lsq_backward_per_channel", _impl_bwd_pc)
_lib_hip.impl("lsq_backward_per_tensor_wide", _impl_bwd_pt_wide)
_lib_hip.impl("lsq_backward_per_channel_wide", _impl_bwd_pc_wide)
_lib_hip.impl("lsq_quantize_per_tensor", _impl_quantize_pt)
_lib_hip.impl("lsq_quantize_per_channel", _impl_quantize_pc)
_lib_hip.impl("lsq_backward_from_mask", hip_backward_from_mask)
_lib_hip.impl("lsq_minmax_per_tensor", _impl_minmax_pt)
_lib_hip.impl("lsq_minmax_per_channel", _impl_minmax_pc)
_lib_hip.impl("lsq_meanstd_per_tensor", _impl_meanstd_pt)
_lib_hip.impl("lsq_meanstd_per_channel", _impl_meanstd_pc)



# the CPU backend ("CPU" dispatch key): _cpu_host.py
_lib_cpu = torch.library.Library("torchlsq", "IMPL", "CPU")
_lib_cpu.impl("lsq_forward_per_tensor", lambda x, s, b, *a: cpu_forward(x, s, b, 0, False, *a))
_lib_cpu.impl("lsq_backward_per_tensor", lambda g, x, s, b, *a: cpu_backward(g, x, s, b, 0, False, *a))
_lib_cpu.impl("lsq_forward_per_channel", lambda x, s, b, axis, *a: cpu_forward(x, s, b, axis, True, *a))
_lib_cpu.impl("lsq_backward_per_channel", lambda g, x, s, b, axis, *a: cpu_backward(g, x, s, b, axis, True, *a))
_lib_cpu.impl("lsq_backward_per_tensor_wide",
              lambda g, x, s, b, *a: cpu_backward(g, x, s, b, 0, False, *a[:-1], numel_for_scaler=a[-1], want_wide=True))
_lib_cpu.impl("lsq_backward_per_channel_wide",
              lambda g, x, s, b, axis, *a: cpu_backward(g, x, s, b, axis, True, *a[:-1], numel_for_scaler=a[-1], want_wide=True))
_lib_cpu.impl("lsq_levels_per_tensor", lambda x, s, b, *a: cpu_levels(x, s, b, 0, False, *a))
_lib_cpu.impl("lsq_levels_per_channel", lambda x, s, b, axis, *a: cpu_levels(x, s, b, axis, True, *a))
_lib_cpu.impl("lsq_minmax_per_tensor", lambda x: _cpu_minmax(x))
_lib_cpu.impl("lsq_minmax_per_channel", lambda x, axis: _cpu_minmax(x, axis))
_lib_cpu.impl("lsq_meanstd_per_tensor", lambda x: _cpu_meanstd(x))
_lib_cpu.impl("lsq_meanstd_per_channel", lambda x, axis: _cpu_meanstd(x, axis))


# -------------------------------------------------------------------------------------------------
# shape-only ("meta") kernels so the ops trace under torch.compile / FakeTensor
# -------------------------------------------------------------------------------------------------
def _meta_like(x):
    return torch.empty_like(x)


@torch.library.register_fake("torchlsq::lsq_forward_per_tensor", lib=_lib_def)
def _fake_fwd_pt(x, scale, shift, *a):
    return _meta_like(x)


@torch.library.register_fake("torchlsq::lsq_forward_per_channel", lib=_lib_def)
def _fake_fwd_pc(x, scale, shift, axis, *a):
    return _meta_like(x)


@torch.library.register_fake("torchlsq::lsq_backward_per_tensor", lib=_lib_def)
def _fake_bwd_pt(grad, x, scale, shift, *a):
    return _meta_like(x), scale.new_empty((1,)), shift.new_empty((1,))


@torch.library.register_fake("torchlsq::lsq_backward_per_channel", lib=_lib_def)
def _fake_bwd_pc(grad, x, scale, shift, axis, *a):
    return _meta_like(x), torch.empty_like(scale), torch.empty_like(shift)


@torch.library.register_fake("torchlsq::lsq_backward_per_tensor_wide", lib=_lib_def)
def _fake_bwd_pt_wide(grad, x, scale, shift, *a):
    return _meta_like(x), x.new_empty((2,), dtype=torch.float64)


@torch.library.register_fake("torchlsq::lsq_backward_per_channel_wide", lib=_lib_def)
def _fake_bwd_pc_wide(grad, x, scale, shift, axis, *a):
    return _meta_like(x), x.new_empty((2, scale.numel()), dtype=torch.float64)


@torch.library.register_fake("torchlsq::lsq_quantize_per_tensor", lib=_lib_def)
def _fake_quantize_pt(x, scale, shift, *a):
    return _meta_like(x), torch.empty_like(x, dtype=torch.int8)


@torch.library.register_fake("torchlsq::lsq_quantize_per_channel", lib=_lib_def)
def _fake_quantize_pc(x, scale, shift, axis, *a):
    return _meta_like(x), torch.empty_like(x, dtype=torch.int8)


@torch.library.register_fake("torchlsq::lsq_levels_per_tensor", lib=_lib_def)
def _fake_levels_pt(x, scale, shift, *a):
    return torch.empty_like(x, dtype=torch.int8)


@torch.library.register_fake("torchlsq::lsq_levels_per_channel", lib=_lib_def)
def _fake_levels_pc(x, scale, shift, axis, *a):
    return torch.empty_like(x, dtype=torch.int8)


@torch.library.register_fake("torchlsq::lsq_backward_from_mask", lib=_lib_def)
def _fake_bwd_mask(grad, mask):
    return torch.empty_strided(mask.shape, mask.stride(), dtype=grad.dtype, device=grad.device)


@torch.library.register_fake("torchlsq::lsq_minmax_per_tensor", lib=_lib_def)
def _fake_minmax_pt(x):
    pd = _param_dtype(x)
    return x.new_empty((), dtype=pd), x.new_empty((), dtype=pd)


@torch.library.register_fake("torchlsq::lsq_minmax_per_channel", lib=_lib_def)
def _fake_minmax_pc(x, axis):
    pd = _param_dtype(x)
    return x.new_empty((x.size(axis),), dtype=pd), x.new_empty((x.size(axis),), dtype=pd)


torch.library.register_fake("torchlsq::lsq_meanstd_per_tensor", _fake_minmax_pt, lib=_lib_def)
torch.library.register_fake("torchlsq::lsq_meanstd_per_channel", _fake_minmax_pc, lib=_lib_def)


# -------------------------------------------------------------------------------------------------
# autograd (restates lsq_autograd.cpp: forward saves {input, scale, shift} + the scalars, backward
# calls the backward op through the dispatcher and returns grads for the three tensors only)
# -------------------------------------------------------------------------------------------------
def _setup_pt(ctx, inputs, output):
    x, scale, shift = inputs[:3]
    ctx.save_for_backward(x, scale, shift)
    ctx.lsq_scalars = tuple(inputs[3:])


def _backward_pt(ctx, grad_out):
    x, scale, shift = ctx.saved_tensors
    dx, ds, db = torch.ops.torchlsq.lsq_backward_per_tensor(grad_out, x, scale, shift, *ctx.lsq_scalars)
    return (dx, ds, db) + (None,) * 9      # lsq_autograd.cpp:69-71


def _setup_pc(ctx, inputs, output):
    x, scale, shift = inputs[:3]
    ctx.save_for_backward(x, scale, shift)
    ctx.lsq_scalars = tuple(inputs[3:])  # axis first


def _backward_pc(ctx, grad_out):
    x, scale, shift = ctx.saved_tensors
    dx, ds, db = torch.ops.torchlsq.lsq_backward_per_channel(grad_out, x, scale, shift, *ctx.lsq_scalars)
    return (dx, ds, db) + (None,) * 10     # lsq_autograd.cpp:169-170


torch.library.register_autograd("torchlsq::lsq_forward_per_tensor", _backward_pt, setup_context=_setup_pt,
                                lib=_lib_def)
torch.library.register_autograd("torchlsq::lsq_forward_per_channel", _backward_pc, setup_context=_setup_pc,
                                lib=_lib_def)


def _no_double_backward(name):
    def bw(ctx, *grads):
        raise RuntimeError("double backwards on %s not supported" % name)  # lsq_autograd.cpp:106,208
    return bw


for _op, _nm in (("lsq_backward_per_tensor", "lsq_per_tensor"), ("lsq_backward_per_channel", "lsq_per_channel"),
                 ("lsq_backward_per_tensor_wide", "lsq_per_tensor"),
                 ("lsq_backward_per_channel_wide", "lsq_per_channel")):
    torch.library.register_autograd("torchlsq::" + _op, _no_double_backward(_nm), lib=_lib_def)


# -------------------------------------------------------------------------------------------------
# the group-wise ops (_group_host.py): GPU tensors -> liblsq_hip_group.so, CPU tensors -> liblsq_cpu.so's per-channel
# kernels on the [numel // G, G] view; shape-only kernels; autograd with the same double-backward refusal
# -------------------------------------------------------------------------------------------------
def _impl_fwd_grp(x, scale, shift, group_size, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode):
    return group_forward(x, scale, shift, group_size, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode)


def _impl_bwd_grp(grad, x, scale, shift, group_size, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode):
    return group_backward(grad, x, scale, shift, group_size, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode)


def _impl_levels_grp(x, scale, shift, group_size, qmin, qmax, tmin, tmax, level_bias):
    return group_forward(x, scale, shift, group_size, qmin, qmax, tmin, tmax, True, 1.0, False, False, False,
                         levels_bias=level_bias, levels_only=True)


for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_forward_per_group", _impl_fwd_grp)
    _lib_key.impl("lsq_backward_per_group", _impl_bwd_grp)
    _lib_key.impl("lsq_levels_per_group", _impl_levels_grp)
del _lib_key


@torch.library.register_fake("torchlsq::lsq_forward_per_group", lib=_lib_def)
def _fake_fwd_grp(x, scale, shift, group_size, *a):
    return torch.empty(x.shape, dtype=x.dtype, device=x.device)


@torch.library.register_fake("torchlsq::lsq_backward_per_group", lib=_lib_def)
def _fake_bwd_grp(grad, x, scale, shift, group_size, *a):
    pd = _param_dtype(x)
    return (torch.empty(x.shape, dtype=x.dtype, device=x.device), torch.empty(scale.shape, dtype=pd, device=x.device),
            torch.empty(shift.shape, dtype=pd, device=x.device))


@torch.library.register_fake("torchlsq::lsq_levels_per_group", lib=_lib_def)
def _fake_levels_grp(x, scale, shift, group_size, *a):
    return torch.empty(x.shape, dtype=torch.int8, device=x.device)


def _setup_grp(ctx, inputs, output):
    x, scale, shift = inputs[:3]
    ctx.save_for_backward(x, scale, shift)
    ctx.lsq_scalars = tuple(inputs[3:])  # group_size first


def _backward_grp(ctx, grad_out):
    x, scale, shift = ctx.saved_tensors
    dx, ds, db = torch.ops.torchlsq.lsq_backward_per_group(grad_out, x, scale, shift, *ctx.lsq_scalars)
    return (dx, ds, db) + (None,) * 10


torch.library.register_autograd("torchlsq::lsq_forward_per_group", _backward_grp, setup_context=_setup_grp, lib=_lib_def)
torch.library.register_autograd("torchlsq::lsq_backward_per_group", _no_double_backward("lsq_per_group"), lib=_lib_def)


# -------------------------------------------------------------------------------------------------
# the packed export ops (_pack_host.py): GPU tensors -> liblsq_hip_pack.so, CPU tensors -> cpu_levels + torch integer ops;
# shape-only kernels.  Conversion-time ops on detached values: no autograd.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_pack_per_group", pack_quantize)
    _lib_key.impl("lsq_unpack_per_group", pack_unpack)
    _lib_key.impl("lsq_dequantize_per_group", pack_dequantize)
del _lib_key


@torch.library.register_fake("torchlsq::lsq_pack_per_group", lib=_lib_def)
def _fake_pack_grp(x, scale, shift, group_size, bits, *a):
    return (torch.empty(x.shape[:-1] + (x.shape[-1] * bits // 8,), dtype=torch.uint8, device=x.device),
            torch.empty(scale.shape, dtype=_param_dtype(x), device=x.device),
            torch.empty(scale.shape, dtype=torch.int32, device=x.device))


@torch.library.register_fake("torchlsq::lsq_unpack_per_group", lib=_lib_def)
def _fake_unpack_grp(codes, bits, *a):
    return torch.empty(codes.shape[:-1] + (codes.shape[-1] * (8 // bits),), dtype=torch.int8, device=codes.device)


@torch.library.register_fake("torchlsq::lsq_dequantize_per_group", lib=_lib_def)
def _fake_dequantize_grp(codes, scale, zero_point, group_size, bits, dtype):
    return torch.empty(codes.shape[:-1] + (codes.shape[-1] * (8 // bits),), dtype=dtype, device=codes.device)


# -------------------------------------------------------------------------------------------------
# the linear op on packed weights (_qlinear_host.py): GPU tensors -> liblsq_hip_qlinear.so (up to 16 rows of x), more rows ->
# liblsq_hip_qgemm.so (16-bit x on the formats it serves; else dequantize and call F.linear), CPU tensors -> torch; a shape-only kernel.  Inference only: the autograd key refuses an x
# (or bias) that wants a gradient instead of cutting the graph without a word.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_linear_packed", qlinear_forward)
del _lib_key


@torch.library.register_fake("torchlsq::lsq_linear_packed", lib=_lib_def)
def _fake_linear_packed(x, codes, scale, zero_point, bias, group_size, bits):
    return torch.empty(x.shape[:-1] + (codes.shape[0],), dtype=x.dtype, device=x.device)


def _linear_packed_no_grad(x, codes, scale, zero_point, bias, group_size, bits):
    if torch.is_grad_enabled() and (x.requires_grad or (bias is not None and bias.requires_grad)):
        raise RuntimeError("lsq_linear_packed is inference-only: x (or the bias) requires grad.  Run it under torch.no_grad() "
                           "or detach the input; train with the fake-quantized layer (lsq_per_group), not with packed codes")
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.torchlsq.lsq_linear_packed(x, codes, scale, zero_point, bias, group_size, bits)


_lib_def.impl("lsq_linear_packed", _linear_packed_no_grad, "Autograd")


# -------------------------------------------------------------------------------------------------
# the 8-bit-activation linear ops on packed weights (_qlinear_a8_host.py): GPU tensors -> liblsq_hip_qlinear_a8.so (16 rows
# a launch; more rows are one launch per block of 16), CPU tensors -> torch int64 products; a
# shape-only kernel each.  Inference only, like lsq_linear_packed.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_linear_packed_q8", qlinear_a8_forward_levels)
    _lib_key.impl("lsq_linear_packed_a8", qlinear_a8_forward)
del _lib_key


@torch.library.register_fake("torchlsq::lsq_linear_packed_q8", lib=_lib_def)
def _fake_linear_packed_q8(x_levels, s_x, zx, codes, scale, zero_point, bias, group_size, bits, out_dtype):
    return torch.empty(x_levels.shape[:-1] + (codes.shape[0],), dtype=out_dtype, device=x_levels.device)


@torch.library.register_fake("torchlsq::lsq_linear_packed_a8", lib=_lib_def)
def _fake_linear_packed_a8(x, act_scale, act_shift, quant_min, quant_max, type_min, type_max, codes, scale, zero_point, bias,
                           group_size, bits):
    return torch.empty(x.shape[:-1] + (codes.shape[0],), dtype=x.dtype, device=x.device)


def _refuse_grad(what, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("%s is inference-only: an input requires grad.  Run it under torch.no_grad() or detach the input; "
                           "train with the fake-quantized layers, not with packed codes and integer levels" % what)


def _linear_packed_q8_no_grad(x_levels, s_x, zx, codes, scale, zero_point, bias, group_size, bits, out_dtype):
    _refuse_grad("lsq_linear_packed_q8", s_x, bias)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.torchlsq.lsq_linear_packed_q8(x_levels, s_x, zx, codes, scale, zero_point, bias, group_size, bits, out_dtype)


def _linear_packed_a8_no_grad(x, act_scale, act_shift, quant_min, quant_max, type_min, type_max, codes, scale, zero_point, bias,
                              group_size, bits):
    _refuse_grad("lsq_linear_packed_a8", x, act_scale, act_shift, bias)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.torchlsq.lsq_linear_packed_a8(x, act_scale, act_shift, quant_min, quant_max, type_min, type_max, codes,
                                                       scale, zero_point, bias, group_size, bits)


_lib_def.impl("lsq_linear_packed_q8", _linear_packed_q8_no_grad, "Autograd")
_lib_def.impl("lsq_linear_packed_a8", _linear_packed_a8_no_grad, "Autograd")


# -------------------------------------------------------------------------------------------------
# the W8A8 linear ops on per-channel weight levels (_qlinear_w8_host.py): GPU tensors -> liblsq_hip_qlinear_w8.so (one call,
# any number of rows), CPU tensors -> one torch int64 product; a shape-only kernel each.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_linear_w8_q8", qlinear_w8_forward_levels)
    _lib_key.impl("lsq_linear_w8_a8", qlinear_w8_forward)
del _lib_key


@torch.library.register_fake("torchlsq::lsq_linear_w8_q8", lib=_lib_def)
def _fake_linear_w8_q8(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_dtype):
    return torch.empty(x_levels.shape[:-1] + (w_levels.shape[0],), dtype=out_dtype, device=x_levels.device)


@torch.library.register_fake("torchlsq::lsq_linear_w8_a8", lib=_lib_def)
def _fake_linear_w8_a8(x, act_scale, act_shift, quant_min, quant_max, type_min, type_max, w_levels, w_scale, w_zero, bias):
    return torch.empty(x.shape[:-1] + (w_levels.shape[0],), dtype=x.dtype, device=x.device)


def _linear_w8_q8_no_grad(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_dtype):
    _refuse_grad("lsq_linear_w8_q8", s_x, w_scale, bias)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.torchlsq.lsq_linear_w8_q8(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_dtype)


def _linear_w8_a8_no_grad(x, act_scale, act_shift, quant_min, quant_max, type_min, type_max, w_levels, w_scale, w_zero, bias):
    _refuse_grad("lsq_linear_w8_a8", x, act_scale, act_shift, w_scale, bias)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.torchlsq.lsq_linear_w8_a8(x, act_scale, act_shift, quant_min, quant_max, type_min, type_max, w_levels,
                                                   w_scale, w_zero, bias)


_lib_def.impl("lsq_linear_w8_q8", _linear_w8_q8_no_grad, "Autograd")
_lib_def.impl("lsq_linear_w8_a8", _linear_w8_a8_no_grad, "Autograd")


# -------------------------------------------------------------------------------------------------
# the W8A8 conv2d ops (_qconv_w8_host.py): GPU tensors -> liblsq_hip_qconv_w8.so (one call), CPU tensors -> one torch int64
# convolution; a shape-only kernel each, which also gives the channels-last memory format.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_conv2d_w8_q8", qconv_w8_forward_levels)
    _lib_key.impl("lsq_conv2d_w8_a8", qconv_w8_forward)
del _lib_key


def _fake_conv2d_w8(x, w_levels, stride, padding, dilation, dtype):
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    oh = (x.shape[2] + 2 * ph - dh * (w_levels.shape[2] - 1) - 1) // sh + 1
    ow = (x.shape[3] + 2 * pw - dw * (w_levels.shape[3] - 1) - 1) // sw + 1
    return torch.empty((x.shape[0], w_levels.shape[0], oh, ow), dtype=dtype, device=x.device, memory_format=torch.channels_last)


@torch.library.register_fake("torchlsq::lsq_conv2d_w8_q8", lib=_lib_def)
def _fake_conv2d_w8_q8(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, out_dtype):
    return _fake_conv2d_w8(x_levels, w_levels, stride, padding, dilation, out_dtype)


@torch.library.register_fake("torchlsq::lsq_conv2d_w8_a8", lib=_lib_def)
def _fake_conv2d_w8_a8(x, act_scale, act_shift, quant_min, quant_max, type_min, type_max, w_levels, w_scale, w_zero, bias, stride,
                       padding, dilation):
    return _fake_conv2d_w8(x, w_levels, stride, padding, dilation, x.dtype)


def _conv2d_w8_q8_no_grad(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, out_dtype):
    _refuse_grad("lsq_conv2d_w8_q8", s_x, w_scale, bias)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.torchlsq.lsq_conv2d_w8_q8(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation,
                                                   out_dtype)


def _conv2d_w8_a8_no_grad(x, act_scale, act_shift, quant_min, quant_max, type_min, type_max, w_levels, w_scale, w_zero, bias, stride,
                          padding, dilation):
    _refuse_grad("lsq_conv2d_w8_a8", x, act_scale, act_shift, w_scale, bias)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.torchlsq.lsq_conv2d_w8_a8(x, act_scale, act_shift, quant_min, quant_max, type_min, type_max, w_levels,
                                                   w_scale, w_zero, bias, stride, padding, dilation)


_lib_def.impl("lsq_conv2d_w8_q8", _conv2d_w8_q8_no_grad, "Autograd")
_lib_def.impl("lsq_conv2d_w8_a8", _conv2d_w8_a8_no_grad, "Autograd")


# -------------------------------------------------------------------------------------------------
# the W8A8 ops with an 8-bit output (_requant_w8_host.py): GPU tensors -> liblsq_hip_requant_w8.so (one call), CPU tensors ->
# the composition of the ops above that defines them; a shape-only kernel each.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_linear_w8_q8_q", requant_w8_linear_levels)
    _lib_key.impl("lsq_linear_w8_a8_q", requant_w8_linear)
    _lib_key.impl("lsq_conv2d_w8_q8_q", requant_w8_conv_levels)
    _lib_key.impl("lsq_conv2d_w8_a8_q", requant_w8_conv)
del _lib_key


def _fake_level_dtype(quant_max, type_max):
    return torch.uint8 if max(quant_max, type_max) > 127 else torch.int8


@torch.library.register_fake("torchlsq::lsq_linear_w8_q8_q", lib=_lib_def)
def _fake_linear_w8_q8_q(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_scale, out_shift, out_quant_min, out_quant_max,
                         out_type_min, out_type_max, relu, mid_dtype):
    return torch.empty(x_levels.shape[:-1] + (w_levels.shape[0],), dtype=_fake_level_dtype(out_quant_max, out_type_max),
                       device=x_levels.device)


@torch.library.register_fake("torchlsq::lsq_linear_w8_a8_q", lib=_lib_def)
def _fake_linear_w8_a8_q(x, act_scale, act_shift, quant_min, quant_max, type_min, type_max, w_levels, w_scale, w_zero, bias, out_scale,
                         out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, relu):
    return torch.empty(x.shape[:-1] + (w_levels.shape[0],), dtype=_fake_level_dtype(out_quant_max, out_type_max), device=x.device)


@torch.library.register_fake("torchlsq::lsq_conv2d_w8_q8_q", lib=_lib_def)
def _fake_conv2d_w8_q8_q(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, out_scale, out_shift,
                         out_quant_min, out_quant_max, out_type_min, out_type_max, relu, mid_dtype):
    return _fake_conv2d_w8(x_levels, w_levels, stride, padding, dilation, _fake_level_dtype(out_quant_max, out_type_max))


@torch.library.register_fake("torchlsq::lsq_conv2d_w8_a8_q", lib=_lib_def)
def _fake_conv2d_w8_a8_q(x, act_scale, act_shift, quant_min, quant_max, type_min, type_max, w_levels, w_scale, w_zero, bias, stride,
                         padding, dilation, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, relu):
    return _fake_conv2d_w8(x, w_levels, stride, padding, dilation, _fake_level_dtype(out_quant_max, out_type_max))


def _requant_no_grad(name, grad_args):
    """the Autograd kernel of an inference-only op: refuses an input that requires grad (`grad_args`: positions of the floating
    tensors among the arguments), then dispatches below autograd"""
    def kernel(*args):
        _refuse_grad(name, *(args[i] for i in grad_args))
        with torch._C._AutoDispatchBelowAutograd():
            return getattr(torch.ops.torchlsq, name)(*args)
    return kernel


_lib_def.impl("lsq_linear_w8_q8_q", _requant_no_grad("lsq_linear_w8_q8_q", (1, 4, 6, 7, 8)), "Autograd")
_lib_def.impl("lsq_linear_w8_a8_q", _requant_no_grad("lsq_linear_w8_a8_q", (0, 1, 2, 8, 10, 11, 12)), "Autograd")
_lib_def.impl("lsq_conv2d_w8_q8_q", _requant_no_grad("lsq_conv2d_w8_q8_q", (1, 4, 6, 10, 11)), "Autograd")
_lib_def.impl("lsq_conv2d_w8_a8_q", _requant_no_grad("lsq_conv2d_w8_a8_q", (0, 1, 2, 8, 10, 14, 15)), "Autograd")


# -------------------------------------------------------------------------------------------------
# the W8A8 ops that add a levels residual in the 8-bit epilogue (_resadd_w8_host.py): GPU tensors -> liblsq_hip_resadd_w8.so (one
# call), CPU tensors -> the composition of the ops above that defines them; a shape-only kernel each.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_linear_w8_q8_add_q", resadd_w8_linear_levels)
    _lib_key.impl("lsq_conv2d_w8_q8_add_q", resadd_w8_conv_levels)
del _lib_key


@torch.library.register_fake("torchlsq::lsq_linear_w8_q8_add_q", lib=_lib_def)
def _fake_linear_w8_q8_add_q(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_scale, out_shift, out_quant_min, out_quant_max,
                             out_type_min, out_type_max, relu, mid_dtype, res_levels, res_scale, res_zero, pre_scale, pre_shift,
                             pre_quant_min, pre_quant_max, pre_type_min, pre_type_max):
    return torch.empty(x_levels.shape[:-1] + (w_levels.shape[0],), dtype=_fake_level_dtype(out_quant_max, out_type_max),
                       device=x_levels.device)


@torch.library.register_fake("torchlsq::lsq_conv2d_w8_q8_add_q", lib=_lib_def)
def _fake_conv2d_w8_q8_add_q(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, out_scale, out_shift,
                             out_quant_min, out_quant_max, out_type_min, out_type_max, relu, mid_dtype, res_levels, res_scale, res_zero,
                             pre_scale, pre_shift, pre_quant_min, pre_quant_max, pre_type_min, pre_type_max):
    return _fake_conv2d_w8(x_levels, w_levels, stride, padding, dilation, _fake_level_dtype(out_quant_max, out_type_max))


_lib_def.impl("lsq_linear_w8_q8_add_q", _requant_no_grad("lsq_linear_w8_q8_add_q", (1, 4, 6, 7, 8, 16, 18, 19)), "Autograd")
_lib_def.impl("lsq_conv2d_w8_q8_add_q", _requant_no_grad("lsq_conv2d_w8_q8_add_q", (1, 4, 6, 10, 11, 19, 21, 22)), "Autograd")


# -------------------------------------------------------------------------------------------------
# pooling on 8-bit levels (_pool_w8_host.py): GPU tensors -> liblsq_hip_pool_w8.so (one call), CPU tensors -> the definition in
# torch ops; a shape-only kernel each.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_max_pool2d_q8", pool_w8_max)
    _lib_key.impl("lsq_avg_pool2d_q8_q", pool_w8_avg_q)
    _lib_key.impl("lsq_avg_pool2d_q8", pool_w8_avg)
del _lib_key


def _fake_pool_w8(levels, kernel_size, stride, padding, dilation, ceil_mode, dtype):
    def extent(n, k, s, p, d):
        num = n + 2 * p - d * (k - 1) - 1
        out = (-(-num // s) if ceil_mode else num // s) + 1
        return out - 1 if ceil_mode and (out - 1) * s >= n + p else out
    B, C, H, W = levels.shape
    return torch.empty((B, C, extent(H, kernel_size[0], stride[0], padding[0], dilation[0]),
                        extent(W, kernel_size[1], stride[1], padding[1], dilation[1])), dtype=dtype, device=levels.device,
                       memory_format=torch.channels_last)


@torch.library.register_fake("torchlsq::lsq_max_pool2d_q8", lib=_lib_def)
def _fake_max_pool2d_q8(levels, kernel_size, stride, padding, dilation, ceil_mode):
    return _fake_pool_w8(levels, kernel_size, stride, padding, dilation, ceil_mode, levels.dtype)


@torch.library.register_fake("torchlsq::lsq_avg_pool2d_q8_q", lib=_lib_def)
def _fake_avg_pool2d_q8_q(levels, x_scale, x_zero, kernel_size, stride, padding, ceil_mode, count_include_pad, divisor_override,
                          out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, mid_dtype):
    return _fake_pool_w8(levels, kernel_size, stride, padding, (1, 1), ceil_mode, _fake_level_dtype(out_quant_max, out_type_max))


@torch.library.register_fake("torchlsq::lsq_avg_pool2d_q8", lib=_lib_def)
def _fake_avg_pool2d_q8(levels, x_scale, x_zero, kernel_size, stride, padding, ceil_mode, count_include_pad, divisor_override, out_dtype):
    return _fake_pool_w8(levels, kernel_size, stride, padding, (1, 1), ceil_mode, out_dtype)


_lib_def.impl("lsq_max_pool2d_q8", _requant_no_grad("lsq_max_pool2d_q8", ()), "Autograd")
_lib_def.impl("lsq_avg_pool2d_q8_q", _requant_no_grad("lsq_avg_pool2d_q8_q", (1, 9, 10)), "Autograd")
_lib_def.impl("lsq_avg_pool2d_q8", _requant_no_grad("lsq_avg_pool2d_q8", (1,)), "Autograd")


# -------------------------------------------------------------------------------------------------
# the W8A8 depthwise conv2d on 8-bit levels (_dwconv_w8_host.py): GPU tensors -> liblsq_hip_dwconv_w8.so (one call), CPU tensors
# -> the definition in torch ops; a shape-only kernel each.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_dwconv2d_w8_q8_q", dwconv_w8_levels_q)
    _lib_key.impl("lsq_dwconv2d_w8_q8", dwconv_w8_levels)
del _lib_key


def _fake_dwconv_w8(x_levels, w_levels, stride, padding, dilation, dtype):
    B, C, H, W = x_levels.shape
    kh, kw = w_levels.shape[:2]
    OH = (H + 2 * padding[0] - dilation[0] * (kh - 1) - 1) // stride[0] + 1
    OW = (W + 2 * padding[1] - dilation[1] * (kw - 1) - 1) // stride[1] + 1
    return torch.empty((B, C, OH, OW), dtype=dtype, device=x_levels.device, memory_format=torch.channels_last)


@torch.library.register_fake("torchlsq::lsq_dwconv2d_w8_q8_q", lib=_lib_def)
def _fake_dwconv2d_w8_q8_q(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, out_scale, out_shift,
                           out_quant_min, out_quant_max, out_type_min, out_type_max, act, mid_dtype):
    return _fake_dwconv_w8(x_levels, w_levels, stride, padding, dilation, _fake_level_dtype(out_quant_max, out_type_max))


@torch.library.register_fake("torchlsq::lsq_dwconv2d_w8_q8", lib=_lib_def)
def _fake_dwconv2d_w8_q8(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, act, out_dtype):
    return _fake_dwconv_w8(x_levels, w_levels, stride, padding, dilation, out_dtype)


_lib_def.impl("lsq_dwconv2d_w8_q8_q", _requant_no_grad("lsq_dwconv2d_w8_q8_q", (1, 4, 6, 10, 11)), "Autograd")
_lib_def.impl("lsq_dwconv2d_w8_q8", _requant_no_grad("lsq_dwconv2d_w8_q8", (1, 4, 6)), "Autograd")


# -------------------------------------------------------------------------------------------------
# the table op and the gate multiply on 8-bit levels (_eltwise_w8_host.py): GPU tensors -> liblsq_hip_eltwise_w8.so (one call), CPU
# tensors -> the definition in torch ops; a shape-only kernel each.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_lut_w8", eltwise_w8_lut)
    _lib_key.impl("lsq_mul_gate_w8_q8_q", eltwise_w8_mul_gate_q)
    _lib_key.impl("lsq_mul_gate_w8_q8", eltwise_w8_mul_gate)
del _lib_key


def _fake_like_levels(x_levels, dtype):
    fmt = torch.channels_last if x_levels.dim() == 4 else torch.contiguous_format
    return torch.empty(x_levels.shape, dtype=dtype, device=x_levels.device, memory_format=fmt)


@torch.library.register_fake("torchlsq::lsq_lut_w8", lib=_lib_def)
def _fake_lut_w8(x_levels, table, out_dtype):
    return torch.empty_like(x_levels, dtype=out_dtype)


@torch.library.register_fake("torchlsq::lsq_mul_gate_w8_q8_q", lib=_lib_def)
def _fake_mul_gate_w8_q8_q(x_levels, x_scale, x_zero, g_levels, g_scale, g_zero, out_scale, out_shift, out_quant_min, out_quant_max,
                           out_type_min, out_type_max, mid_dtype):
    return _fake_like_levels(x_levels, _fake_level_dtype(out_quant_max, out_type_max))


@torch.library.register_fake("torchlsq::lsq_mul_gate_w8_q8", lib=_lib_def)
def _fake_mul_gate_w8_q8(x_levels, x_scale, x_zero, g_levels, g_scale, g_zero, out_dtype):
    return _fake_like_levels(x_levels, out_dtype)


_lib_def.impl("lsq_lut_w8", _requant_no_grad("lsq_lut_w8", ()), "Autograd")
_lib_def.impl("lsq_mul_gate_w8_q8_q", _requant_no_grad("lsq_mul_gate_w8_q8_q", (1, 4, 6, 7)), "Autograd")
_lib_def.impl("lsq_mul_gate_w8_q8", _requant_no_grad("lsq_mul_gate_w8_q8", (1, 4)), "Autograd")


# -------------------------------------------------------------------------------------------------
# composite front op (restates quantops::ops::lsq, lsq.cpp:104-134) and _cuda_version
# -------------------------------------------------------------------------------------------------
def _lsq_front(x, scale, shift, quant_min, quant_max, type_min, type_max, axis, use_grad_scaling, grad_scale,
               is_affine, is_perchannel, eval_mode, init_mode):
    _check(scale.dim() == 1,
           "scale should be a 1-D tensor, even in per tensor case(please, avoid torch.Scalar too)")
    _check(shift.dim() == 1,
           "shift should be a 1-D tensor, even in per tensor case(please, avoid torch.Scalar too)")
    sym = not is_affine
    if is_perchannel:
        # a size-1 parameter is repeated up to the larger size; `repeat` is differentiable, so the
        # size-1 leaf still receives the summed gradient (lsq.cpp:124-126)
        size = max(scale.size(0), shift.size(0))
        _scale = scale if scale.size(0) == size else scale.repeat(size)
        _shift = shift if shift.size(0) == size else shift.repeat(size)
        return torch.ops.torchlsq.lsq_forward_per_channel(x, _scale, _shift, axis, quant_min, quant_max, type_min,
                                                          type_max, use_grad_scaling, grad_scale, sym, eval_mode,
                                                          init_mode)
    return torch.ops.torchlsq.lsq_forward_per_tensor(x, scale, shift, quant_min, quant_max, type_min, type_max,
                                                     use_grad_scaling, grad_scale, sym, eval_mode, init_mode)


_lib_def.impl("lsq", _lsq_front, "CompositeImplicitAutograd")


def _runtime_version():
    """torchlsq::_cuda_version of this build: the HIP_VERSION the kernels were compiled with, or -1
    when the native library is missing (reference torchlsq.cpp:25-31 returns CUDA_VERSION / -1)."""
    return int(_abi._LIB.lsq_hip_runtime_version()) if _abi._HAS_OPS else -1


_lib_def.impl("_cuda_version", _runtime_version, "CompositeExplicitAutograd")

_check_hip_version()


# -------------------------------------------------------------------------------------------------
# LayerNorm and RMSNorm on 8-bit levels (_norm_w8_host.py): GPU tensors -> liblsq_hip_norm_w8.so (one call), CPU tensors -> the
# definition in torch ops; a shape-only kernel each.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_layer_norm_w8_q8_q", norm_w8_layer_q)
    _lib_key.impl("lsq_layer_norm_w8_q8", norm_w8_layer)
    _lib_key.impl("lsq_rms_norm_w8_q8_q", norm_w8_rms_q)
    _lib_key.impl("lsq_rms_norm_w8_q8", norm_w8_rms)
del _lib_key


def _fake_norm_w8_q(x_levels, x_scale, x_zero, weight, bias, eps, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min,
                    out_type_max, mid_dtype):
    return torch.empty(x_levels.shape, dtype=_fake_level_dtype(out_quant_max, out_type_max), device=x_levels.device)


def _fake_norm_w8(x_levels, x_scale, x_zero, weight, bias, eps, out_dtype):
    return torch.empty(x_levels.shape, dtype=out_dtype, device=x_levels.device)


for _norm_name in ("lsq_layer_norm_w8_q8", "lsq_rms_norm_w8_q8"):
    torch.library.register_fake("torchlsq::%s_q" % _norm_name, _fake_norm_w8_q, lib=_lib_def)
    torch.library.register_fake("torchlsq::%s" % _norm_name, _fake_norm_w8, lib=_lib_def)
    _lib_def.impl(_norm_name + "_q", _requant_no_grad(_norm_name + "_q", (1, 3, 4, 6, 7)), "Autograd")
    _lib_def.impl(_norm_name, _requant_no_grad(_norm_name, (1, 3, 4)), "Autograd")
del _norm_name


# -------------------------------------------------------------------------------------------------
# the attention core on 8-bit levels (_attn_w8_host.py): GPU tensors -> liblsq_hip_attn_w8.so (one call), CPU tensors -> the
# definition in torch ops; a shape-only kernel each.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_bmm_w8_q8_q", attn_w8_bmm_q)
    _lib_key.impl("lsq_bmm_w8_q8", attn_w8_bmm)
    _lib_key.impl("lsq_softmax_w8_q8_q", attn_w8_softmax_q)
    _lib_key.impl("lsq_softmax_w8_q8", attn_w8_softmax)
del _lib_key


def _fake_bmm_shape(a_levels, b_levels, transpose_b):
    return tuple(a_levels.shape[:-1]) + (b_levels.shape[-2] if transpose_b else b_levels.shape[-1],)


def _fake_bmm_w8_q(a_levels, a_scale, a_zero, b_levels, b_scale, b_zero, transpose_b, out_scale, out_shift, out_quant_min, out_quant_max,
                   out_type_min, out_type_max, mid_dtype):
    return torch.empty(_fake_bmm_shape(a_levels, b_levels, transpose_b), dtype=_fake_level_dtype(out_quant_max, out_type_max),
                       device=a_levels.device)


def _fake_bmm_w8(a_levels, a_scale, a_zero, b_levels, b_scale, b_zero, transpose_b, out_dtype):
    return torch.empty(_fake_bmm_shape(a_levels, b_levels, transpose_b), dtype=out_dtype, device=a_levels.device)


def _fake_softmax_w8_q(x_levels, table, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, mid_dtype, row_pad=1):
    C = x_levels.shape[-1]
    full = torch.empty(tuple(x_levels.shape[:-1]) + ((C + row_pad - 1) // row_pad * row_pad,),
                       dtype=_fake_level_dtype(out_quant_max, out_type_max), device=x_levels.device)
    return full[..., :C]


def _fake_softmax_w8(x_levels, table, out_dtype):
    return torch.empty(x_levels.shape, dtype=out_dtype, device=x_levels.device)


torch.library.register_fake("torchlsq::lsq_bmm_w8_q8_q", _fake_bmm_w8_q, lib=_lib_def)
torch.library.register_fake("torchlsq::lsq_bmm_w8_q8", _fake_bmm_w8, lib=_lib_def)
torch.library.register_fake("torchlsq::lsq_softmax_w8_q8_q", _fake_softmax_w8_q, lib=_lib_def)
torch.library.register_fake("torchlsq::lsq_softmax_w8_q8", _fake_softmax_w8, lib=_lib_def)
_lib_def.impl("lsq_bmm_w8_q8_q", _requant_no_grad("lsq_bmm_w8_q8_q", (1, 4, 7, 8)), "Autograd")
_lib_def.impl("lsq_bmm_w8_q8", _requant_no_grad("lsq_bmm_w8_q8", (1, 4)), "Autograd")
_lib_def.impl("lsq_softmax_w8_q8_q", _requant_no_grad("lsq_softmax_w8_q8_q", (2, 3)), "Autograd")
_lib_def.impl("lsq_softmax_w8_q8", _requant_no_grad("lsq_softmax_w8_q8", ()), "Autograd")


# -------------------------------------------------------------------------------------------------
# the attention core on 8-bit levels in one launch (_attn_fused_w8_host.py): GPU tensors -> liblsq_hip_attn_fused_w8.so (one call; the
# three launches of liblsq_hip_attn_w8.so where the fused kernel does not serve the shape), CPU tensors -> the three CPU paths
# composed; a shape-only kernel.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_attention_w8_q8_q", attn_fused_w8_q)
del _lib_key


def _fake_attention_w8_q(q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table, scores_scale, scores_shift,
                         scores_quant_min, scores_quant_max, scores_type_min, scores_type_max, probs_scale, probs_shift, probs_quant_min,
                         probs_quant_max, probs_type_min, probs_type_max, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min,
                         out_type_max, mid_dtype):
    B, H, Tq, D = q_levels.shape
    return torch.empty((B, Tq, H * D), dtype=_fake_level_dtype(out_quant_max, out_type_max), device=q_levels.device)


torch.library.register_fake("torchlsq::lsq_attention_w8_q8_q", _fake_attention_w8_q, lib=_lib_def)
_lib_def.impl("lsq_attention_w8_q8_q", _requant_no_grad("lsq_attention_w8_q8_q", (1, 4, 7, 10, 11, 16, 17, 22, 23)), "Autograd")


# -------------------------------------------------------------------------------------------------
# the masked softmax on 8-bit levels (_attn_mask_w8_host.py): GPU tensors -> liblsq_hip_attn_mask_w8.so (one call), CPU tensors -> the
# definition in torch ops; a shape-only kernel each.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_softmax_mask_w8_q8_q", attn_mask_w8_softmax_q)
    _lib_key.impl("lsq_softmax_mask_w8_q8", attn_mask_w8_softmax)
del _lib_key


def _fake_softmax_mask_w8_q(x_levels, table, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, mid_dtype,
                            causal=False, causal_offset=0, key_lengths=None, row_pad=1):
    return _fake_softmax_w8_q(x_levels, table, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, mid_dtype,
                              row_pad)


def _fake_softmax_mask_w8(x_levels, table, out_dtype, causal=False, causal_offset=0, key_lengths=None):
    return torch.empty(x_levels.shape, dtype=out_dtype, device=x_levels.device)


torch.library.register_fake("torchlsq::lsq_softmax_mask_w8_q8_q", _fake_softmax_mask_w8_q, lib=_lib_def)
torch.library.register_fake("torchlsq::lsq_softmax_mask_w8_q8", _fake_softmax_mask_w8, lib=_lib_def)
_lib_def.impl("lsq_softmax_mask_w8_q8_q", _requant_no_grad("lsq_softmax_mask_w8_q8_q", (2, 3)), "Autograd")
_lib_def.impl("lsq_softmax_mask_w8_q8", _requant_no_grad("lsq_softmax_mask_w8_q8", ()), "Autograd")


# -------------------------------------------------------------------------------------------------
# rotary embedding and the KV-cache append on 8-bit levels (_rope_w8_host.py): GPU tensors -> liblsq_hip_rope_w8.so (one call), CPU
# tensors -> the definition in torch ops; a shape-only kernel each.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_rope_w8_q8_q", rope_w8_q)
    _lib_key.impl("lsq_rope_w8_q8", rope_w8)
    _lib_key.impl("lsq_kv_copy_w8", rope_w8_kv_copy)
del _lib_key


def _fake_rope_w8_q(x_levels, x_scale, x_zero, cos, sin, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max,
                    mid_dtype, positions=None, interleaved=False):
    return torch.empty(x_levels.shape, dtype=_fake_level_dtype(out_quant_max, out_type_max), device=x_levels.device)


def _fake_rope_w8(x_levels, x_scale, x_zero, cos, sin, out_dtype, positions=None, interleaved=False):
    return torch.empty(x_levels.shape, dtype=out_dtype, device=x_levels.device)


def _fake_kv_copy_w8(x_levels, out, positions=None, scatter=True):
    return None


torch.library.register_fake("torchlsq::lsq_rope_w8_q8_q", _fake_rope_w8_q, lib=_lib_def)
torch.library.register_fake("torchlsq::lsq_rope_w8_q8", _fake_rope_w8, lib=_lib_def)
torch.library.register_fake("torchlsq::lsq_kv_copy_w8", _fake_kv_copy_w8, lib=_lib_def)
_lib_def.impl("lsq_rope_w8_q8_q", _requant_no_grad("lsq_rope_w8_q8_q", (1, 3, 4, 5, 6)), "Autograd")
_lib_def.impl("lsq_rope_w8_q8", _requant_no_grad("lsq_rope_w8_q8", (1, 3, 4)), "Autograd")
_lib_def.impl("lsq_kv_copy_w8", _requant_no_grad("lsq_kv_copy_w8", ()), "Autograd")


# -------------------------------------------------------------------------------------------------
# decode attention on 8-bit levels against a grouped-query KV cache (_attn_decode_w8_host.py): GPU tensors ->
# liblsq_hip_attn_decode_w8.so (one call; the existing ops composed where the decode kernel does not serve the shape), CPU tensors ->
# that composition; a shape-only kernel.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_attention_decode_w8_q8_q", attn_decode_w8_q)
del _lib_key


def _fake_attention_decode_w8_q(q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table, scores_scale,
                                scores_shift, scores_quant_min, scores_quant_max, scores_type_min, scores_type_max, probs_scale, probs_shift,
                                probs_quant_min, probs_quant_max, probs_type_min, probs_type_max, out_scale, out_shift, out_quant_min,
                                out_quant_max, out_type_min, out_type_max, mid_dtype, causal=False, causal_offset=0, key_lengths=None):
    B, H, Tq, D = q_levels.shape
    return torch.empty((B, Tq, H * D), dtype=_fake_level_dtype(out_quant_max, out_type_max), device=q_levels.device)


torch.library.register_fake("torchlsq::lsq_attention_decode_w8_q8_q", _fake_attention_decode_w8_q, lib=_lib_def)
_lib_def.impl("lsq_attention_decode_w8_q8_q", _requant_no_grad("lsq_attention_decode_w8_q8_q", (1, 4, 7, 10, 11, 16, 17, 22, 23)), "Autograd")


# -------------------------------------------------------------------------------------------------
# prefill attention on 8-bit levels (_attn_prefill_w8_host.py): GPU tensors -> liblsq_hip_attn_decode_w8.so where G Tq <= 16, else
# liblsq_hip_attn_prefill_w8.so (one call each), else the existing ops composed; CPU tensors -> that composition; the decode op's
# shape-only kernel.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_attention_prefill_w8_q8_q", attn_prefill_w8_q)
del _lib_key
torch.library.register_fake("torchlsq::lsq_attention_prefill_w8_q8_q", _fake_attention_decode_w8_q, lib=_lib_def)
_lib_def.impl("lsq_attention_prefill_w8_q8_q", _requant_no_grad("lsq_attention_prefill_w8_q8_q", (1, 4, 7, 10, 11, 16, 17, 22, 23)), "Autograd")


# -------------------------------------------------------------------------------------------------
# split-key decode attention on 8-bit levels (_attn_decode_split_w8_host.py): GPU tensors -> liblsq_hip_attn_decode_split_w8.so (one
# call, three launches, a workspace from one torch.empty) where its plan says "split", else the existing ops composed; CPU tensors ->
# that composition; the decode op's shape-only kernel.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_attention_decode_split_w8_q8_q", attn_decode_split_w8_q)
del _lib_key


def _fake_attention_decode_split_w8_q(q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table, scores_scale,
                                      scores_shift, scores_quant_min, scores_quant_max, scores_type_min, scores_type_max, probs_scale,
                                      probs_shift, probs_quant_min, probs_quant_max, probs_type_min, probs_type_max, out_scale, out_shift,
                                      out_quant_min, out_quant_max, out_type_min, out_type_max, mid_dtype, causal=False, causal_offset=0,
                                      key_lengths=None, splits=0):
    B, H, Tq, D = q_levels.shape
    return torch.empty((B, Tq, H * D), dtype=_fake_level_dtype(out_quant_max, out_type_max), device=q_levels.device)


torch.library.register_fake("torchlsq::lsq_attention_decode_split_w8_q8_q", _fake_attention_decode_split_w8_q, lib=_lib_def)
_lib_def.impl("lsq_attention_decode_split_w8_q8_q", _requant_no_grad("lsq_attention_decode_split_w8_q8_q", (1, 4, 7, 10, 11, 16, 17, 22, 23)),
              "Autograd")


# -------------------------------------------------------------------------------------------------
# the paged KV cache on 8-bit levels (_attn_paged_w8_host.py): GPU tensors -> liblsq_hip_attn_paged_w8.so (the decode: one call, three
# launches, a workspace from one torch.empty where its plan says "paged", else the gather and the existing ops composed; the append:
# one call, one launch); CPU tensors -> the gather and that composition, and plain index assignment; a shape-only kernel each.
# Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_attention_decode_paged_w8_q8_q", attn_paged_w8_q)
    _lib_key.impl("lsq_kv_append_paged_w8", kv_append_paged_w8)
del _lib_key


def _fake_attention_decode_paged_w8_q(q_levels, q_scale, q_zero, k_pool, k_scale, k_zero, v_pool, v_scale, v_zero, block_table, table,
                                      scores_scale, scores_shift, scores_quant_min, scores_quant_max, scores_type_min, scores_type_max,
                                      probs_scale, probs_shift, probs_quant_min, probs_quant_max, probs_type_min, probs_type_max, out_scale,
                                      out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, mid_dtype, causal=False,
                                      causal_offset=0, key_lengths=None, splits=0):
    B, H, Tq, D = q_levels.shape
    return torch.empty((B, Tq, H * D), dtype=_fake_level_dtype(out_quant_max, out_type_max), device=q_levels.device)


def _fake_kv_append_paged_w8(k_levels, v_levels, k_pool, v_pool, block_table, positions=None):
    return None


torch.library.register_fake("torchlsq::lsq_attention_decode_paged_w8_q8_q", _fake_attention_decode_paged_w8_q, lib=_lib_def)
torch.library.register_fake("torchlsq::lsq_kv_append_paged_w8", _fake_kv_append_paged_w8, lib=_lib_def)
_lib_def.impl("lsq_attention_decode_paged_w8_q8_q", _requant_no_grad("lsq_attention_decode_paged_w8_q8_q", (1, 4, 7, 11, 12, 17, 18, 23, 24)),
              "Autograd")
_lib_def.impl("lsq_kv_append_paged_w8", _requant_no_grad("lsq_kv_append_paged_w8", ()), "Autograd")


# -------------------------------------------------------------------------------------------------
# chunked prefill attention on 8-bit levels (_attn_chunk_w8_host.py): GPU tensors -> liblsq_hip_attn_chunk_w8.so (one call, three
# launches over row tiles, a workspace from one torch.empty) where its plan says "chunk", else (the gather and) the existing ops
# composed with per-row key counts; CPU tensors -> that composition; the decode ops' shape-only kernels.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_attention_chunk_w8_q8_q", attn_chunk_w8_q)
    _lib_key.impl("lsq_attention_chunk_paged_w8_q8_q", attn_chunk_paged_w8_q)
del _lib_key
torch.library.register_fake("torchlsq::lsq_attention_chunk_w8_q8_q", _fake_attention_decode_split_w8_q, lib=_lib_def)
torch.library.register_fake("torchlsq::lsq_attention_chunk_paged_w8_q8_q", _fake_attention_decode_paged_w8_q, lib=_lib_def)
_lib_def.impl("lsq_attention_chunk_w8_q8_q", _requant_no_grad("lsq_attention_chunk_w8_q8_q", (1, 4, 7, 10, 11, 16, 17, 22, 23)), "Autograd")
_lib_def.impl("lsq_attention_chunk_paged_w8_q8_q", _requant_no_grad("lsq_attention_chunk_paged_w8_q8_q", (1, 4, 7, 11, 12, 17, 18, 23, 24)),
              "Autograd")


# -------------------------------------------------------------------------------------------------
# the gated product on 8-bit levels (_glu_w8_host.py): GPU tensors -> liblsq_hip_glu_w8.so (one call, one launch), CPU tensors -> the
# definition in torch ops; a shape-only kernel each.  Inference only.
# -------------------------------------------------------------------------------------------------
for _lib_key in (_lib_hip, _lib_cpu):
    _lib_key.impl("lsq_glu_w8_q8_q", glu_w8_q)
    _lib_key.impl("lsq_glu_w8_q8", glu_w8)
del _lib_key


@torch.library.register_fake("torchlsq::lsq_glu_w8_q8_q", lib=_lib_def)
def _fake_glu_w8_q8_q(gate_levels, up_levels, up_scale, up_zero, table, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min,
                      out_type_max, mid_dtype):
    return torch.empty(gate_levels.shape, dtype=_fake_level_dtype(out_quant_max, out_type_max), device=gate_levels.device)


@torch.library.register_fake("torchlsq::lsq_glu_w8_q8", lib=_lib_def)
def _fake_glu_w8_q8(gate_levels, up_levels, up_scale, up_zero, table, out_dtype):
    return torch.empty(gate_levels.shape, dtype=out_dtype, device=gate_levels.device)


_lib_def.impl("lsq_glu_w8_q8_q", _requant_no_grad("lsq_glu_w8_q8_q", (2, 4, 5, 6)), "Autograd")
_lib_def.impl("lsq_glu_w8_q8", _requant_no_grad("lsq_glu_w8_q8", (2, 4)), "Autograd")
