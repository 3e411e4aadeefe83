"""Host layer of the W8A8 ops that CLOSE A RESIDUAL BLOCK (include/lsq_hip_resadd_w8.h states the contract): the integer sum and
the fp32 steps of `_requant_w8_host.py`, then a residual given as 8-bit levels added in the epilogue:

    v = ((s_w[n] * float(I)) * s_x) + bias[n]                  fp32, each step rounded
    u = float(round_to(mid, v))                                float32 (identity), bfloat16 or float16
    p = pre ? float(round_to(mid, dequant(level(u; pre), pre))) : u     the layer's own output fake-quantizer (optional)
    d = float(round_to(mid, (float(l_r) - float(z_r)) * s_r))  the residual's level at the same (m, n)
    t = float(round_to(mid, p + d))                            torch's add in `mid`; d and the add are not one fma
    r = relu ? (t < 0 ? 0 : t) : t                             a select: a NaN stays a NaN
    y = level(r) of (out_scale, out_shift, range)              one byte

Two ops, `lsq_linear_w8_q8_add_q` / `lsq_conv2d_w8_q8_add_q`: levels in, levels out.  By DEFINITION the result equals the
composition of existing ops: the float-output op writing a `mid` y; with `pre` the per-tensor fake-quantize forward on that y;
`+ residual.dequantize(mid)`; the select; `lsq_levels_per_tensor`.  The CPU path IS that composition; the GPU path is ONE ctypes
call into liblsq_hip_resadd_w8.so, nothing is read back, and it equals the CPU path bit for bit.
"""
import ctypes

import torch

from ._abi import LsqQconvW8Geom, LsqResaddW8Pre, LsqResaddW8Res, _assert_has_ops, resadd_w8_library
from ._cpu_host import _require_cpu, cpu_forward
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._qconv_w8_host import _CL, _check_conv_args, _cpu_levels_conv, _geometry, _pair
from ._qconv_w8_host import _weight_args as _conv_weight_args
from ._qlinear_w8_host import _LEVEL_CODE, _check_w8_args, _cpu_levels_linear
from ._qlinear_w8_host import _weight_args as _linear_weight_args
from ._requant_w8_host import _SHAPES, _STORES, _check_out, _cpu_requant, _out_struct
from ._w8_host_common import _check_range, _name, _status, _take_out

_LOADS = ("bytes", "packets")
_ERR = "lsq_resadd_w8_last_error"


def _check_res(what, res_levels, res_scale, res_zero, shape):
    _check(res_levels.dtype in _LEVEL_CODE, "%s: the residual levels must be uint8 (0..255) or int8 (-128..127), got '%s'" %
           (what, _name(res_levels.dtype)))
    _check(tuple(res_levels.shape) == tuple(shape), "%s: the residual levels have shape %s, the output has %s" %
           (what, tuple(res_levels.shape), tuple(shape)))
    _check(res_scale.dtype == torch.float32 and res_scale.numel() == 1 and res_zero.dtype == torch.int32 and res_zero.numel() == 1,
           "%s: res_scale must be one float32 value and res_zero one int32 value (tensors on x's device)" % what)


def _check_pre(what, pre_scale, pre_shift, pre_rng):
    """whether there is a pre-quantizer, after its checks"""
    _check((pre_scale is None) == (pre_shift is None), "%s: pre_scale and pre_shift come together" % what)
    if pre_scale is None:
        return False
    _check_range(what + " (pre-quantizer)", *pre_rng)
    _check(pre_scale.dtype == torch.float32 and pre_shift.dtype == torch.float32 and pre_scale.numel() == 1 and pre_shift.numel() == 1,
           "%s: pre_scale and pre_shift must be float32 tensors of one value (a per-tensor quantizer) on x's device" % what)
    return True


def _cpu_pre(y, pre_scale, pre_shift, pre_rng):
    """step 2 of the definition: the per-tensor fake-quantize forward (`torchlsq.functional.lsq`'s CPU kernel) on a `mid` y"""
    sc, sh = pre_scale.detach().reshape(-1), pre_shift.detach().reshape(-1)
    args = (sc, sh, 0, False, pre_rng[0], pre_rng[1], pre_rng[2], pre_rng[3], True, 1.0, False, False, False)
    if y.dtype == torch.float16:
        # liblsq_cpu.so has no float16 storage type: the float32 forward on the exactly converted values, rounded to float16
        # once -- what the 16-bit kernels compute
        return cpu_forward(y.to(torch.float32), *args).to(torch.float16)
    return cpu_forward(y, *args)


def _cpu_resadd(y, res_levels, res_scale, res_zero, pre_scale, pre_shift, pre_rng, out_scale, out_shift, rng, relu, level_dtype):
    """steps 2 to 5 of the definition on a `mid` y that has the residual's shape"""
    if pre_scale is not None:
        y = _cpu_pre(y, pre_scale, pre_shift, pre_rng)
    d = ((res_levels.to(torch.float32) - res_zero.to(torch.float32)) * res_scale).to(y.dtype)       # LevelsTensor.dequantize(mid)
    return _cpu_requant(y + d, out_scale, out_shift, rng, relu, level_dtype)


def _res_struct(res_levels, res_scale, res_zero):
    return LsqResaddW8Res(res_levels.data_ptr(), _LEVEL_CODE[res_levels.dtype], res_scale.data_ptr(), res_zero.data_ptr())


def _pre_ref(pre_scale, pre_shift, pre_rng):
    """(the struct, which must outlive the call; the pointer argument)"""
    if pre_scale is None:
        return None, None
    pre = LsqResaddW8Pre(pre_scale.data_ptr(), pre_shift.data_ptr(), *pre_rng)
    return pre, ctypes.byref(pre)


# -------------------------------------------------------------------------------------------------
# linear
# -------------------------------------------------------------------------------------------------
def resadd_w8_linear_levels(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_scale, out_shift, quant_min, quant_max, type_min,
                            type_max, relu, mid_dtype, res_levels, res_scale, res_zero, pre_scale=None, pre_shift=None, pre_quant_min=0,
                            pre_quant_max=255, pre_type_min=0, pre_type_max=255, out=None):
    """x_levels [..., K] bytes and residual levels [..., N] -> the output quantizer's levels [..., N] (uint8 or int8).  `out` (not
    an argument of the op): a dense [M, N] level tensor to write into, at any byte offset.  Inference only."""
    what = "lsq_linear_w8_q8_add_q"
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    rng = (int(quant_min), int(quant_max), int(type_min), int(type_max))
    pre_rng = (int(pre_quant_min), int(pre_quant_max), int(pre_type_min), int(pre_type_max))
    ldt = _check_out(what, out_scale, out_shift, *rng, mid_dtype)
    N, K = _check_w8_args(what, x_levels, w_levels, w_scale, w_zero, bias, mid_dtype)
    _check(s_x.dtype == torch.float32 and s_x.numel() == 1 and zx.dtype == torch.int32 and zx.numel() == 1,
           "%s: s_x must be one float32 value and zx one int32 value (tensors on x's device)" % what)
    out_shape = x_levels.shape[:-1] + (N,)
    _check_res(what, res_levels, res_scale, res_zero, out_shape)
    has_pre = _check_pre(what, pre_scale, pre_shift, pre_rng)
    tensors = (x_levels, s_x, zx, w_levels, w_scale, w_zero, out_scale, out_shift, res_levels, res_scale, res_zero) + \
        ((bias,) if bias is not None else ()) + ((pre_scale, pre_shift) if has_pre else ())
    lx = x_levels.reshape(-1, K)
    M = lx.size(0)
    if not any(t.is_cuda for t in tensors):
        _require_cpu(what, *tensors)
        if M == 0 or N == 0:
            return torch.empty(out_shape, dtype=ldt)
        y = _cpu_levels_linear(lx, s_x, zx, w_levels, w_scale, w_zero, bias, mid_dtype)
        return _cpu_resadd(y, res_levels.reshape(M, N), res_scale, res_zero, pre_scale, pre_shift, pre_rng, out_scale, out_shift, rng,
                           relu, ldt).reshape(out_shape)
    _require_gpu(what, *tensors)
    if M == 0 or N == 0:
        return torch.empty(out_shape, dtype=ldt, device=x_levels.device)
    lib = resadd_w8_library()
    lx, wl, ws, wz = lx.contiguous(), w_levels.contiguous(), w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    rl = res_levels.reshape(M, N).contiguous()
    y = _take_out(what, out, (M, N), ldt, lx.device)
    oq = _out_struct(out_scale, out_shift, rng, relu, mid_dtype)
    rs = _res_struct(rl, res_scale, res_zero)
    pre, pre_arg = _pre_ref(pre_scale, pre_shift, pre_rng)
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_resadd_w8_linear_levels, _LEVEL_CODE[lx.dtype], lx.data_ptr(), M, s_x.data_ptr(), zx.data_ptr(),
                    *_linear_weight_args(wl, ws, wz, bd, N, K), ctypes.byref(oq), ctypes.byref(rs), pre_arg, y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_resadd_w8_linear_levels", lib, _ERR)
    return y.reshape(out_shape)


# -------------------------------------------------------------------------------------------------
# conv2d
# -------------------------------------------------------------------------------------------------
def resadd_w8_conv_levels(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, out_scale, out_shift, quant_min,
                          quant_max, type_min, type_max, relu, mid_dtype, res_levels, res_scale, res_zero, pre_scale=None, pre_shift=None,
                          pre_quant_min=0, pre_quant_max=255, pre_type_min=0, pre_type_max=255, out=None):
    """x_levels [B, Cin, H, W] bytes and residual levels [B, Cout, OH, OW] -> the output quantizer's levels [B, Cout, OH, OW] in
    channels-last memory.  A residual that is not channels-last is copied into that format first.  `out` (not an argument of the
    op): a channels-last level tensor of that shape to write into, at any byte offset.  Inference only."""
    what = "lsq_conv2d_w8_q8_add_q"
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    rng = (int(quant_min), int(quant_max), int(type_min), int(type_max))
    pre_rng = (int(pre_quant_min), int(pre_quant_max), int(pre_type_min), int(pre_type_max))
    ldt = _check_out(what, out_scale, out_shift, *rng, mid_dtype)
    _check_conv_args(what, x_levels, w_levels, w_scale, w_zero, bias, mid_dtype)
    _check(s_x.dtype == torch.float32 and s_x.numel() == 1 and zx.dtype == torch.int32 and zx.numel() == 1,
           "%s: s_x must be one float32 value and zx one int32 value (tensors on x's device)" % what)
    geom, OH, OW = _geometry(what, x_levels.shape, w_levels.shape, stride, padding, dilation)
    B, N = geom.B, geom.Cout
    _check_res(what, res_levels, res_scale, res_zero, (B, N, OH, OW))
    has_pre = _check_pre(what, pre_scale, pre_shift, pre_rng)
    tensors = (x_levels, s_x, zx, w_levels, w_scale, w_zero, out_scale, out_shift, res_levels, res_scale, res_zero) + \
        ((bias,) if bias is not None else ()) + ((pre_scale, pre_shift) if has_pre else ())
    if not any(t.is_cuda for t in tensors):
        _require_cpu(what, *tensors)
        if B == 0 or N == 0:
            return torch.empty((B, N, OH, OW), dtype=ldt, memory_format=_CL)
        y = _cpu_levels_conv(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, (geom.sh, geom.sw), (geom.ph, geom.pw),
                             (geom.dh, geom.dw), mid_dtype)
        return _cpu_resadd(y, res_levels, res_scale, res_zero, pre_scale, pre_shift, pre_rng, out_scale, out_shift, rng, relu,
                           ldt).contiguous(memory_format=_CL)
    _require_gpu(what, *tensors)
    if B == 0 or N == 0:
        return torch.empty((B, N, OH, OW), dtype=ldt, device=x_levels.device, memory_format=_CL)
    lib = resadd_w8_library()
    lx, wl = x_levels.contiguous(memory_format=_CL), w_levels.contiguous(memory_format=_CL)
    ws, wz = w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    rl = res_levels.contiguous(memory_format=_CL)
    y = _take_out(what, out, (B, N, OH, OW), ldt, lx.device, _CL)
    oq = _out_struct(out_scale, out_shift, rng, relu, mid_dtype)
    rs = _res_struct(rl, res_scale, res_zero)
    pre, pre_arg = _pre_ref(pre_scale, pre_shift, pre_rng)
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_resadd_w8_conv_levels, _LEVEL_CODE[lx.dtype], lx.data_ptr(), s_x.data_ptr(), zx.data_ptr(),
                    ctypes.byref(geom), *_conv_weight_args(wl, ws, wz, bd), ctypes.byref(oq), ctypes.byref(rs), pre_arg, y.data_ptr(),
                    _stream_of(idx))
    _status(rc, "lsq_resadd_w8_conv_levels", lib, _ERR)
    return y


# -------------------------------------------------------------------------------------------------
# plans: host only, nothing is launched
# -------------------------------------------------------------------------------------------------
def _plan_dict(out):
    return dict(form="mfma" if out[0] else "generic", shape=_SHAPES[out[1]], grid=out[2], block=out[3], rows_per_tile=out[4],
                cols_per_tile=out[5], lds_bytes=out[6], k_split=out[7], store=_STORES[out[8]], res_load=_LOADS[out[9]])


def resadd_w8_plan_linear(M, N, K, aligned=True, y_aligned=True, res_aligned=True):
    """The launch liblsq_hip_resadd_w8.so makes for (M, N, K): `requant_w8_plan_linear`'s fields and `res_load`, "packets"
    (N % 16 == 0 and a 16-byte aligned residual, matrix-core form) or "bytes"."""
    lib = resadd_w8_library()
    out = (ctypes.c_int32 * 10)()
    rc = lib.lsq_resadd_w8_plan_linear(int(M), int(N), int(K), 1 if aligned else 0, 1 if y_aligned else 0, 1 if res_aligned else 0,
                                       ctypes.byref(out))
    _status(rc, "lsq_resadd_w8_plan_linear", lib, _ERR)
    return _plan_dict(out)


def resadd_w8_plan_conv(B, Cin, H, W, Cout, kernel_size, stride=1, padding=0, dilation=1, aligned=True, y_aligned=True, res_aligned=True):
    """The same for x [B, Cin, H, W] and a [Cout, Cin, kh, kw] weight; plus M, N, K of the implicit GEMM."""
    what = "resadd_w8_plan_conv"
    lib = resadd_w8_library()
    kh, kw = _pair(what, "kernel_size", kernel_size)
    (sh, sw), (ph, pw), (dh, dw) = _pair(what, "stride", stride), _pair(what, "padding", padding), _pair(what, "dilation", dilation)
    geom = LsqQconvW8Geom(int(B), int(Cin), int(H), int(W), int(Cout), kh, kw, sh, sw, ph, pw, dh, dw)
    out = (ctypes.c_int32 * 10)()
    rc = lib.lsq_resadd_w8_plan_conv(ctypes.byref(geom), 1 if aligned else 0, 1 if y_aligned else 0, 1 if res_aligned else 0,
                                     ctypes.byref(out))
    _status(rc, "lsq_resadd_w8_plan_conv", lib, _ERR)
    OH = (int(H) + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    OW = (int(W) + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    return dict(_plan_dict(out), M=int(B) * OH * OW, N=int(Cout), K=kh * kw * int(Cin))
