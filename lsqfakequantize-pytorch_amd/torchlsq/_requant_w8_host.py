"""Host layer of the W8A8 ops with an 8-bit OUTPUT (include/lsq_hip_requant_w8.h states the contract): the integer sum and the
fp32 steps of `_qlinear_w8_host.py` / `_qconv_w8_host.py`, then (a ReLU and) the NEXT layer's per-tensor quantizer:

    v = ((s_w[n] * float(I)) * s_x) + bias[n]          fp32, each step rounded
    u = float(round_to(mid_dtype, v))                  float32 (identity), bfloat16 or float16
    r = relu ? (u < 0 ? 0 : u) : u                     a select: a NaN stays a NaN
    y = level(r) of (out_scale, out_shift, range)      one byte: uint8 for a range in 0..255, int8 for one in -128..127

Four ops: `lsq_linear_w8_q8_q` / `lsq_conv2d_w8_q8_q` take the activation levels with s_x and zx, `lsq_linear_w8_a8_q` /
`lsq_conv2d_w8_a8_q` a floating x and the INPUT quantizer's constants (mid_dtype is x's dtype).  Each returns the level tensor;
a convolution's is a logical [B, Cout, OH, OW] tensor in channels-last memory -- the next layer's operand as it lies.

By DEFINITION the result equals the composition of three existing ops: the float-output op writing a `mid_dtype` y, the
select, and `lsq_levels_per_tensor` on the result.  The CPU path IS that composition (`_cpu_levels_linear` /
`_cpu_levels_conv`, `torch.where`, `cpu_levels`); the GPU path is ONE ctypes call into liblsq_hip_requant_w8.so (plus the
pre-pass of the fused forms), nothing is read back, and it equals the CPU path bit for bit.
"""
import ctypes

import torch

from ._abi import _DTYPE_CODE, LsqQconvW8Geom, LsqRequantW8Out, _assert_has_ops, requant_w8_library
from ._cpu_host import _require_cpu, cpu_levels
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._qconv_w8_host import _CL, _check_conv_args, _cpu_levels_conv, _geometry, _pair
from ._qconv_w8_host import _weight_args as _conv_weight_args
from ._qlinear_w8_host import _LEVEL_CODE, _Y_DTYPES, _check_w8_args, _cpu_levels_linear
from ._qlinear_w8_host import _weight_args as _linear_weight_args
from ._w8_host_common import _act_constants, _check_range, _name, _status, _take_out

_SHAPES = ("generic", "tiles", "tiles_split_k")
_STORES = ("bytes", "packets")
_ERR = "lsq_requant_w8_last_error"


def _check_out(what, out_scale, out_shift, qmin, qmax, tmin, tmax, mid_dtype):
    """the level dtype of the output after the checks of the output quantizer"""
    _check(mid_dtype in _Y_DTYPES, "%s: mid_dtype must be float32, bfloat16 or float16, got '%s'" % (what, _name(mid_dtype)))
    unsigned = _check_range(what + " (output quantizer)", qmin, qmax, tmin, tmax)
    _check(out_scale.dtype == torch.float32 and out_shift.dtype == torch.float32 and out_scale.numel() == 1 and out_shift.numel() == 1,
           "%s: out_scale and out_shift must be float32 tensors of one value (a per-tensor quantizer) on x's device" % what)
    return torch.uint8 if unsigned else torch.int8


def _out_struct(out_scale, out_shift, rng, relu, mid_dtype):
    return LsqRequantW8Out(out_scale.data_ptr(), out_shift.data_ptr(), rng[0], rng[1], rng[2], rng[3], 1 if relu else 0,
                           _DTYPE_CODE[mid_dtype])


def _cpu_requant(y, out_scale, out_shift, rng, relu, level_dtype):
    """the select and the per-tensor levels forward on a `mid_dtype` y: steps 2 and 3 of the definition"""
    if relu:
        y = torch.where(y < 0, torch.zeros_like(y), y)
    lv = cpu_levels(y, out_scale.detach().reshape(-1), out_shift.detach().reshape(-1), 0, False, rng[0], rng[1], rng[2], rng[3], 0)
    return lv.view(torch.uint8) if level_dtype == torch.uint8 else lv


def _input_levels(what, x, act_scale, act_shift, rng):
    """CPU: (levels, s_x, zx) of a floating x under the input quantizer"""
    sc, sh = act_scale.detach().reshape(-1)[:1], act_shift.detach().reshape(-1)[:1]
    lv = cpu_levels(x.detach(), sc, sh, 0, False, rng[0], rng[1], rng[2], rng[3], 0)
    s_x, zx = _act_constants(sc, sh, rng[2], rng[3])
    return (lv.view(torch.uint8) if max(rng[1], rng[3]) > 127 else lv), s_x, zx


# -------------------------------------------------------------------------------------------------
# linear
# -------------------------------------------------------------------------------------------------
def requant_w8_linear_levels(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_scale, out_shift, quant_min, quant_max, type_min,
                             type_max, relu, mid_dtype, out=None):
    """x_levels [..., K] bytes -> the output quantizer's levels [..., N] (uint8 or int8).  `out` (not an argument of the op):
    a dense [M, N] level tensor to write into, at any byte offset.  Inference only."""
    what = "lsq_linear_w8_q8_q"
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    rng = (int(quant_min), int(quant_max), int(type_min), int(type_max))
    ldt = _check_out(what, out_scale, out_shift, *rng, mid_dtype)
    N, K = _check_w8_args(what, x_levels, w_levels, w_scale, w_zero, bias, mid_dtype)
    _check(s_x.dtype == torch.float32 and s_x.numel() == 1 and zx.dtype == torch.int32 and zx.numel() == 1,
           "%s: s_x must be one float32 value and zx one int32 value (tensors on x's device)" % what)
    out_shape = x_levels.shape[:-1] + (N,)
    tensors = (x_levels, s_x, zx, w_levels, w_scale, w_zero, out_scale, out_shift) + ((bias,) if bias is not None else ())
    lx = x_levels.reshape(-1, K)
    M = lx.size(0)
    if not any(t.is_cuda for t in tensors):
        _require_cpu(what, *tensors)
        if M == 0 or N == 0:
            return torch.empty(out_shape, dtype=ldt)
        y = _cpu_levels_linear(lx, s_x, zx, w_levels, w_scale, w_zero, bias, mid_dtype)
        return _cpu_requant(y, out_scale, out_shift, rng, relu, ldt).reshape(out_shape)
    _require_gpu(what, *tensors)
    if M == 0 or N == 0:
        return torch.empty(out_shape, dtype=ldt, device=x_levels.device)
    lib = requant_w8_library()
    lx, wl, ws, wz = lx.contiguous(), w_levels.contiguous(), w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    y = _take_out(what, out, (M, N), ldt, lx.device)
    oq = _out_struct(out_scale, out_shift, rng, relu, mid_dtype)
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_requant_w8_linear_levels, _LEVEL_CODE[lx.dtype], lx.data_ptr(), M, s_x.data_ptr(), zx.data_ptr(),
                    *_linear_weight_args(wl, ws, wz, bd, N, K), ctypes.byref(oq), y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_requant_w8_linear_levels", lib, _ERR)
    return y.reshape(out_shape)


def requant_w8_linear(x, act_scale, act_shift, qmin, qmax, tmin, tmax, w_levels, w_scale, w_zero, bias, out_scale, out_shift, quant_min,
                      quant_max, type_min, type_max, relu):
    """floating x [..., K] -> the output quantizer's levels [..., N]; mid_dtype is x's dtype.  Inference only."""
    what = "lsq_linear_w8_a8_q"
    _assert_has_ops()
    _check(x.is_floating_point(), "%s: x must be a floating-point tensor" % what)
    _check(x.dtype in _Y_DTYPES, "%s: x must be float32, bfloat16 or float16, got '%s'" % (what, _name(x.dtype)))
    rng = (int(quant_min), int(quant_max), int(type_min), int(type_max))
    ldt = _check_out(what, out_scale, out_shift, *rng, x.dtype)
    N, K = _check_w8_args(what, x, w_levels, w_scale, w_zero, bias, x.dtype)
    _check_range(what, qmin, qmax, tmin, tmax)
    _check(act_scale.dtype == torch.float32 and act_shift.dtype == torch.float32 and act_scale.numel() >= 1 and act_shift.numel() >= 1,
           "%s: the activation quantizer's scale and shift must be float32 tensors of one value (a per-tensor quantizer)" % what)
    out_shape = x.shape[:-1] + (N,)
    tensors = (x, act_scale, act_shift, w_levels, w_scale, w_zero, out_scale, out_shift) + ((bias,) if bias is not None else ())
    xd = x.reshape(-1, K)
    M = xd.size(0)
    on_gpu = any(t.is_cuda for t in tensors)
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    if M == 0 or N == 0:
        return torch.empty(out_shape, dtype=ldt, device=x.device)
    if not on_gpu:
        lv, s_x, zx = _input_levels(what, xd, act_scale, act_shift, (qmin, qmax, tmin, tmax))
        y = _cpu_levels_linear(lv, s_x, zx, w_levels, w_scale, w_zero, bias, x.dtype)
        return _cpu_requant(y, out_scale, out_shift, rng, relu, ldt).reshape(out_shape)
    lib = requant_w8_library()
    sc, sh = act_scale.detach().contiguous(), act_shift.detach().contiguous()
    xd, wl, ws, wz = xd.detach().contiguous(), w_levels.contiguous(), w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    y = torch.empty((M, N), dtype=ldt, device=x.device)
    levels_ws = torch.empty((M, max(K, 16)), dtype=torch.int8, device=x.device)
    oq = _out_struct(out_scale, out_shift, rng, relu, x.dtype)
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_requant_w8_linear, _DTYPE_CODE[x.dtype], xd.data_ptr(), M, sc.data_ptr(), sh.data_ptr(), qmin, qmax, tmin,
                    tmax, *_linear_weight_args(wl, ws, wz, bd, N, K), ctypes.byref(oq), y.data_ptr(), levels_ws.data_ptr(),
                    _stream_of(idx))
    _status(rc, "lsq_requant_w8_linear", lib, _ERR)
    return y.reshape(out_shape)


# -------------------------------------------------------------------------------------------------
# conv2d
# -------------------------------------------------------------------------------------------------
def requant_w8_conv_levels(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, out_scale, out_shift, quant_min,
                           quant_max, type_min, type_max, relu, mid_dtype, out=None):
    """x_levels [B, Cin, H, W] bytes -> the output quantizer's levels [B, Cout, OH, OW] in channels-last memory.  `out` (not an
    argument of the op): a channels-last level tensor of that shape to write into, at any byte offset.  Inference only."""
    what = "lsq_conv2d_w8_q8_q"
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    rng = (int(quant_min), int(quant_max), int(type_min), int(type_max))
    ldt = _check_out(what, out_scale, out_shift, *rng, mid_dtype)
    _check_conv_args(what, x_levels, w_levels, w_scale, w_zero, bias, mid_dtype)
    _check(s_x.dtype == torch.float32 and s_x.numel() == 1 and zx.dtype == torch.int32 and zx.numel() == 1,
           "%s: s_x must be one float32 value and zx one int32 value (tensors on x's device)" % what)
    geom, OH, OW = _geometry(what, x_levels.shape, w_levels.shape, stride, padding, dilation)
    B, N = geom.B, geom.Cout
    tensors = (x_levels, s_x, zx, w_levels, w_scale, w_zero, out_scale, out_shift) + ((bias,) if bias is not None else ())
    if not any(t.is_cuda for t in tensors):
        _require_cpu(what, *tensors)
        if B == 0 or N == 0:
            return torch.empty((B, N, OH, OW), dtype=ldt, memory_format=_CL)
        y = _cpu_levels_conv(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, (geom.sh, geom.sw), (geom.ph, geom.pw),
                             (geom.dh, geom.dw), mid_dtype)
        return _cpu_requant(y, out_scale, out_shift, rng, relu, ldt).contiguous(memory_format=_CL)
    _require_gpu(what, *tensors)
    if B == 0 or N == 0:
        return torch.empty((B, N, OH, OW), dtype=ldt, device=x_levels.device, memory_format=_CL)
    lib = requant_w8_library()
    lx, wl = x_levels.contiguous(memory_format=_CL), w_levels.contiguous(memory_format=_CL)
    ws, wz = w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    y = _take_out(what, out, (B, N, OH, OW), ldt, lx.device, _CL)
    oq = _out_struct(out_scale, out_shift, rng, relu, mid_dtype)
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_requant_w8_conv_levels, _LEVEL_CODE[lx.dtype], lx.data_ptr(), s_x.data_ptr(), zx.data_ptr(),
                    ctypes.byref(geom), *_conv_weight_args(wl, ws, wz, bd), ctypes.byref(oq), y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_requant_w8_conv_levels", lib, _ERR)
    return y


def requant_w8_conv(x, act_scale, act_shift, qmin, qmax, tmin, tmax, w_levels, w_scale, w_zero, bias, stride, padding, dilation, out_scale,
                    out_shift, quant_min, quant_max, type_min, type_max, relu):
    """floating x [B, Cin, H, W] -> the output quantizer's levels [B, Cout, OH, OW] in channels-last memory; mid_dtype is x's
    dtype.  Inference only."""
    what = "lsq_conv2d_w8_a8_q"
    _assert_has_ops()
    _check(x.is_floating_point(), "%s: x must be a floating-point tensor" % what)
    _check(x.dtype in _Y_DTYPES, "%s: x must be float32, bfloat16 or float16, got '%s'" % (what, _name(x.dtype)))
    rng = (int(quant_min), int(quant_max), int(type_min), int(type_max))
    ldt = _check_out(what, out_scale, out_shift, *rng, x.dtype)
    _check_conv_args(what, x, w_levels, w_scale, w_zero, bias, x.dtype)
    _check_range(what, qmin, qmax, tmin, tmax)
    _check(act_scale.dtype == torch.float32 and act_shift.dtype == torch.float32 and act_scale.numel() >= 1 and act_shift.numel() >= 1,
           "%s: the activation quantizer's scale and shift must be float32 tensors of one value (a per-tensor quantizer)" % what)
    geom, OH, OW = _geometry(what, x.shape, w_levels.shape, stride, padding, dilation)
    B, N = geom.B, geom.Cout
    tensors = (x, act_scale, act_shift, w_levels, w_scale, w_zero, out_scale, out_shift) + ((bias,) if bias is not None else ())
    on_gpu = any(t.is_cuda for t in tensors)
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    if B == 0 or N == 0:
        return torch.empty((B, N, OH, OW), dtype=ldt, device=x.device, memory_format=_CL)
    if not on_gpu:
        lv, s_x, zx = _input_levels(what, x, act_scale, act_shift, (qmin, qmax, tmin, tmax))
        y = _cpu_levels_conv(lv, s_x, zx, w_levels, w_scale, w_zero, bias, (geom.sh, geom.sw), (geom.ph, geom.pw), (geom.dh, geom.dw),
                             x.dtype)
        return _cpu_requant(y, out_scale, out_shift, rng, relu, ldt).contiguous(memory_format=_CL)
    lib = requant_w8_library()
    sc, sh = act_scale.detach().contiguous(), act_shift.detach().contiguous()
    xd, wl = x.detach().contiguous(memory_format=_CL), w_levels.contiguous(memory_format=_CL)
    ws, wz = w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    y = torch.empty((B, N, OH, OW), dtype=ldt, device=x.device, memory_format=_CL)
    levels_ws = torch.empty(max(xd.numel(), 16), dtype=torch.int8, device=x.device)
    oq = _out_struct(out_scale, out_shift, rng, relu, x.dtype)
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_requant_w8_conv, _DTYPE_CODE[x.dtype], xd.data_ptr(), sc.data_ptr(), sh.data_ptr(), qmin, qmax, tmin, tmax,
                    ctypes.byref(geom), *_conv_weight_args(wl, ws, wz, bd), ctypes.byref(oq), y.data_ptr(), levels_ws.data_ptr(),
                    _stream_of(idx))
    _status(rc, "lsq_requant_w8_conv", lib, _ERR)
    return y


# -------------------------------------------------------------------------------------------------
# plans: host only, nothing is launched
# -------------------------------------------------------------------------------------------------
def _plan_dict(out):
    return dict(form="mfma" if out[0] else "generic", shape=_SHAPES[out[1]], grid=out[2], block=out[3], rows_per_tile=out[4],
                cols_per_tile=out[5], lds_bytes=out[6], k_split=out[7], store=_STORES[out[8]])


def requant_w8_plan_linear(M, N, K, aligned=True, y_aligned=True):
    """The launch liblsq_hip_requant_w8.so makes for (M, N, K), a weight and levels that are (not) 16-byte aligned and a y that is
    (not).  form "mfma" / "generic"; shape "tiles", "tiles_split_k" or "generic" (no decode shape); store "packets" / "bytes"."""
    lib = requant_w8_library()
    out = (ctypes.c_int32 * 9)()
    rc = lib.lsq_requant_w8_plan_linear(int(M), int(N), int(K), 1 if aligned else 0, 1 if y_aligned else 0, ctypes.byref(out))
    _status(rc, "lsq_requant_w8_plan_linear", lib, _ERR)
    return _plan_dict(out)


def requant_w8_plan_conv(B, Cin, H, W, Cout, kernel_size, stride=1, padding=0, dilation=1, aligned=True, y_aligned=True):
    """The same for x [B, Cin, H, W] and a [Cout, Cin, kh, kw] weight; plus M, N, K of the implicit GEMM."""
    what = "requant_w8_plan_conv"
    lib = requant_w8_library()
    kh, kw = _pair(what, "kernel_size", kernel_size)
    (sh, sw), (ph, pw), (dh, dw) = _pair(what, "stride", stride), _pair(what, "padding", padding), _pair(what, "dilation", dilation)
    geom = LsqQconvW8Geom(int(B), int(Cin), int(H), int(W), int(Cout), kh, kw, sh, sw, ph, pw, dh, dw)
    out = (ctypes.c_int32 * 9)()
    rc = lib.lsq_requant_w8_plan_conv(ctypes.byref(geom), 1 if aligned else 0, 1 if y_aligned else 0, ctypes.byref(out))
    _status(rc, "lsq_requant_w8_plan_conv", lib, _ERR)
    OH = (int(H) + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    OW = (int(W) + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    return dict(_plan_dict(out), M=int(B) * OH * OW, N=int(Cout), K=kh * kw * int(Cin))
