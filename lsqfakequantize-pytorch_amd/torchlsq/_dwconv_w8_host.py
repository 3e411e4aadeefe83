"""Host layer of the W8A8 DEPTHWISE conv2d on 8-bit levels (include/lsq_hip_dwconv_w8.h states the contract): groups == C, one
output channel per input channel, no reduction over channels:

    I[b, c, oh, ow] = sum over the taps (i, j) inside x of (lx[b, c, oh sh - ph + i dh, ow sw - pw + j dw] - zx) * (lw[i, j, c] - zw[c])
    v = ((s_w[c] * float(I)) * s_x) + bias[c]          fp32, each step rounded once
    u = float(round_to(mid_dtype, v))                  float32 (identity), bfloat16 or float16
    r = act == 0 ? u : act == 1 ? (u < 0 ? 0 : u) : (u < 0 ? 0 : (u > 6 ? 6 : u))      selects: a NaN stays a NaN
    y = level(r) of (out_scale, out_shift, range), one byte -- or r itself, stored as mid_dtype

Two ops: `lsq_dwconv2d_w8_q8_q` (levels out) and `lsq_dwconv2d_w8_q8` (`out_dtype` floats out).  Each takes a logical
[B, C, H, W] level tensor (read channels-last) and the weight levels TAP-MAJOR, [kh, kw, C], and returns a logical
[B, C, OH, OW] tensor in channels-last memory.  There is no fused floating-x form: a floating input goes through
`lsq_levels_per_tensor` first.

The CPU path IS the definition: one int64 `F.conv2d(..., groups=C)` of lx - zx with lw - zw (zero padding of the difference is
padding with zx), the fp32 steps of `_cpu_levels_linear`, `.to(mid_dtype)`, `torch.where`, `cpu_levels`.  The geometry's checks
are the library's on both devices: every op first calls the library's plan function (host only, it runs without a GPU and
enqueues nothing), which refuses an illegal geometry with the library's message and gives OH and OW for the allocation of y.
The GPU path is then ONE ctypes call that enqueues; nothing is read back, and it equals the CPU path bit for bit.
"""
import ctypes

import torch
import torch.nn.functional as F

from ._abi import _DTYPE_CODE, LsqDwconvW8Out, LsqQconvW8Geom, _assert_has_ops, dwconv_w8_library
from ._hip_host import _check, _on_device, _stream_of
from ._w8_host_common import _LEVEL_CODE, _check_out_q, _cpu_finish, _name, _on_one_device, _pair, _status, _take_out

_CL = torch.channels_last
_FAMILIES = ("generic", "packets")
_ERR = "lsq_dwconv_w8_last_error"
ACTS = {"none": 0, "relu": 1, "relu6": 2}


def _plan_call(what, geom, aligned, y_aligned):
    lib = dwconv_w8_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_dwconv_w8_plan(ctypes.byref(geom), 1 if aligned else 0, 1 if y_aligned else 0, ctypes.byref(out))
    _status(rc, what, lib, _ERR)
    return out


def _geometry(what, x_shape, w_shape, stride, padding, dilation):
    """(geom, OH, OW) after the library's checks of the geometry; an empty batch is let through with B = 1"""
    _check(len(x_shape) == 4, "%s: the levels must be a [B, C, H, W] tensor, got %d dims" % (what, len(x_shape)))
    _check(len(w_shape) == 3, "%s: the weight levels must be tap-major, [kh, kw, C], got %d dims" % (what, len(w_shape)))
    B, C, H, W = (int(v) for v in x_shape)
    kh, kw, Cw = (int(v) for v in w_shape)
    _check(Cw == C, "%s: x has %d channels, the weight [kh, kw, C] has C = %d (a depthwise convolution: one filter per channel)" % (what, C, Cw))
    (sh, sw), (ph, pw), (dh, dw) = _pair(what, "stride", stride), _pair(what, "padding", padding), _pair(what, "dilation", dilation)
    geom = LsqQconvW8Geom(max(B, 1), C, H, W, C, kh, kw, sh, sw, ph, pw, dh, dw)
    out = _plan_call(what, geom, True, True)
    geom.B = B
    return geom, out[4], out[5]


def _cpu_value(lx, s_x, zx, w_levels, w_scale, w_zero, bias, geom, act, mid_dtype):
    """r of the definition, a `mid_dtype` [B, C, OH, OW] tensor"""
    C = geom.Cin
    a = lx.to(torch.int64) - zx.to(torch.int64).reshape(())
    wz = (w_levels.to(torch.int64) - w_zero.to(torch.int64).reshape(1, 1, -1)).permute(2, 0, 1).reshape(C, 1, geom.kh, geom.kw)
    I = F.conv2d(a, wz, None, (geom.sh, geom.sw), (geom.ph, geom.pw), (geom.dh, geom.dw), C)      # exact in int64
    y = (w_scale.reshape(1, -1, 1, 1) * I.to(torch.float32)) * s_x.reshape(())                   # one rounding each
    if bias is not None:
        y = y + bias.to(torch.float32).reshape(1, -1, 1, 1)
    u = y.to(mid_dtype)
    if act >= 1:
        u = torch.where(u < 0, torch.zeros_like(u), u)
    if act == 2:
        u = torch.where(u > 6, torch.full_like(u, 6), u)
    return u


def _dwconv(what, x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, out_q, act, mid_dtype, out):
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    _check(w_levels.dtype in _LEVEL_CODE, "%s: the weight levels must be int8 (-128..127) or uint8 (0..255), got '%s'"
           % (what, _name(w_levels.dtype)))
    ydt, rng, qt = _check_out_q(what, out_q, mid_dtype, "x's device")
    act = int(act)
    _check(act in (0, 1, 2), "%s: act must be 0 (none), 1 (ReLU) or 2 (ReLU6), got %d" % (what, act))
    _check(s_x.dtype == torch.float32 and s_x.numel() == 1 and zx.dtype == torch.int32 and zx.numel() == 1,
           "%s: s_x must be one float32 value and zx one int32 value (tensors on x's device)" % what)
    geom, OH, OW = _geometry(what, x_levels.shape, w_levels.shape, stride, padding, dilation)
    B, C = geom.B, geom.Cin
    _check(w_scale.dtype == torch.float32 and w_scale.dim() == 1 and w_scale.numel() == C,
           "%s: w_scale must be %d float32 values, one per channel, got %s of '%s'" % (what, C, tuple(w_scale.shape), _name(w_scale.dtype)))
    _check(w_zero.dtype == torch.int32 and w_zero.dim() == 1 and w_zero.numel() == C,
           "%s: w_zero must be %d int32 values, one per channel, got %s of '%s'" % (what, C, tuple(w_zero.shape), _name(w_zero.dtype)))
    if bias is not None:
        _check(bias.dim() == 1 and bias.numel() == C, "%s: the bias needs %d values, got shape %s" % (what, C, tuple(bias.shape)))
        _check(bias.dtype in (torch.float32, mid_dtype), "%s: the bias must be float32 or of %s" % (what, "mid_dtype" if out_q else "out_dtype"))
    tensors = (x_levels, s_x, zx, w_levels, w_scale, w_zero) + ((bias,) if bias is not None else ())
    on_gpu = _on_one_device(what, tensors + qt)
    if B == 0:
        return torch.empty((B, C, OH, OW), dtype=ydt, device=x_levels.device, memory_format=_CL)
    if not on_gpu:
        u = _cpu_value(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, geom, act, mid_dtype)
        return _cpu_finish(u, out_q, rng, ydt).contiguous(memory_format=_CL)
    lib = dwconv_w8_library()
    lx, wl, ws, wz = x_levels.contiguous(memory_format=_CL), w_levels.contiguous(), w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    y = _take_out(what, out, (B, C, OH, OW), ydt, lx.device, _CL)
    oq = LsqDwconvW8Out(qt[0].data_ptr() if out_q else None, qt[1].data_ptr() if out_q else None, rng[0], rng[1], rng[2], rng[3],
                        act, _DTYPE_CODE[mid_dtype])
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_dwconv_w8_forward_levels, _LEVEL_CODE[lx.dtype], lx.data_ptr(), s_x.data_ptr(), zx.data_ptr(),
                    ctypes.byref(geom), _LEVEL_CODE[wl.dtype], wl.data_ptr(), ws.data_ptr(), wz.data_ptr(),
                    None if bd is None else bd.data_ptr(), 0 if bd is None else _DTYPE_CODE[bd.dtype], ctypes.byref(oq), y.data_ptr(),
                    _stream_of(idx))
    _status(rc, "lsq_dwconv_w8_forward_levels", lib, _ERR)
    return y


def dwconv_w8_levels_q(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, out_scale, out_shift, quant_min,
                       quant_max, type_min, type_max, act, mid_dtype, out=None):
    """x_levels [B, C, H, W] bytes and w_levels [kh, kw, C] bytes -> the output quantizer's levels [B, C, OH, OW] (uint8 or int8)
    in channels-last memory.  `out` (not an argument of the op): a channels-last level tensor of that shape to write into, at any
    byte offset.  Inference only."""
    return _dwconv("lsq_dwconv2d_w8_q8_q", x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation,
                   (out_scale, out_shift, quant_min, quant_max, type_min, type_max), act, mid_dtype, out)


def dwconv_w8_levels(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, act, out_dtype, out=None):
    """The same with `out_dtype` floats out: r of the contract as it is.  Inference only."""
    return _dwconv("lsq_dwconv2d_w8_q8", x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, None, act,
                   out_dtype, out)


def dwconv_w8_plan(B, C, H, W, kernel_size, stride=1, padding=0, dilation=1, aligned=True, y_aligned=True):
    """The launch liblsq_hip_dwconv_w8.so makes for x [B, C, H, W] and a [kh, kw, C] weight whose x and weight buffers are (not)
    16-byte aligned and whose y is (not): family "packets" / "generic", grid, block, pixels_per_lane, OH, OW, unrolled_window (3
    where the packet kernel has the 3 x 3 window without dilation unrolled, else 0) and unrolled_stride (1 or 2, else 0).  Host
    only, nothing is launched."""
    what = "dwconv_w8_plan"
    kh, kw = _pair(what, "kernel_size", kernel_size)
    (sh, sw), (ph, pw), (dh, dw) = _pair(what, "stride", stride), _pair(what, "padding", padding), _pair(what, "dilation", dilation)
    geom = LsqQconvW8Geom(int(B), int(C), int(H), int(W), int(C), kh, kw, sh, sw, ph, pw, dh, dw)
    out = _plan_call("lsq_dwconv_w8_plan", geom, aligned, y_aligned)
    return dict(family=_FAMILIES[out[0]], grid=out[1], block=out[2], pixels_per_lane=out[3], OH=out[4], OW=out[5], unrolled_window=out[6],
                unrolled_stride=out[7])
