"""Host layer of the W8A8 conv2d op: 8-bit activation levels times 8-bit weight levels with one (scale, zero point) per
output channel, groups == 1, zero padding (include/lsq_hip_qconv_w8.h states the arithmetic):

    I[b, n, oh, ow] = sum_{i, j, c} (lx[b, c, oh sh - ph + i dh, ow sw - pw + j dw] - zx) * (lw[n, c, i, j] - zw[n])
    y[b, n, oh, ow] = ((s_w[n] * float(I)) * s_x) + bias[n]                   fp32, each step rounded, then y's type

an exact integer over every tap and input channel; a tap in the padding contributes 0 (it holds the LEVEL zx).

Two ops over it, the twins of `_qlinear_w8_host.py`'s.  `lsq_conv2d_w8_q8` takes the activation levels lx [B, Cin, H, W] as bytes
(uint8: 0..255, int8: -128..127) with s_x (float32) and zx (int32) as one-element tensors on x's device.  `lsq_conv2d_w8_a8`
takes a floating x and a per-tensor quantizer's scale, shift and range and forms the levels itself -- a pre-pass of the library
on the GPU, `cpu_levels` on the CPU -- so its result is the levels op on `lsq_levels_per_tensor`'s bytes, bit for bit.  The weight
is its levels [Cout, Cin, kh, kw] (int8 or uint8), `w_scale` [Cout] float32 and `w_zero` [Cout] int32.

MEMORY.  The library reads channels-last operands: x as [B, H, W, Cin], the weight as [Cout, kh, kw, Cin] -- what
`t.contiguous(memory_format=torch.channels_last)` is.  An x (levels or floating) or a weight that is not channels-last is made so
by the framework before the call: one extra read and write of that tensor per call.  Keep a model's activations and the
module's weight channels-last (Conv2dW8A8 does) and nothing is copied.  The result is a logical [B, Cout, OH, OW] tensor in
channels-last memory.

GPU tensors: ONE ctypes call into liblsq_hip_qconv_w8.so; nothing is read back; the fused op allocates the B H W Cin bytes of
levels the pre-pass writes.  CPU tensors: one int64 `F.conv2d` of lx - zx with lw - zw[n] (zero padding of the difference is
padding with zx), then the same fp32 steps -- the GPU result bit for bit; not a hot path.
"""
import ctypes

import torch
import torch.nn.functional as F

from ._abi import _DTYPE_CODE, LSQ_W8_I8, LSQ_W8_U8, LsqQconvW8Geom, _assert_has_ops, qconv_w8_library
from ._cpu_host import _require_cpu, cpu_levels
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._qlinear_w8_host import _Y_DTYPES
from ._w8_host_common import _act_constants, _check_range, _name, _status

_LEVEL_CODE = {torch.uint8: LSQ_W8_U8, torch.int8: LSQ_W8_I8}      # LSQ_QCONV_W8_U8 / _I8 have the same values
_SHAPES = ("generic", "tiles", "tiles_split_k")
_CL = torch.channels_last


def _pair(what, name, v):
    v = tuple(int(e) for e in v) if isinstance(v, (tuple, list)) else (int(v),)
    _check(len(v) in (1, 2), "%s: %s must be one int or a pair of ints, got %d values" % (what, name, len(v)))
    return v * 2 if len(v) == 1 else v


def _geometry(what, x_shape, w_shape, stride, padding, dilation):
    """(lsq_qconv_w8_geom, OH, OW) after the checks of the geometry both ops and both devices share"""
    B, Cin, H, W = (int(v) for v in x_shape)
    Cout, _, kh, kw = (int(v) for v in w_shape)
    (sh, sw), (ph, pw), (dh, dw) = _pair(what, "stride", stride), _pair(what, "padding", padding), _pair(what, "dilation", dilation)
    _check(sh >= 1 and sw >= 1, "%s: the stride must be positive, got (%d, %d)" % (what, sh, sw))
    _check(dh >= 1 and dw >= 1, "%s: the dilation must be positive, got (%d, %d)" % (what, dh, dw))
    _check(ph >= 0 and pw >= 0, "%s: the padding must not be negative, got (%d, %d)" % (what, ph, pw))
    _check(kh >= 1 and kw >= 1 and Cin >= 1 and H >= 1 and W >= 1,
           "%s: x [%d, %d, %d, %d] and a %d x %d kernel: Cin, H, W, kh and kw must be at least 1" % (what, B, Cin, H, W, kh, kw))
    OH = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    OW = (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    _check(H + 2 * ph - dh * (kh - 1) >= 1 and W + 2 * pw - dw * (kw - 1) >= 1,
           "%s: an empty output: the dilated %d x %d kernel does not fit the padded [%d, %d] image" % (what, kh, kw, H + 2 * ph, W + 2 * pw))
    return LsqQconvW8Geom(B, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw), OH, OW


def _check_conv_args(what, x, w_levels, w_scale, w_zero, bias, y_dtype):
    _check(w_levels.dtype in _LEVEL_CODE, "%s: the weight levels must be int8 (-128..127) or uint8 (0..255), got '%s'"
           % (what, _name(w_levels.dtype)))
    _check(w_levels.dim() == 4, "%s: the weight levels must be [Cout, Cin, kh, kw], got %d dims" % (what, w_levels.dim()))
    _check(x.dim() == 4, "%s: x must be [B, Cin, H, W], got %d dims" % (what, x.dim()))
    N, Cin = w_levels.shape[:2]
    _check(x.size(1) == Cin, "%s: x has %d channels, the weight has Cin = %d (groups == 1)" % (what, x.size(1), Cin))
    _check(w_scale.dtype == torch.float32 and w_scale.dim() == 1 and w_scale.numel() == N,
           "%s: w_scale must be %d float32 values, one per output channel, got %s of '%s'" % (what, N, tuple(w_scale.shape), _name(w_scale.dtype)))
    _check(w_zero.dtype == torch.int32 and w_zero.dim() == 1 and w_zero.numel() == N,
           "%s: w_zero must be %d int32 values, one per output channel, got %s of '%s'" % (what, N, tuple(w_zero.shape), _name(w_zero.dtype)))
    _check(y_dtype in _Y_DTYPES, "%s: the output must be float32, bfloat16 or float16, got '%s'" % (what, _name(y_dtype)))
    if bias is not None:
        _check(bias.dim() == 1 and bias.numel() == N, "%s: the bias needs %d values, got shape %s" % (what, N, tuple(bias.shape)))
        _check(bias.dtype in (torch.float32, y_dtype), "%s: the bias must be float32 or of the output's dtype" % what)


def _cpu_levels_conv(lx, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, y_dtype):
    a = lx.to(torch.int64) - zx.to(torch.int64).reshape(())
    wz = w_levels.to(torch.int64) - w_zero.to(torch.int64).reshape(-1, 1, 1, 1)
    I = F.conv2d(a, wz, None, stride, padding, dilation)                # exact in int64; zero padding of lx - zx is padding with zx
    y = (w_scale.reshape(1, -1, 1, 1) * I.to(torch.float32)) * s_x.reshape(())     # one rounding each
    if bias is not None:
        y = y + bias.to(torch.float32).reshape(1, -1, 1, 1)
    return y.to(y_dtype).contiguous(memory_format=_CL)


def _empty_y(B, N, OH, OW, dtype, device):
    return torch.empty((B, N, OH, OW), dtype=dtype, device=device, memory_format=_CL)


def _weight_args(wl, ws, wz, bias):
    return (_LEVEL_CODE[wl.dtype], wl.data_ptr(), ws.data_ptr(), wz.data_ptr(), None if bias is None else bias.data_ptr(),
            0 if bias is None else _DTYPE_CODE[bias.dtype])


def qconv_w8_forward_levels(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, stride, padding, dilation, out_dtype):
    """x_levels [B, Cin, H, W] bytes -> y [B, Cout, OH, OW] of out_dtype in channels-last memory.  Inference only."""
    what = "lsq_conv2d_w8_q8"
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    _check_conv_args(what, x_levels, w_levels, w_scale, w_zero, bias, out_dtype)
    _check(s_x.dtype == torch.float32 and s_x.numel() == 1 and zx.dtype == torch.int32 and zx.numel() == 1,
           "%s: s_x must be one float32 value and zx one int32 value (tensors on x's device)" % what)
    geom, OH, OW = _geometry(what, x_levels.shape, w_levels.shape, stride, padding, dilation)
    B, N = geom.B, geom.Cout
    tensors = (x_levels, s_x, zx, w_levels, w_scale, w_zero) + ((bias,) if bias is not None else ())
    if not any(t.is_cuda for t in tensors):
        _require_cpu(what, *tensors)
        if B == 0 or N == 0:
            return _empty_y(B, N, OH, OW, out_dtype, x_levels.device)
        return _cpu_levels_conv(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, (geom.sh, geom.sw), (geom.ph, geom.pw),
                                (geom.dh, geom.dw), out_dtype)
    _require_gpu(what, *tensors)
    y = _empty_y(B, N, OH, OW, out_dtype, x_levels.device)
    if B == 0 or N == 0:
        return y
    lib = qconv_w8_library()
    lx, wl = x_levels.contiguous(memory_format=_CL), w_levels.contiguous(memory_format=_CL)
    ws, wz = w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    idx = lx.device.index
    wa = _weight_args(wl, ws, wz, bd)
    rc = _on_device(idx, lib.lsq_qconv_w8_forward_levels, _LEVEL_CODE[lx.dtype], lx.data_ptr(), s_x.data_ptr(), zx.data_ptr(),
                    ctypes.byref(geom), *wa, y.data_ptr(), _DTYPE_CODE[out_dtype], _stream_of(idx))
    _status(rc, "lsq_qconv_w8_forward_levels", lib, "lsq_qconv_w8_last_error")
    return y


def qconv_w8_forward(x, act_scale, act_shift, qmin, qmax, tmin, tmax, w_levels, w_scale, w_zero, bias, stride, padding, dilation):
    """floating x [B, Cin, H, W] -> y [B, Cout, OH, OW] of x's dtype in channels-last memory: the levels of the per-tensor
    quantizer (act_scale, act_shift, range) are formed on the way.  Inference only."""
    what = "lsq_conv2d_w8_a8"
    _assert_has_ops()
    _check(x.is_floating_point(), "%s: x must be a floating-point tensor" % what)
    _check(x.dtype in _Y_DTYPES, "%s: x must be float32, bfloat16 or float16, got '%s'" % (what, _name(x.dtype)))
    _check_conv_args(what, x, w_levels, w_scale, w_zero, bias, x.dtype)
    unsigned = _check_range(what, qmin, qmax, tmin, tmax)
    _check(act_scale.dtype == torch.float32 and act_shift.dtype == torch.float32 and act_scale.numel() >= 1 and act_shift.numel() >= 1,
           "%s: the activation quantizer's scale and shift must be float32 tensors of one value (a per-tensor quantizer)" % what)
    geom, OH, OW = _geometry(what, x.shape, w_levels.shape, stride, padding, dilation)
    B, N = geom.B, geom.Cout
    tensors = (x, act_scale, act_shift, w_levels, w_scale, w_zero) + ((bias,) if bias is not None else ())
    on_gpu = any(t.is_cuda for t in tensors)
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    if B == 0 or N == 0:
        return _empty_y(B, N, OH, OW, x.dtype, x.device)
    if not on_gpu:
        sc, sh = act_scale.detach().reshape(-1)[:1], act_shift.detach().reshape(-1)[:1]
        lv = cpu_levels(x.detach(), sc, sh, 0, False, qmin, qmax, tmin, tmax, 0)
        lv = lv.view(torch.uint8) if unsigned else lv
        s_x, zx = _act_constants(sc, sh, tmin, tmax)
        return _cpu_levels_conv(lv, s_x, zx, w_levels, w_scale, w_zero, bias, (geom.sh, geom.sw), (geom.ph, geom.pw),
                                (geom.dh, geom.dw), x.dtype)
    lib = qconv_w8_library()
    sc, sh = act_scale.detach().contiguous(), act_shift.detach().contiguous()
    xd, wl = x.detach().contiguous(memory_format=_CL), w_levels.contiguous(memory_format=_CL)
    ws, wz = w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    y = _empty_y(B, N, OH, OW, x.dtype, x.device)
    levels_ws = torch.empty(max(xd.numel(), 16), dtype=torch.int8, device=x.device)
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_qconv_w8_forward, _DTYPE_CODE[x.dtype], xd.data_ptr(), sc.data_ptr(), sh.data_ptr(), qmin, qmax, tmin,
                    tmax, ctypes.byref(geom), *_weight_args(wl, ws, wz, bd), y.data_ptr(), levels_ws.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_qconv_w8_forward", lib, "lsq_qconv_w8_last_error")
    return y


def qconv_w8_plan(B, Cin, H, W, Cout, kernel_size, stride=1, padding=0, dilation=1, aligned=True):
    """The launch liblsq_hip_qconv_w8.so makes for x [B, Cin, H, W] and a [Cout, Cin, kh, kw] weight with (not) 16-byte aligned
    levels and weight -- host only, nothing is launched.  form "mfma" / "generic"; shape "tiles", "tiles_split_k" or
    "generic"; rows_per_tile counts output pixels, cols_per_tile output channels; plus M, N, K of the implicit GEMM."""
    what = "qconv_w8_plan"
    lib = qconv_w8_library()
    kh, kw = _pair(what, "kernel_size", kernel_size)
    (sh, sw), (ph, pw), (dh, dw) = _pair(what, "stride", stride), _pair(what, "padding", padding), _pair(what, "dilation", dilation)
    geom = LsqQconvW8Geom(int(B), int(Cin), int(H), int(W), int(Cout), kh, kw, sh, sw, ph, pw, dh, dw)
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_qconv_w8_plan(ctypes.byref(geom), 1 if aligned else 0, ctypes.byref(out))
    _status(rc, "lsq_qconv_w8_plan", lib, "lsq_qconv_w8_last_error")
    OH = (int(H) + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    OW = (int(W) + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    return dict(form="mfma" if out[0] else "generic", shape=_SHAPES[out[1]], grid=out[2], block=out[3], rows_per_tile=out[4],
                cols_per_tile=out[5], lds_bytes=out[6], k_split=out[7], M=int(B) * OH * OW, N=int(Cout), K=kh * kw * int(Cin))
