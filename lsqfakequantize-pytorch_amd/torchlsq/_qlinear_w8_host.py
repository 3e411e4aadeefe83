"""Host layer of the W8A8 linear op: 8-bit activation levels times 8-bit weight levels with one (scale, zero point) per
output row (include/lsq_hip_qlinear_w8.h states the arithmetic):

    I[m, n] = sum_k (lx[m, k] - zx) * (lw[n, k] - zw[n])                      an exact integer
    y[m, n] = ((s_w[n] * float(I)) * s_x) + bias[n]                           fp32, each step rounded, then y's type

Two ops over it.  `lsq_linear_w8_q8` takes the activation levels lx as bytes (uint8: 0..255, int8: -128..127) with s_x
(float32) and zx (int32) as one-element tensors on x's device.  `lsq_linear_w8_a8` takes a floating x and a per-tensor
quantizer's scale, shift and range and forms the levels itself -- a pre-pass of the library on the GPU, `cpu_levels` on the
CPU -- so its result is the levels op on `lsq_levels_per_tensor`'s bytes, bit for bit.  The weight is its levels [N, K]
(int8 or uint8), `w_scale` [N] float32 and `w_zero` [N] int32: what a per-channel quantized tensor of `lsq_quantize` holds.

GPU tensors: ONE ctypes call into liblsq_hip_qlinear_w8.so for any number of rows (the product of the leading dims);
nothing is read back; the fused op allocates the M * K bytes of levels the pre-pass writes.  CPU tensors: one int64 matrix
product, then the same fp32 steps -- the GPU result bit for bit; not a hot path.
"""
import ctypes

import torch

from ._abi import _DTYPE_CODE, LSQ_W8_I8, LSQ_W8_U8, _assert_has_ops, qlinear_w8_library
from ._cpu_host import _require_cpu, cpu_levels
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._w8_host_common import _act_constants, _check_range, _name, _status

_Y_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_LEVEL_CODE = {torch.uint8: LSQ_W8_U8, torch.int8: LSQ_W8_I8}
_SHAPES = ("generic", "decode", "tiles", "tiles_split_k")


def _check_w8_args(what, x, w_levels, w_scale, w_zero, bias, y_dtype):
    """(N, K) of the weight, after the checks both ops and both devices share"""
    _check(w_levels.dtype in _LEVEL_CODE, "%s: the weight levels must be int8 (-128..127) or uint8 (0..255), got '%s'"
           % (what, _name(w_levels.dtype)))
    _check(w_levels.dim() == 2, "%s: the weight levels must be [N, K], got %d dims" % (what, w_levels.dim()))
    N, K = w_levels.shape
    _check(w_scale.dtype == torch.float32 and w_scale.dim() == 1 and w_scale.numel() == N,
           "%s: w_scale must be %d float32 values, one per output row, got %s of '%s'" % (what, N, tuple(w_scale.shape), _name(w_scale.dtype)))
    _check(w_zero.dtype == torch.int32 and w_zero.dim() == 1 and w_zero.numel() == N,
           "%s: w_zero must be %d int32 values, one per output row, got %s of '%s'" % (what, N, tuple(w_zero.shape), _name(w_zero.dtype)))
    _check(x.dim() >= 1 and x.size(-1) == K,
           "%s: the last dimension of x is %s, the weight has K = %d" % (what, x.size(-1) if x.dim() else "missing", K))
    _check(y_dtype in _Y_DTYPES, "%s: the output must be float32, bfloat16 or float16, got '%s'" % (what, _name(y_dtype)))
    if bias is not None:
        _check(bias.dim() == 1 and bias.numel() == N, "%s: the bias needs %d values, got shape %s" % (what, N, tuple(bias.shape)))
        _check(bias.dtype in (torch.float32, y_dtype), "%s: the bias must be float32 or of the output's dtype" % what)
    return N, K


def _cpu_levels_linear(lx, s_x, zx, w_levels, w_scale, w_zero, bias, y_dtype):
    a = lx.to(torch.int64) - zx.to(torch.int64).reshape(())
    wz = w_levels.to(torch.int64) - w_zero.to(torch.int64).reshape(-1, 1)
    I = a @ wz.t()                                                      # exact in int64
    y = (w_scale.reshape(1, -1) * I.to(torch.float32)) * s_x.reshape(())    # one rounding each
    if bias is not None:
        y = y + bias.to(torch.float32)
    return y.to(y_dtype)


def _weight_args(wl, ws, wz, bias, N, K):
    return (_LEVEL_CODE[wl.dtype], wl.data_ptr(), N, K, ws.data_ptr(), wz.data_ptr(), None if bias is None else bias.data_ptr(),
            0 if bias is None else _DTYPE_CODE[bias.dtype])


def qlinear_w8_forward_levels(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_dtype):
    """x_levels [..., K] bytes -> y [..., N] of out_dtype.  Inference only."""
    what = "lsq_linear_w8_q8"
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    N, K = _check_w8_args(what, x_levels, w_levels, w_scale, w_zero, bias, out_dtype)
    _check(s_x.dtype == torch.float32 and s_x.numel() == 1 and zx.dtype == torch.int32 and zx.numel() == 1,
           "%s: s_x must be one float32 value and zx one int32 value (tensors on x's device)" % what)
    out_shape = x_levels.shape[:-1] + (N,)
    tensors = (x_levels, s_x, zx, w_levels, w_scale, w_zero) + ((bias,) if bias is not None else ())
    lx = x_levels.reshape(-1, K)
    M = lx.size(0)
    if not any(t.is_cuda for t in tensors):
        _require_cpu(what, *tensors)
        if M == 0 or N == 0:
            return torch.empty(out_shape, dtype=out_dtype)
        return _cpu_levels_linear(lx, s_x, zx, w_levels, w_scale, w_zero, bias, out_dtype).reshape(out_shape)
    _require_gpu(what, *tensors)
    if M == 0 or N == 0:
        return torch.empty(out_shape, dtype=out_dtype, device=x_levels.device)
    lib = qlinear_w8_library()
    lx, wl, ws, wz = lx.contiguous(), w_levels.contiguous(), w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    y = torch.empty((M, N), dtype=out_dtype, device=lx.device)
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_qlinear_w8_forward_levels, _LEVEL_CODE[lx.dtype], lx.data_ptr(), M, s_x.data_ptr(), zx.data_ptr(),
                    *_weight_args(wl, ws, wz, bd, N, K), y.data_ptr(), _DTYPE_CODE[out_dtype], _stream_of(idx))
    _status(rc, "lsq_qlinear_w8_forward_levels", lib, "lsq_qlinear_w8_last_error")
    return y.reshape(out_shape)


def qlinear_w8_forward(x, act_scale, act_shift, qmin, qmax, tmin, tmax, w_levels, w_scale, w_zero, bias):
    """floating x [..., K] -> y [..., N] of x's dtype: the levels of the per-tensor quantizer (act_scale, act_shift, range)
    are formed on the way.  Inference only."""
    what = "lsq_linear_w8_a8"
    _assert_has_ops()
    _check(x.is_floating_point(), "%s: x must be a floating-point tensor" % what)
    _check(x.dtype in _Y_DTYPES, "%s: x must be float32, bfloat16 or float16, got '%s'" % (what, _name(x.dtype)))
    N, K = _check_w8_args(what, x, w_levels, w_scale, w_zero, bias, x.dtype)
    unsigned = _check_range(what, qmin, qmax, tmin, tmax)
    _check(act_scale.dtype == torch.float32 and act_shift.dtype == torch.float32 and act_scale.numel() >= 1 and act_shift.numel() >= 1,
           "%s: the activation quantizer's scale and shift must be float32 tensors of one value (a per-tensor quantizer)" % what)
    out_shape = x.shape[:-1] + (N,)
    tensors = (x, act_scale, act_shift, w_levels, w_scale, w_zero) + ((bias,) if bias is not None else ())
    xd = x.reshape(-1, K)
    M = xd.size(0)
    on_gpu = any(t.is_cuda for t in tensors)
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    if M == 0 or N == 0:
        return torch.empty(out_shape, dtype=x.dtype, device=x.device)
    if not on_gpu:
        sc, sh = act_scale.detach().reshape(-1)[:1], act_shift.detach().reshape(-1)[:1]
        lv = cpu_levels(xd, sc, sh, 0, False, qmin, qmax, tmin, tmax, 0)
        lv = lv.view(torch.uint8) if unsigned else lv
        s_x, zx = _act_constants(sc, sh, tmin, tmax)
        return _cpu_levels_linear(lv, s_x, zx, w_levels, w_scale, w_zero, bias, x.dtype).reshape(out_shape)
    lib = qlinear_w8_library()
    sc, sh = act_scale.detach().contiguous(), act_shift.detach().contiguous()
    xd, wl, ws, wz = xd.contiguous(), w_levels.contiguous(), w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    levels_ws = torch.empty((M, max(K, 16)), dtype=torch.int8, device=x.device)
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_qlinear_w8_forward, _DTYPE_CODE[x.dtype], xd.data_ptr(), M, sc.data_ptr(), sh.data_ptr(), qmin, qmax,
                    tmin, tmax, *_weight_args(wl, ws, wz, bd, N, K), y.data_ptr(), levels_ws.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_qlinear_w8_forward", lib, "lsq_qlinear_w8_last_error")
    return y.reshape(out_shape)


def qlinear_w8_plan(M, N, K, w_aligned=True):
    """The launch liblsq_hip_qlinear_w8.so makes for (M, N, K) and a weight that is (not) 16-byte aligned -- host only,
    nothing is launched.  form "mfma" / "generic"; shape "decode" (M <= 16), "tiles", "tiles_split_k" or "generic"."""
    lib = qlinear_w8_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_qlinear_w8_plan(int(M), int(N), int(K), 1 if w_aligned else 0, ctypes.byref(out))
    _status(rc, "lsq_qlinear_w8_plan", lib, "lsq_qlinear_w8_last_error")
    return dict(form="mfma" if out[0] else "generic", shape=_SHAPES[out[1]], grid=out[2], block=out[3], rows_per_tile=out[4],
                cols_per_tile=out[5], lds_bytes=out[6], k_split=out[7])
