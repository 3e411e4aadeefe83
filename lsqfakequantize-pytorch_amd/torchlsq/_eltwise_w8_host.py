"""Host layer of the elementwise ops on 8-bit LEVELS (include/lsq_hip_eltwise_w8.h states the contract): what keeps a converted
block in levels at its activation functions and at its squeeze-and-excitation gate.

    table op        y[i] = table[x[i]], the index being the byte as stored (an int8 level l reads entry l & 0xff)
    gate multiply   a = float(round_to(mid, (float(lx) - float(zx)) * s_x))          LevelsTensor.dequantize(mid)
                    g = float(round_to(mid, (float(lg[b, c]) - float(zg)) * s_g))
                    t = float(round_to(mid, a * g))                                  one rounded fp32 multiply
                    y = level(t) of (out_scale, out_shift, range), one byte -- or t itself, stored as mid_dtype

Three ops: `lsq_lut_w8`, `lsq_mul_gate_w8_q8_q` (levels out) and `lsq_mul_gate_w8_q8` (floats out).  The table op takes level
bytes of any shape and returns the same shape and memory layout; the gate multiply takes a logical [B, C, H, W] level tensor
(read channels-last) or a [B, C] one and a gate of [B, C] or [B, C, 1, 1], and returns x's shape (4-D: channels-last memory).

The CPU path IS the definition: `table[x.long()]`; for the multiply the existing ops composed -- torch float32 arithmetic,
`.to(mid_dtype)`, torch's multiply in `mid_dtype` and the existing `cpu_levels`.  Every op first calls the library's plan
function (host only, it runs without a GPU and enqueues nothing), which refuses an illegal shape with the library's message.
The GPU path is then ONE ctypes call that enqueues; nothing is read back, and it equals the CPU path bit for bit.
"""
import ctypes

import torch

from ._abi import _DTYPE_CODE, LsqEltwiseW8Mul, LsqEltwiseW8Shape, _assert_has_ops, eltwise_w8_library
from ._cpu_host import _require_cpu
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._w8_host_common import _LEVEL_CODE, _check_out_q, _cpu_finish, _name, _on_one_device, _one, _status, _take_out

_CL = torch.channels_last
_FAMILIES = ("generic", "packets")
_ERR = "lsq_eltwise_w8_last_error"


def _check_levels(what, name, levels):
    _check(levels.dtype in _LEVEL_CODE, "%s: %s must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, name, _name(levels.dtype)))


# -------------------------------------------------------------------------------------------------
# the table op
# -------------------------------------------------------------------------------------------------
def _dense(x):
    """x as it lies if its memory is dense in the default or the channels-last order, else a contiguous copy"""
    if x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(memory_format=_CL)):
        return x
    return x.contiguous()


def eltwise_w8_lut(x_levels, table, out_dtype, out=None):
    """level bytes of any shape -> table[byte] in the same shape and memory layout, as `out_dtype` (uint8 / int8: the same
    bytes).  `table`: 256 uint8 or int8 values on x's device.  `out` (not an argument of the op): a tensor like the result to
    write into, at any byte offset."""
    what = "lsq_lut_w8"
    _assert_has_ops()
    _check_levels(what, "the levels", x_levels)
    _check(table.dtype in _LEVEL_CODE and table.dim() == 1 and table.numel() == 256 and table.is_contiguous(),
           "%s: the table must be a dense uint8 or int8 tensor of 256 entries, got '%s' %s" % (what, _name(table.dtype), tuple(table.shape)))
    _check(out_dtype in _LEVEL_CODE, "%s: out_dtype must be uint8 or int8, got '%s'" % (what, _name(out_dtype)))
    on_gpu = x_levels.is_cuda or table.is_cuda
    if on_gpu:
        _require_gpu(what, x_levels, table)
    else:
        _require_cpu(what, x_levels, table)
    lx = _dense(x_levels)
    n = lx.numel()
    if out is None:
        y = torch.empty_like(lx, dtype=out_dtype)
    else:
        _check(out.dtype == out_dtype and out.shape == lx.shape and out.device == lx.device and out.stride() == lx.stride(),
               "%s: `out` must be a %s tensor of x's shape and strides on x's device" % (what, _name(out_dtype)))
        y = out
    if n == 0:
        return y
    if not on_gpu:
        y.view(torch.uint8).copy_(table.view(torch.uint8)[lx.view(torch.uint8).long()])
        return y
    lib = eltwise_w8_library()
    plan = (ctypes.c_int32 * 8)()
    _status(lib.lsq_eltwise_w8_plan_lut(n, 1, ctypes.byref(plan)), "lsq_eltwise_w8_plan_lut", lib, _ERR)
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_eltwise_w8_lut, lx.data_ptr(), table.data_ptr(), n, y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_eltwise_w8_lut", lib, _ERR)
    return y


# -------------------------------------------------------------------------------------------------
# the gate multiply
# -------------------------------------------------------------------------------------------------
def _mul_shape(what, x_levels, g_levels):
    """(B, C, H, W) after the library's checks of the shape; an empty batch is let through with B = 1"""
    _check(x_levels.dim() in (2, 4), "%s: x must be a [B, C, H, W] or a [B, C] level tensor, got %d dims" % (what, x_levels.dim()))
    B, C = int(x_levels.shape[0]), int(x_levels.shape[1])
    H, W = (int(x_levels.shape[2]), int(x_levels.shape[3])) if x_levels.dim() == 4 else (1, 1)
    _check(tuple(g_levels.shape) in ((B, C), (B, C, 1, 1)),
           "%s: the gate must be [B, C] or [B, C, 1, 1] = [%d, %d(, 1, 1)], got %s" % (what, B, C, tuple(g_levels.shape)))
    lib = eltwise_w8_library()
    out = (ctypes.c_int32 * 8)()
    _status(lib.lsq_eltwise_w8_plan_mul(ctypes.byref(LsqEltwiseW8Shape(max(B, 1), C, H, W)), 1, ctypes.byref(out)), what, lib, _ERR)
    return B, C, H, W


def cpu_mul_gate_value(x_levels, s_x, zx, g_levels, s_g, zg, mid_dtype):
    """t of the definition, a `mid_dtype` tensor of x's shape: the two `LevelsTensor.dequantize(mid_dtype)` and torch's multiply"""
    a = ((x_levels.to(torch.float32) - zx.to(torch.float32).reshape(())) * s_x.reshape(())).to(mid_dtype)
    g = ((g_levels.to(torch.float32) - zg.to(torch.float32).reshape(())) * s_g.reshape(())).to(mid_dtype)
    return a * g.reshape(g.shape[0], g.shape[1], *([1] * (x_levels.dim() - 2)))


def _mul(what, x_levels, s_x, zx, g_levels, s_g, zg, out_q, mid_dtype, out):
    _assert_has_ops()
    _check_levels(what, "x_levels", x_levels)
    _check_levels(what, "g_levels", g_levels)
    _check(_one(s_x, torch.float32) and _one(zx, torch.int32) and _one(s_g, torch.float32) and _one(zg, torch.int32),
           "%s: x_scale and g_scale must be one float32 value and x_zero and g_zero one int32 value (tensors on the levels' device)" % what)
    ydt, rng, qt = _check_out_q(what, out_q, mid_dtype)
    B, C, H, W = _mul_shape(what, x_levels, g_levels)
    on_gpu = _on_one_device(what, (x_levels, s_x, zx, g_levels, s_g, zg) + qt)
    four = x_levels.dim() == 4
    fmt = _CL if four else torch.contiguous_format
    if B == 0:
        return torch.empty(x_levels.shape, dtype=ydt, device=x_levels.device, memory_format=fmt)
    if not on_gpu:
        t = cpu_mul_gate_value(x_levels, s_x, zx, g_levels, s_g, zg, mid_dtype)
        return _cpu_finish(t, out_q, rng, ydt).contiguous(memory_format=fmt)
    lib = eltwise_w8_library()
    lx = x_levels.contiguous(memory_format=fmt)
    lg = g_levels.reshape(B, C).contiguous()
    y = _take_out(what, out, tuple(x_levels.shape), ydt, lx.device, fmt)
    mul = LsqEltwiseW8Mul(s_x.data_ptr(), zx.data_ptr(), s_g.data_ptr(), zg.data_ptr(), qt[0].data_ptr() if out_q else None,
                          qt[1].data_ptr() if out_q else None, rng[0], rng[1], rng[2], rng[3], _DTYPE_CODE[mid_dtype])
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_eltwise_w8_mul_gate, _LEVEL_CODE[lx.dtype], lx.data_ptr(), _LEVEL_CODE[lg.dtype], lg.data_ptr(),
                    ctypes.byref(LsqEltwiseW8Shape(B, C, H, W)), ctypes.byref(mul), y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_eltwise_w8_mul_gate", lib, _ERR)
    return y


def eltwise_w8_mul_gate_q(x_levels, x_scale, x_zero, g_levels, g_scale, g_zero, out_scale, out_shift, quant_min, quant_max, type_min,
                          type_max, mid_dtype, out=None):
    """x levels [B, C, H, W] (or [B, C]) times gate levels [B, C] (or [B, C, 1, 1]) -> the output quantizer's levels in x's shape
    (uint8 or int8; 4-D: channels-last memory).  `out` (not an argument of the op): a tensor like the result to write into, at
    any byte offset."""
    return _mul("lsq_mul_gate_w8_q8_q", x_levels, x_scale, x_zero, g_levels, g_scale, g_zero,
                (out_scale, out_shift, quant_min, quant_max, type_min, type_max), mid_dtype, out)


def eltwise_w8_mul_gate(x_levels, x_scale, x_zero, g_levels, g_scale, g_zero, out_dtype, out=None):
    """the same -> the products as `out_dtype` floats in x's shape."""
    return _mul("lsq_mul_gate_w8_q8", x_levels, x_scale, x_zero, g_levels, g_scale, g_zero, None, out_dtype, out)


# -------------------------------------------------------------------------------------------------
# plans: host only, nothing is launched
# -------------------------------------------------------------------------------------------------
def eltwise_w8_plan_lut(n, aligned=True):
    """The launch liblsq_hip_eltwise_w8.so makes for the table op on n bytes whose buffers are (not) 16-byte aligned: family
    "packets" / "generic", grid, block, packets_per_lane, lds_bytes, packets (n // 16) and tail_bytes (n % 16, served by the
    first workgroup of the same launch)."""
    lib = eltwise_w8_library()
    out = (ctypes.c_int32 * 8)()
    _status(lib.lsq_eltwise_w8_plan_lut(int(n), 1 if aligned else 0, ctypes.byref(out)), "lsq_eltwise_w8_plan_lut", lib, _ERR)
    return dict(family=_FAMILIES[out[0]], grid=out[1], block=out[2], packets_per_lane=out[3], lds_bytes=out[4], packets=out[5],
                tail_bytes=out[6])


def eltwise_w8_plan_mul(B, C, H=1, W=1, aligned=True):
    """The same for the gate multiply of x [B, C, H, W]: family, grid, block, pixels_per_lane, lds_bytes (0) and lanes_per_image
    (packets: C / 16 * ceil(H W / pixels_per_lane))."""
    lib = eltwise_w8_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_eltwise_w8_plan_mul(ctypes.byref(LsqEltwiseW8Shape(int(B), int(C), int(H), int(W))), 1 if aligned else 0, ctypes.byref(out))
    _status(rc, "lsq_eltwise_w8_plan_mul", lib, _ERR)
    return dict(family=_FAMILIES[out[0]], grid=out[1], block=out[2], pixels_per_lane=out[3], lds_bytes=out[4], lanes_per_image=out[5])
