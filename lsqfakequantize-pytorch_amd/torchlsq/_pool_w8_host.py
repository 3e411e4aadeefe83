"""Host layer of 2-D pooling on 8-bit LEVELS (include/lsq_hip_pool_w8.h states the contract): what keeps a converted network in
levels between its W8A8 layers.

    max pool       y = max over the window's taps inside the input of the levels, as integers: levels of the SAME quantizer
    average pool   S = sum over the window's taps inside the input of (l - z_x)         exact integer
                   v = (float(S) * s_x) / float(D)                                    fp32, each step rounded once
                   u = float(round_to(mid_dtype, v))
                   y = level(u) of (out_scale, out_shift, range), one byte -- or u itself, stored as mid_dtype

with D ATen's divisor (divisor_override, else the window clipped to the padded extent with count_include_pad, else the taps
inside the input).  Three ops: `lsq_max_pool2d_q8`, `lsq_avg_pool2d_q8_q` (levels out) and `lsq_avg_pool2d_q8` (floats out).
Each takes a logical [B, C, H, W] level tensor (read channels-last) and returns a logical [B, C, OH, OW] tensor in
channels-last memory.

The CPU path IS the definition: `F.max_pool2d` on the levels as integers; for the average an exact window sum, torch float32
ops, `.to(mid_dtype)` and the existing `cpu_levels`.  The geometry's checks are the library's on both devices: every op first
calls the library's plan function (host only, it runs without a GPU and enqueues nothing), which refuses an illegal geometry
with the library's message and gives OH and OW for the allocation of y.  The GPU path is then ONE ctypes call that enqueues
(`lsq_pool_w8_max` / `lsq_pool_w8_avg_forward`, which repeats those checks itself: two ctypes calls per op in all, three for the
adaptive forms, which ask `lsq_pool_w8_adaptive` for the kernel); nothing is read back, and it equals the CPU path bit for bit.
"""
import ctypes

import torch
import torch.nn.functional as F

from ._abi import _DTYPE_CODE, LsqPoolW8Avg, LsqPoolW8Geom, _assert_has_ops, pool_w8_library
from ._cpu_host import _require_cpu
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._w8_host_common import (_LEVEL_CODE, _check_out_q, _check_x_constants, _cpu_finish, _name, _on_one_device, _pair, _status,
                              _take_out)

_CL = torch.channels_last
_FAMILIES = ("generic", "packets", "packets_shared")
_ERR = "lsq_pool_w8_last_error"


def _geometry(what, shape, kernel, stride, padding, dilation, ceil_mode, average):
    """(geom, OH, OW) after the library's checks of the geometry; an empty batch is let through with B = 1"""
    _check(len(shape) == 4, "%s: the levels must be a [B, C, H, W] tensor, got %d dims" % (what, len(shape)))
    (kh, kw), (sh, sw) = _pair(what, "kernel_size", kernel), _pair(what, "stride", stride)
    (ph, pw), (dh, dw) = _pair(what, "padding", padding), _pair(what, "dilation", dilation)
    B, C, H, W = (int(v) for v in shape)
    geom = LsqPoolW8Geom(max(B, 1), C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, 1 if ceil_mode else 0)
    lib = pool_w8_library()
    out = (ctypes.c_int32 * 8)()
    rc = (lib.lsq_pool_w8_plan_avg if average else lib.lsq_pool_w8_plan_max)(ctypes.byref(geom), 1, ctypes.byref(out))
    _status(rc, what, lib, _ERR)
    geom.B = B
    return geom, out[4], out[5]


def _check_levels(what, levels):
    _check(levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(levels.dtype)))


# -------------------------------------------------------------------------------------------------
# max pool
# -------------------------------------------------------------------------------------------------
def pool_w8_max(levels, kernel_size, stride, padding, dilation, ceil_mode, out=None):
    """levels [B, C, H, W] bytes -> [B, C, OH, OW] bytes of the same dtype in channels-last memory.  `out` (not an argument of the
    op): a channels-last level tensor of that shape to write into, at any byte offset."""
    what = "lsq_max_pool2d_q8"
    _assert_has_ops()
    _check_levels(what, levels)
    geom, OH, OW = _geometry(what, levels.shape, kernel_size, stride, padding, dilation, ceil_mode, False)
    B, C = geom.B, geom.C
    if not levels.is_cuda:
        _require_cpu(what, levels)
        if B == 0:
            return torch.empty((B, C, OH, OW), dtype=levels.dtype, memory_format=_CL)
        y = F.max_pool2d(levels.to(torch.float32), (geom.kh, geom.kw), (geom.sh, geom.sw), (geom.ph, geom.pw), (geom.dh, geom.dw),
                         bool(geom.ceil_mode))
        return y.to(levels.dtype).contiguous(memory_format=_CL)
    _require_gpu(what, levels)
    if B == 0:
        return torch.empty((B, C, OH, OW), dtype=levels.dtype, device=levels.device, memory_format=_CL)
    lib = pool_w8_library()
    lx = levels.contiguous(memory_format=_CL)
    y = _take_out(what, out, (B, C, OH, OW), lx.dtype, lx.device, _CL)
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_pool_w8_max, _LEVEL_CODE[lx.dtype], lx.data_ptr(), ctypes.byref(geom), y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_pool_w8_max", lib, _ERR)
    return y


# -------------------------------------------------------------------------------------------------
# average pool
# -------------------------------------------------------------------------------------------------
def _divisor(geom, OH, OW, count_include_pad, divisor_override):
    """ATen's divisor per output pixel, float32 [OH, OW]"""
    if divisor_override is not None:
        return torch.full((OH, OW), int(divisor_override), dtype=torch.int64).to(torch.float32)
    h0 = torch.arange(OH, dtype=torch.int64) * geom.sh - geom.ph
    w0 = torch.arange(OW, dtype=torch.int64) * geom.sw - geom.pw
    if count_include_pad:
        nh = torch.clamp(h0 + geom.kh, max=geom.H + geom.ph) - h0
        nw = torch.clamp(w0 + geom.kw, max=geom.W + geom.pw) - w0
    else:
        nh = torch.clamp(h0 + geom.kh, max=geom.H) - torch.clamp(h0, min=0)
        nw = torch.clamp(w0 + geom.kw, max=geom.W) - torch.clamp(w0, min=0)
    return (nh.reshape(-1, 1) * nw.reshape(1, -1)).to(torch.float32)


def _cpu_avg_value(levels, s_x, zx, geom, OH, OW, count_include_pad, divisor_override, mid_dtype):
    """u of the definition, a `mid_dtype` [B, C, OH, OW] tensor: the window sums of (l - z_x) are exact in float64 (a zero-padded
    tap adds 0), everything after them is torch float32 arithmetic, each step rounded once"""
    centred = levels.to(torch.float64) - zx.to(torch.float64).reshape(())
    S = F.avg_pool2d(centred, (geom.kh, geom.kw), (geom.sh, geom.sw), (geom.ph, geom.pw), bool(geom.ceil_mode), True, 1)
    a = S.to(torch.float32) * s_x.to(torch.float32).reshape(())
    v = a / _divisor(geom, OH, OW, count_include_pad, divisor_override)
    return v.to(mid_dtype)


def _avg(what, levels, s_x, zx, kernel_size, stride, padding, ceil_mode, count_include_pad, divisor_override, out_q, mid_dtype, out):
    _assert_has_ops()
    _check_levels(what, levels)
    _check_x_constants(what, s_x, zx)
    _check(divisor_override is None or int(divisor_override) >= 1, "%s: divisor_override must be at least 1, got %s" % (what, divisor_override))
    ydt, rng, qt = _check_out_q(what, out_q, mid_dtype)
    geom, OH, OW = _geometry(what, levels.shape, kernel_size, stride, padding, 1, ceil_mode, True)
    B, C = geom.B, geom.C
    on_gpu = _on_one_device(what, (levels, s_x, zx) + qt)
    if B == 0:
        return torch.empty((B, C, OH, OW), dtype=ydt, device=levels.device, memory_format=_CL)
    if not on_gpu:
        u = _cpu_avg_value(levels, s_x, zx, geom, OH, OW, count_include_pad, divisor_override, mid_dtype)
        return _cpu_finish(u, out_q, rng, ydt).contiguous(memory_format=_CL)
    lib = pool_w8_library()
    lx = levels.contiguous(memory_format=_CL)
    y = _take_out(what, out, (B, C, OH, OW), ydt, lx.device, _CL)
    avg = LsqPoolW8Avg(s_x.data_ptr(), zx.data_ptr(), qt[0].data_ptr() if out_q else None, qt[1].data_ptr() if out_q else None,
                       rng[0], rng[1], rng[2], rng[3], _DTYPE_CODE[mid_dtype], 1 if count_include_pad else 0,
                       0 if divisor_override is None else 1, 0 if divisor_override is None else int(divisor_override))
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_pool_w8_avg_forward, _LEVEL_CODE[lx.dtype], lx.data_ptr(), ctypes.byref(geom), ctypes.byref(avg),
                    y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_pool_w8_avg_forward", lib, _ERR)
    return y


def pool_w8_avg_q(levels, x_scale, x_zero, kernel_size, stride, padding, ceil_mode, count_include_pad, divisor_override, out_scale,
                  out_shift, quant_min, quant_max, type_min, type_max, mid_dtype, out=None):
    """levels [B, C, H, W] bytes -> the output quantizer's levels [B, C, OH, OW] (uint8 or int8) in channels-last memory.  `out`
    (not an argument of the op): a channels-last level tensor of that shape to write into, at any byte offset."""
    return _avg("lsq_avg_pool2d_q8_q", levels, x_scale, x_zero, kernel_size, stride, padding, ceil_mode, count_include_pad,
                divisor_override, (out_scale, out_shift, quant_min, quant_max, type_min, type_max), mid_dtype, out)


def pool_w8_avg(levels, x_scale, x_zero, kernel_size, stride, padding, ceil_mode, count_include_pad, divisor_override, out_dtype,
                out=None):
    """levels [B, C, H, W] bytes -> the averages as `out_dtype` floats [B, C, OH, OW] in channels-last memory."""
    return _avg("lsq_avg_pool2d_q8", levels, x_scale, x_zero, kernel_size, stride, padding, ceil_mode, count_include_pad,
                divisor_override, None, out_dtype, out)


def pool_w8_adaptive_kernel(H, W, output_size):
    """(kh, kw) = (H / OH, W / OW), the kernel and stride of adaptive pooling to `output_size` (None: that extent as it is);
    refused where the output size does not divide the input's evenly"""
    what = "lsq_adaptive_avg_pool2d_w8"
    oh, ow = output_size if isinstance(output_size, (tuple, list)) else (output_size, output_size)
    lib = pool_w8_library()
    geom = LsqPoolW8Geom(1, 1, int(H), int(W), 1, 1, 1, 1, 0, 0, 1, 1, 0)
    rc = lib.lsq_pool_w8_adaptive(int(H) if oh is None else int(oh), int(W) if ow is None else int(ow), ctypes.byref(geom))
    _status(rc, what, lib, _ERR)
    return geom.kh, geom.kw


# -------------------------------------------------------------------------------------------------
# plans: host only, nothing is launched
# -------------------------------------------------------------------------------------------------
def _plan(fn_name, what, B, C, H, W, kernel_size, stride, padding, dilation, ceil_mode, aligned):
    lib = pool_w8_library()
    kh, kw = _pair(what, "kernel_size", kernel_size)
    (sh, sw) = (kh, kw) if stride is None else _pair(what, "stride", stride)
    (ph, pw), (dh, dw) = _pair(what, "padding", padding), _pair(what, "dilation", dilation)
    geom = LsqPoolW8Geom(int(B), int(C), int(H), int(W), kh, kw, sh, sw, ph, pw, dh, dw, 1 if ceil_mode else 0)
    out = (ctypes.c_int32 * 8)()
    rc = getattr(lib, fn_name)(ctypes.byref(geom), 1 if aligned else 0, ctypes.byref(out))
    _status(rc, fn_name, lib, _ERR)
    return out


def pool_w8_plan_max(B, C, H, W, kernel_size, stride=None, padding=0, dilation=1, ceil_mode=False, aligned=True):
    """The launch liblsq_hip_pool_w8.so makes for a max pool of x [B, C, H, W] whose buffers are (not) 16-byte aligned: family
    "packets" / "generic", grid, block, pixels_per_lane, OH, OW, and unrolled_window: K where the packet kernel has the K x K window
    without dilation unrolled (2, 3), else 0."""
    out = _plan("lsq_pool_w8_plan_max", "pool_w8_plan_max", B, C, H, W, kernel_size, stride, padding, dilation, ceil_mode, aligned)
    return dict(family=_FAMILIES[out[0]], grid=out[1], block=out[2], pixels_per_lane=out[3], OH=out[4], OW=out[5], unrolled_window=out[7])


def pool_w8_plan_avg(B, C, H, W, kernel_size, stride=None, padding=0, ceil_mode=False, aligned=True):
    """The same for an average pool: family "packets" (a lane owns a window), "packets_shared" (`lanes_per_window` lanes of a
    workgroup share one; `packets_per_workgroup`, `lds_bytes`) or "generic"; `unrolled_window` as for the max pool."""
    out = _plan("lsq_pool_w8_plan_avg", "pool_w8_plan_avg", B, C, H, W, kernel_size, stride, padding, 1, ceil_mode, aligned)
    return dict(family=_FAMILIES[out[0]], grid=out[1], block=out[2], lanes_per_window=out[3], OH=out[4], OW=out[5], lds_bytes=out[6],
                packets_per_workgroup=out[7] if out[0] == 2 else 0, unrolled_window=out[7] if out[0] == 1 else 0)
