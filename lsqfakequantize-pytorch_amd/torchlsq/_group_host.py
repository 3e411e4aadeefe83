"""Host layer of the group-wise ops: one scale / shift per run of `group_size` (G) consecutive elements of the last dim.

GPU tensors go to liblsq_hip_group.so (include/lsq_hip_group.h) with one ctypes call per op; CPU tensors go to the
per-channel kernels of liblsq_cpu.so on the [n / G, G] view (axis 0), which is what a group IS, value for value.
Checks and layout rules as in _hip_host.py: the flat stream needs x in row-major order (a non-contiguous x is made
contiguous first, like a non-dense per-channel input); element-aligned views (x[1:]) run in place.
"""
import ctypes

import torch

from . import _abi
from ._abi import _DTYPE_CODE, _assert_has_ops, group_library
from ._hip_host import (_aux_output, _check, _on_device, _param_dtype, _params, _require_gpu, _stream_of,
                        check_backward_dtypes, check_forward_dtypes)
from ._cpu_host import cpu_backward, cpu_forward, cpu_levels


def check_group_args(x, scale, shift, group_size):
    """x.shape[-1] % G == 0 and one scale / shift per group (any shape with x.numel() // G elements)"""
    _check(isinstance(group_size, int) and group_size >= 1, "group_size must be a positive integer")
    _check(x.dim() >= 1, "lsq_per_group: x needs at least one dimension")
    _check(x.size(-1) % group_size == 0,
           "lsq_per_group: the last dimension (%d) is not a multiple of group_size %d" % (x.size(-1), group_size))
    groups = x.numel() // group_size
    _check(scale.numel() == groups and shift.numel() == groups,
           "lsq_per_group: scale and shift need x.numel() // group_size = %d elements, got %d and %d" %
           (groups, scale.numel(), shift.numel()))


def _group_status(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, _abi._GROUP_LIB.lsq_group_last_error().decode("utf-8", "replace")))


def group_forward(x, scale, shift, group_size, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode,
                  levels_bias=None, want_mask=False, levels_only=False):
    """y (contiguous, x's shape); with levels_bias / want_mask also the one byte per element; levels_only: the bytes alone"""
    _assert_has_ops()
    check_forward_dtypes(x, scale, shift)
    check_group_args(x, scale, shift, group_size)
    if not x.is_cuda:
        return _cpu_forward(x, scale, shift, group_size, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode,
                            levels_bias, want_mask, levels_only)
    lib = group_library()
    _require_gpu("lsq_forward_per_group", x, scale, shift)
    xd = x.contiguous()
    y = None if levels_only else torch.empty_like(xd)
    has_aux = levels_bias is not None or want_mask
    if xd.numel() == 0:
        lv = torch.empty(x.shape, dtype=torch.int8, device=x.device)
        return lv if levels_only else ((y, lv) if has_aux else y)
    lv, ex = _aux_output(xd, levels_bias, want_mask)
    _, pref = _params(qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode)
    sc, sh = scale.contiguous(), shift.contiguous()
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_group_forward, _DTYPE_CODE[x.dtype], xd.data_ptr(), None if levels_only else y.data_ptr(),
                    xd.numel(), group_size, sc.data_ptr(), sh.data_ptr(), pref, ex, _stream_of(idx))
    if rc:
        _group_status(rc, "lsq_group_forward")
    if levels_only:
        return lv
    return (y, lv) if has_aux else y


def group_backward(grad, x, scale, shift, group_size, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode):
    """(dx, d_scale, d_shift); the parameter gradients come back in the parameters' shapes"""
    _assert_has_ops()
    check_backward_dtypes(grad, x, scale, shift)
    check_group_args(x, scale, shift, group_size)
    if x.numel() == 0:
        return x.clone(), scale.clone(), shift.clone()
    if not x.is_cuda:
        _check(not grad.is_cuda, "lsq_backward_per_group: grad and x must be on the same device")
        rows = x.numel() // group_size
        dx, ds, db = cpu_backward(grad.reshape(rows, group_size), x.reshape(rows, group_size), scale.reshape(-1),
                                  shift.reshape(-1), 0, True, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode)
        return dx.reshape(x.shape), ds.reshape(scale.shape), db.reshape(shift.shape)
    lib = group_library()
    _require_gpu("lsq_backward_per_group", x, grad, scale, shift)
    xd = x.contiguous()
    gd = grad.contiguous() if grad.shape == x.shape else grad.reshape(x.shape).contiguous()
    dx = torch.empty_like(xd)
    pd = _param_dtype(x)
    ds = torch.empty(scale.shape, dtype=pd, device=x.device)
    db = torch.empty(shift.shape, dtype=pd, device=x.device)
    _, pref = _params(qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode)
    sc, sh = scale.contiguous(), shift.contiguous()
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_group_backward, _DTYPE_CODE[x.dtype], gd.data_ptr(), xd.data_ptr(), dx.data_ptr(),
                    ds.data_ptr(), db.data_ptr(), xd.numel(), group_size, sc.data_ptr(), sh.data_ptr(), pref, _stream_of(idx))
    if rc:
        _group_status(rc, "lsq_group_backward")
    return dx, ds, db


def _cpu_forward(x, scale, shift, group_size, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode, levels_bias,
                 want_mask, levels_only):
    rows = x.numel() // group_size
    x2, s, b = x.reshape(rows, group_size), scale.reshape(-1), shift.reshape(-1)
    if levels_only:
        return cpu_levels(x2, s, b, 0, True, qmin, qmax, tmin, tmax, levels_bias).reshape(x.shape)
    _check(levels_bias is None and not want_mask, "lsq_per_group: the one-byte outputs are GPU-only")
    return cpu_forward(x2, s, b, 0, True, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode).reshape(x.shape)


def group_plan(dtype, n, group_size):
    """The launches liblsq_hip_group.so makes for (dtype, n, G) -- host only, nothing is launched (lsq_group_plan)."""
    lib = group_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_group_plan(_DTYPE_CODE[dtype], int(n), int(group_size), ctypes.byref(out))
    if rc:
        _group_status(rc, "lsq_group_plan")
    return dict(fwd_grid=out[0], bwd_grid=out[1], block=out[2], form="packet" if out[3] else "element", lanes_per_group=out[4],
                reduction="butterfly" if out[5] == 1 else "scan", vec=out[6])
