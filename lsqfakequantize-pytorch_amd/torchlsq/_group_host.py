"""Host layer of the group-wise ops: one scale / shift per run of `group_size` (G) consecutive elements of the last dim.

GPU tensors go to liblsq_hip_group.so (include/lsq_hip_group.h) with one ctypes call per op; CPU tensors go to the
per-channel kernels of liblsq_cpu.so on the [n / G, G] view (axis 0), which is what a group IS, value for value.
`group_forward_multi` / `group_backward_multi`: many GPU tensors of one dtype in one ctypes call each way (the fused calls
of the same library), with the same checks and layout rules.
Checks and layout rules as in _hip_host.py: the flat stream needs x in row-major order (a non-contiguous x is made
contiguous first, like a non-dense per-channel input); element-aligned views (x[1:]) run in place.
"""
import ctypes

import torch

from . import _abi
from ._abi import _DTYPE_CODE, LsqGroupItem, _assert_has_ops, group_library
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


def _fwd_buffers(x, scale, shift):
    """the inputs as the flat stream reads them: contiguous x, scale and shift"""
    return x.contiguous(), scale.contiguous(), shift.contiguous()


def _bwd_buffers(grad, x, scale, shift):
    """(grad, x, scale, shift) as the flat stream reads them -- contiguous, grad in x's shape -- and the outputs (dx,
    d_scale, d_shift), the parameter gradients in the parameters' shapes"""
    xd, sc, sh = _fwd_buffers(x, scale, shift)
    gd = grad.contiguous() if grad.shape == x.shape else grad.reshape(x.shape).contiguous()
    pd = _param_dtype(x)
    outs = (torch.empty_like(xd), torch.empty(scale.shape, dtype=pd, device=x.device),
            torch.empty(shift.shape, dtype=pd, device=x.device))
    return (gd, xd, sc, sh), outs


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
    xd, sc, sh = _fwd_buffers(x, scale, shift)
    y = None if levels_only else torch.empty_like(xd)
    has_aux = levels_bias is not None or want_mask
    if xd.numel() == 0:
        lv = torch.empty(x.shape, dtype=torch.int8, device=x.device)
        return lv if levels_only else ((y, lv) if has_aux else y)
    lv, ex = _aux_output(xd, levels_bias, want_mask)
    _, pref = _params(qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode)
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
    (gd, xd, sc, sh), (dx, ds, db) = _bwd_buffers(grad, x, scale, shift)
    _, pref = _params(qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode)
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


def _multi_common(what, xs, scales, shifts, group_sizes):
    """checks of the single calls for every tensor; (device index, dtype code)"""
    n = len(xs)
    _check(n > 0 and len(scales) == n and len(shifts) == n and len(group_sizes) == n,
           "%s: xs, scales, shifts and group sizes must be non-empty lists of the same length" % what)
    x0 = xs[0]
    for x, sc, sh, G in zip(xs, scales, shifts, group_sizes):
        check_forward_dtypes(x, sc, sh)
        check_group_args(x, sc, sh, G)
        _check(x.dtype == x0.dtype, "%s: every tensor of one call must have the same dtype" % what)
        _require_gpu(what, x0, x, sc, sh)
    return x0.device.index, _DTYPE_CODE[x0.dtype]


def group_forward_multi(xs, scales, shifts, group_sizes, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode):
    """[y_i] = [group_forward(x_i, ...)]: one ctypes call, one launch per class of reduction and per 28 tensors"""
    _assert_has_ops()
    lib = group_library()
    idx, code = _multi_common("lsq_group_multi_forward", xs, scales, shifts, group_sizes)
    _, pref = _params(qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode)
    items = (LsqGroupItem * len(xs))()
    keep, ys = [], []
    for k, (x, sc, sh, G) in enumerate(zip(xs, scales, shifts, group_sizes)):
        xd, scc, shc = _fwd_buffers(x, sc, sh)
        y = torch.empty_like(xd)
        keep += [xd, scc, shc]
        ys.append(y)
        it = items[k]
        it.x, it.y, it.scale, it.shift = xd.data_ptr(), y.data_ptr(), scc.data_ptr(), shc.data_ptr()
        it.n, it.group_size = xd.numel(), G
    rc = _on_device(idx, lib.lsq_group_multi_forward, code, items, len(xs), pref, _stream_of(idx))
    if rc:
        _group_status(rc, "lsq_group_multi_forward")
    return ys


def group_backward_multi(grads, xs, scales, shifts, group_sizes, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode):
    """[(dx_i, d_scale_i, d_shift_i)] = [group_backward(grad_i, x_i, ...)]: one ctypes call; the parameter gradients come
    back in the parameters' shapes"""
    _assert_has_ops()
    lib = group_library()
    idx, code = _multi_common("lsq_group_multi_backward", xs, scales, shifts, group_sizes)
    _check(len(grads) == len(xs), "lsq_group_multi_backward: one gradient per tensor")
    _, pref = _params(qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode)
    items = (LsqGroupItem * len(xs))()
    keep, outs = [], []
    for k, (g, x, sc, sh, G) in enumerate(zip(grads, xs, scales, shifts, group_sizes)):
        check_backward_dtypes(g, x, sc, sh)
        _require_gpu("lsq_group_multi_backward", x, g)
        (gd, xd, scc, shc), (dx, ds, db) = _bwd_buffers(g, x, sc, sh)
        keep += [xd, gd, scc, shc]
        outs.append((dx, ds, db))
        it = items[k]
        it.x, it.grad, it.dx, it.scale, it.shift = xd.data_ptr(), gd.data_ptr(), dx.data_ptr(), scc.data_ptr(), shc.data_ptr()
        it.ds, it.db, it.n, it.group_size = ds.data_ptr(), db.data_ptr(), xd.numel(), G
    rc = _on_device(idx, lib.lsq_group_multi_backward, code, items, len(xs), pref, _stream_of(idx))
    if rc:
        _group_status(rc, "lsq_group_multi_backward")
    return outs


def group_multi_plan(dtype, sizes, group_sizes):
    """How the fused calls of liblsq_hip_group.so launch tensors of `sizes` elements with `group_sizes` -- host only, nothing is
    launched (lsq_group_multi_plan): (per tensor (launch index, forward workgroups, backward workgroups), launches)"""
    lib = group_library()
    n = len(sizes)
    items = (LsqGroupItem * max(n, 1))()
    for k, (m, G) in enumerate(zip(sizes, group_sizes)):
        items[k].n, items[k].group_size = int(m), int(G)
    out = (ctypes.c_int32 * (3 * max(n, 1)))()
    launches = ctypes.c_int32(0)
    rc = lib.lsq_group_multi_plan(_DTYPE_CODE[dtype], items, n, out, ctypes.byref(launches))
    if rc:
        _group_status(rc, "lsq_group_multi_plan")
    return [(out[3 * k], out[3 * k + 1], out[3 * k + 2]) for k in range(n)], launches.value
