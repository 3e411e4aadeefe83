"""Host layer of rotary position embedding and the KV-cache append on 8-bit LEVELS (include/lsq_hip_rope_w8.h states the contract).
x is [B, T, H, D] levels with one scale and zero point, `cos` and `sin` are float32 [P, R / 2] tables that hold values of `mid_dtype`,
`positions` is an int32 tensor [B] on x's device (None: zeros) that is read in the kernel and never on the host, and token (b, t) has
the position p = positions[b] + t:

    d(l) = round_to(mid, (float(l) - float(zx)) * s_x)                                    LevelsTensor.dequantize(mid)
    pair (i, j):  half style j = i + R / 2, column i;  interleaved (2 i, 2 i + 1), column i;   c = cos[p, col], s = sin[p, col]
    u_i = round_to(mid, round_to(mid, d_i * c) - round_to(mid, d_j * s))
    u_j = round_to(mid, round_to(mid, d_j * c) + round_to(mid, d_i * s))                  features R .. D - 1:  u = d
    y = level(u) of (out_scale, out_shift, range), one byte -- or u itself

Three ops: `lsq_rope_w8_q8_q` (levels out), `lsq_rope_w8_q8` (floats out) and `lsq_kv_copy_w8` (COPY: y byte = x byte, into `out`).
Without `scatter` token t is written at output token t; with it at output token p.  A token with p < 0 or p >= P (COPY: p >= Tout),
or with scatter p >= Tout, is not written at all.  x is read IN PLACE where its innermost stride is 1 (a q, k or v view of a qkv
buffer), and `out` (not an argument of the rotating ops) may be any [B, Tout, H, D] view with unit innermost stride whose rows do
not overlap, e.g. the `.permute(0, 2, 1, 3)` view of a [B, H, Tmax, D] cache.  An `out` that overlaps x, the tables or
`positions` is refused on the host, on both devices: the op in place is not served.

The CPU path IS the definition: `dequantize(mid)`, `torch.mul`, `torch.sub` / `torch.add` on `mid_dtype` tensors, the existing
`cpu_levels`, and plain index assignment for the placement.  Every op first calls the library's plan function (host only: it runs
without a GPU and enqueues nothing), which refuses an illegal shape with the library's message; the GPU path is then ONE ctypes call
that enqueues, nothing is read back, and it equals the CPU path bit for bit.
"""
import ctypes

import torch

from ._abi import _DTYPE_CODE, LsqRopeW8Geom, LsqRopeW8In, LsqRopeW8Out, _assert_has_ops, rope_w8_library
from ._cpu_host import _require_cpu
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._w8_host_common import _LEVEL_CODE, _check_out_q, _check_x_constants, _cpu_finish, _name, _status

_ERR = "lsq_rope_w8_last_error"
_FAMILIES = ("generic", "packets")
_KERNELS = ("generic", "packets_half", "packets_interleaved", "copy_packets", "copy_generic")


def _strides3(t):
    """the strides of the first three axes of t [B, T, H, D] in elements; an axis of one element has no stride to speak of"""
    return tuple(int(s) if int(n) > 1 else 0 for n, s in zip(t.shape[:3], t.stride()[:3]))


def _span(t):
    """(first byte, one past the last byte) that t's elements occupy"""
    last = sum((int(n) - 1) * int(st) for n, st in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()


def _refuse_overlap(what, y, others):
    """what the library refuses on the GPU holds on both devices: y must not overlap x, the tables or positions"""
    if not y.numel():
        return
    lo, hi = _span(y)
    for name, t in others:
        if t is not None and t.numel() and t.device == y.device:
            a, b = _span(t)
            _check(not (lo < b and a < hi), "%s: `out` overlaps %s: the op in place is not served" % (what, name))


def cpu_rope_value(x_levels, s_x, zx, cos, sin, p, mid_dtype, interleaved):
    """u of the definition for x [B, T, H, D] and the positions p (int64 [B, T], every one a row of the tables): a `mid_dtype`
    tensor [B, T, H, D]"""
    d = ((x_levels.to(torch.float32) - zx.detach().reshape(()).to(torch.float32)) * s_x.detach().reshape(())).to(mid_dtype)
    half = int(cos.shape[1])
    R = 2 * half
    c, s = cos[p].to(mid_dtype).unsqueeze(2), sin[p].to(mid_dtype).unsqueeze(2)        # [B, T, 1, R / 2]: the same for every head
    rot, rest = d[..., :R], d[..., R:]
    xi, xj = (rot[..., 0::2], rot[..., 1::2]) if interleaved else (rot[..., :half], rot[..., half:])
    ui = torch.sub(torch.mul(xi, c), torch.mul(xj, s))
    uj = torch.add(torch.mul(xj, c), torch.mul(xi, s))
    u = torch.stack((ui, uj), -1).flatten(-2) if interleaved else torch.cat((ui, uj), -1)
    return torch.cat((u, rest), -1)


def cpu_place(y, val, positions, limit, scatter):
    """the placement of the definition by plain index assignment: val [B, T, H, D] into y [B, Tout, H, D]"""
    B, T = int(val.shape[0]), int(val.shape[1])
    Tout = int(y.shape[1])
    t = torch.arange(T, dtype=torch.int64)
    for b in range(B):
        p = t + (0 if positions is None else int(positions[b]))
        ok = (p >= 0) & (p < limit)
        if scatter:
            ok &= p < Tout
        y[b, (p if scatter else t)[ok]] = val[b, ok]


def _common(what, x, positions, out, ydt, scatter):
    """x as the kernels read it, y, and the geometry's shape part after the checks the host can make"""
    _check(x.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x.dtype)))
    _check(x.dim() == 4, "%s: the levels must be [B, T, H, D], got %s" % (what, tuple(x.shape)))
    B, T, H, D = (int(n) for n in x.shape)
    if positions is not None:
        _check(positions.dtype == torch.int32 and tuple(positions.shape) == (B,) and positions.is_contiguous(),
               "%s: positions must be a dense int32 tensor of [%d], one entry per batch, got '%s' %s"
               % (what, B, _name(positions.dtype), tuple(positions.shape)))
        _check(positions.device == x.device, "%s: positions must be on the levels' device (%s), got %s" % (what, x.device, positions.device))
    if out is None:
        _check(not scatter, "%s: scatter needs `out`, the tensor the tokens are scattered into" % what)
        y = torch.empty((B, T, H, D), dtype=ydt, device=x.device)
    else:
        _check(out.dtype == ydt and out.dim() == 4 and (int(out.shape[0]), int(out.shape[2]), int(out.shape[3])) == (B, H, D) and
               (D == 1 or out.stride(-1) == 1),
               "%s: `out` must be a %s tensor of shape [%d, Tout, %d, %d] whose innermost stride is 1, got '%s' %s"
               % (what, _name(ydt), B, H, D, _name(out.dtype), tuple(out.shape)))
        y = out
    if D != 1 and x.stride(-1) != 1:
        x = x.contiguous()          # as lsq_bmm_w8_q does: only a view without unit innermost stride is made dense
    return x, y, (B, T, H, D, int(y.shape[1]))


def _rope(what, x, s_x, zx, cos, sin, out_q, mid_dtype, positions, interleaved, out, scatter):
    _assert_has_ops()
    scatter, interleaved = bool(scatter), bool(interleaved)
    ydt, rng, qt = _check_out_q(what, out_q, mid_dtype)
    x, y, (B, T, H, D, Tout) = _common(what, x, positions, out, ydt, scatter)
    _check_x_constants(what, s_x, zx)
    _check(cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.dim() == 2 and tuple(cos.shape) == tuple(sin.shape) and
           cos.is_contiguous() and sin.is_contiguous(),
           "%s: cos and sin must be dense float32 tensors of one shape [P, R / 2] (lsq_rope_tables), got '%s' %s and '%s' %s"
           % (what, _name(cos.dtype), tuple(cos.shape), _name(sin.dtype), tuple(sin.shape)))
    P, R = int(cos.shape[0]), 2 * int(cos.shape[1])
    tensors = (x, s_x, zx, cos, sin) + qt + (() if positions is None else (positions,)) + (() if out is None else (out,))
    on_gpu = any(t.is_cuda for t in tensors)
    lib = rope_w8_library()
    _refuse_overlap(what, y, (("x", x), ("cos", cos), ("sin", sin), ("positions", positions)))
    if x.numel() and y.numel():
        geom = LsqRopeW8Geom(B, T, H, D, R, P, Tout, *_strides3(x), *_strides3(y), _LEVEL_CODE[x.dtype], 1 if interleaved else 0,
                             1 if scatter else 0, 0)
        plan = (ctypes.c_int32 * 8)()
        _status(lib.lsq_rope_w8_plan(ctypes.byref(geom), y.element_size(), ctypes.byref(plan)), what, lib, _ERR)       # the shape's checks
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    if not (x.numel() and y.numel()):
        return y
    if not on_gpu:
        t = torch.arange(T, dtype=torch.int64).reshape(1, T)
        p = t + (0 if positions is None else positions.to(torch.int64).reshape(B, 1))
        u = cpu_rope_value(x, s_x, zx, cos, sin, p.clamp(0, P - 1), mid_dtype, interleaved)       # (a skipped token's value is not placed)
        cpu_place(y, _cpu_finish(u, out_q, rng, ydt), positions, P, scatter)
        return y
    side = LsqRopeW8In(s_x.data_ptr(), zx.data_ptr())
    o = LsqRopeW8Out(out_q[0].data_ptr() if out_q else None, out_q[1].data_ptr() if out_q else None, rng[0], rng[1], rng[2], rng[3],
                     _DTYPE_CODE[mid_dtype])
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_rope_w8, ctypes.byref(geom), ctypes.byref(side), ctypes.byref(o), cos.data_ptr(), sin.data_ptr(),
                    None if positions is None else positions.data_ptr(), x.data_ptr(), y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_rope_w8", lib, _ERR)
    return y


def rope_w8_q(x_levels, x_scale, x_zero, cos, sin, out_scale, out_shift, quant_min, quant_max, type_min, type_max, mid_dtype, positions=None,
              interleaved=False, out=None, scatter=False):
    """x's levels [B, T, H, D] rotated by the tables at the positions `positions[b] + t` -> the output quantizer's levels [B, T, H, D]
    (uint8 or int8, dense).  `out` and `scatter` (not arguments of the op): a [B, Tout, H, D] view to write into, token t at t or,
    with `scatter`, at its position; tokens outside the tables or outside `out` are not written."""
    return _rope("lsq_rope_w8_q8_q", x_levels, x_scale, x_zero, cos, sin, (out_scale, out_shift, quant_min, quant_max, type_min, type_max),
                 mid_dtype, positions, interleaved, out, scatter)


def rope_w8(x_levels, x_scale, x_zero, cos, sin, out_dtype, positions=None, interleaved=False, out=None, scatter=False):
    """the same -> the rotated values as `out_dtype` floats [B, T, H, D]."""
    return _rope("lsq_rope_w8_q8", x_levels, x_scale, x_zero, cos, sin, None, out_dtype, positions, interleaved, out, scatter)


def rope_w8_kv_copy(x_levels, out, positions=None, scatter=True):
    """COPY: x's levels [B, T, H, D] into `out` [B, Tout, H, D] (the same dtype), token t at output token t or, with `scatter`, at
    `positions[b] + t`; a token whose position lies outside 0 .. Tout - 1 is not written.  Returns nothing: `out` is written."""
    what = "lsq_kv_copy_w8"
    _assert_has_ops()
    scatter = bool(scatter)
    _check(out is not None and out.dtype == x_levels.dtype, "%s: x and `out` must have one level dtype" % what)
    x, y, (B, T, H, D, Tout) = _common(what, x_levels, positions, out, x_levels.dtype, scatter)
    tensors = (x, y) + (() if positions is None else (positions,))
    on_gpu = any(t.is_cuda for t in tensors)
    lib = rope_w8_library()
    _refuse_overlap(what, y, (("x", x), ("positions", positions)))
    if x.numel() and y.numel():
        geom = LsqRopeW8Geom(B, T, H, D, 0, 0, Tout, *_strides3(x), *_strides3(y), _LEVEL_CODE[x.dtype], 0, 1 if scatter else 0, 1)
        plan = (ctypes.c_int32 * 8)()
        _status(lib.lsq_rope_w8_plan(ctypes.byref(geom), 1, ctypes.byref(plan)), what, lib, _ERR)
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    if not (x.numel() and y.numel()):
        return
    if not on_gpu:
        cpu_place(y, x, positions, Tout, scatter)
        return
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_rope_w8, ctypes.byref(geom), None, None, None, None, None if positions is None else positions.data_ptr(),
                    x.data_ptr(), y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_rope_w8", lib, _ERR)


def rope_w8_plan(B, T, H, D, R=None, P=1, Tout=None, x_strides=None, y_strides=None, aligned=True, y_elem=1, x_dtype=torch.uint8,
                 interleaved=False, scatter=False, copy=False):
    """The launch liblsq_hip_rope_w8.so makes for x [B, T, H, D] into y [B, Tout, H, D] (`Tout`: T by default) with the rotary
    dimension R (D by default) and tables of P positions; `*_strides`: the three outer strides in elements, dense by default;
    `aligned`: x, y and the tables are 16-byte aligned; `y_elem`: the bytes of one element of y; `copy`: the COPY mode.  Returns
    family "packets" / "generic", grid, block, heads_per_lane, units (work units per token and head), rotating_units, lds_bytes and
    kernel ("packets_half", "packets_interleaved", "generic", "copy_packets", "copy_generic")."""
    B, T, H, D = int(B), int(T), int(H), int(D)
    Tout = T if Tout is None else int(Tout)
    xs = (T * H * D, H * D, D) if x_strides is None else tuple(int(v) for v in x_strides)
    ys = (Tout * H * D, H * D, D) if y_strides is None else tuple(int(v) for v in y_strides)
    geom = LsqRopeW8Geom(B, T, H, D, 0 if copy else int(D if R is None else R), 0 if copy else int(P), Tout, *xs, *ys, _LEVEL_CODE[x_dtype],
                         1 if interleaved else 0, 1 if scatter else 0, 1 if copy else 0)
    out = (ctypes.c_int32 * 8)()
    lib = rope_w8_library()
    _status(lib.lsq_rope_w8_plan(ctypes.byref(geom), int(y_elem) if aligned else 0, ctypes.byref(out)), "lsq_rope_w8_plan", lib, _ERR)
    return dict(family=_FAMILIES[out[0]], grid=out[1], block=out[2], heads_per_lane=out[3], units=out[4], rotating_units=out[5],
                lds_bytes=out[6], kernel=_KERNELS[out[7]])
