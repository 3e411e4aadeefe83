"""Host layer of LayerNorm and RMSNorm on 8-bit LEVELS (include/lsq_hip_norm_w8.h states the contract): what keeps a converted
ConvNeXt block and a converted token block in levels at the norm.

x is rows of C level bytes of ONE per-tensor quantizer (s_x, zx).  With b_i the level as an integer, every integer exact and every
float32 step one rounded operation:

    LayerNorm   S1 = sum b    S2 = sum b^2    V = C S2 - S1^2    n_i = C b_i - S1          (zx is not used)
                var = float(V) / (float(C) * float(C))    e = eps / (s_x * s_x)
                r = 1 / sqrt(var + e)    rc = r / float(C)    t_i = float(n_i) * rc
    RMSNorm     d_i = b_i - zx    Q = sum d^2    var = float(Q) / float(C)    r as above    t_i = float(d_i) * r
    both        a_i = (t_i * w[c]) + bias[c]  (either may be absent)    u_i = round_to(mid_dtype, a_i)
                y_i = level(u_i) of (out_scale, out_shift, range), one byte -- or u_i itself, stored as mid_dtype

Four ops: `lsq_layer_norm_w8_q8_q` / `lsq_rms_norm_w8_q8_q` (levels out) and `lsq_layer_norm_w8_q8` / `lsq_rms_norm_w8_q8` (floats
out).  They normalise the LAST axis of a level tensor of any shape and return that shape, dense.

The CPU path IS the definition: int64 torch sums, torch float32 ops one at a time, `.to(mid_dtype)` and the existing `cpu_levels`.
Every op first calls the library's plan function (host only, it runs without a GPU and enqueues nothing), which refuses an illegal
shape with the library's message.  The GPU path is then ONE ctypes call that enqueues; nothing is read back, and it equals the CPU
path bit for bit.  It is not ATen's `layer_norm`: against `F.layer_norm(x.dequantize())` taken to levels, a small share of the
outputs differs by one level.
"""
import ctypes
import math

import torch

from ._abi import _DTYPE_CODE, LsqNormW8Consts, LsqNormW8Geom, _assert_has_ops, norm_w8_library
from ._hip_host import _check, _on_device, _stream_of
from ._w8_host_common import (_FLOATS, _LEVEL_CODE, _check_out_q, _check_x_constants, _cpu_finish, _name, _on_one_device, _status,
                              _take_out)

_KINDS = {"layer": 0, "rms": 1}
_FAMILIES = ("generic", "packets")
_PARAMS = ("none", "registers", "lds")
_ERR = "lsq_norm_w8_last_error"


def _plan(lib, what, R, C, kind, x_dtype, aligned, has_w, has_b):
    out = (ctypes.c_int32 * 8)()
    geom = LsqNormW8Geom(int(R), int(C), _KINDS[kind], _LEVEL_CODE[x_dtype])
    _status(lib.lsq_norm_w8_plan(ctypes.byref(geom), 1 if aligned else 0, 1 if has_w else 0, 1 if has_b else 0, ctypes.byref(out)),
            what, lib, _ERR)
    return out


def cpu_norm_value(kind, x_levels, s_x, zx, weight, bias, eps, mid_dtype):
    """u of the definition, a `mid_dtype` tensor of x's shape"""
    f32 = torch.float32
    b = x_levels.to(torch.int64)
    C = int(b.shape[-1])
    fC = torch.full((), C, dtype=f32)
    s = s_x.detach().reshape(())
    e = torch.full((), eps, dtype=f32) / (s * s)
    if kind == "layer":
        S1 = b.sum(-1, keepdim=True)
        S2 = (b * b).sum(-1, keepdim=True)
        V = C * S2 - S1 * S1
        num = C * b - S1
        var = V.to(f32) / (fC * fC)
    else:
        num = b - zx.reshape(()).to(torch.int64)
        var = (num * num).sum(-1, keepdim=True).to(f32) / fC
    # the correctly rounded float32 square root: torch's float32 sqrt on the CPU is NOT (it is off by one ulp for about 0.7 % of
    # its arguments); the float64 root of a float32 number, rounded to float32, is (53 bits are more than 2 * 24 + 2)
    root = torch.sqrt((var + e).to(torch.float64)).to(f32)
    r = torch.ones_like(root) / root
    t = num.to(f32) * (r / fC if kind == "layer" else r)
    if weight is not None:
        t = t * weight.detach().to(f32)
    if bias is not None:
        t = t + bias.detach().to(f32)
    return t.to(mid_dtype)


def _norm(kind, what, x_levels, s_x, zx, weight, bias, eps, out_q, mid_dtype, out):
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    _check(x_levels.dim() >= 1, "%s: the levels need at least one axis" % what)
    _check_x_constants(what, s_x, zx)
    eps = float(eps)
    _check(eps >= 0.0 and not math.isnan(eps), "%s: eps = %r must be a number that is not negative" % (what, eps))
    C = int(x_levels.shape[-1])
    tensors = (x_levels, s_x, zx)
    pdt = None
    for name, p in (("weight", weight), ("bias", bias)):
        if p is None:
            continue
        _check(p.dtype in _FLOATS and tuple(p.shape) == (C,), "%s: %s must be a float32, bfloat16 or float16 tensor of [%d], got '%s' %s"
               % (what, name, C, _name(p.dtype), tuple(p.shape)))
        _check(pdt is None or p.dtype == pdt, "%s: weight and bias must have one dtype, got '%s' and '%s'" % (what, _name(pdt), _name(p.dtype)))
        pdt = p.dtype
        tensors += (p,)
    ydt, rng, qt = _check_out_q(what, out_q, mid_dtype)
    R = x_levels.numel() // max(C, 1)
    lib = norm_w8_library()
    _plan(lib, what, max(R, 1), C, kind, x_levels.dtype, True, weight is not None, bias is not None)       # the shape's checks
    on_gpu = _on_one_device(what, tensors + qt)
    if R == 0:
        return torch.empty(x_levels.shape, dtype=ydt, device=x_levels.device)
    if not on_gpu:
        u = _cpu_finish(cpu_norm_value(kind, x_levels, s_x, zx, weight, bias, eps, mid_dtype), out_q, rng, ydt).contiguous()
        if out is not None:
            _take_out(what, out, tuple(x_levels.shape), ydt, x_levels.device).copy_(u)
            return out
        return u
    lx = x_levels.contiguous()
    w = None if weight is None else weight.detach().contiguous()
    b = None if bias is None else bias.detach().contiguous()
    y = _take_out(what, out, tuple(x_levels.shape), ydt, lx.device)
    consts = LsqNormW8Consts(s_x.data_ptr(), zx.data_ptr(), None if w is None else w.data_ptr(), None if b is None else b.data_ptr(),
                             qt[0].data_ptr() if out_q else None, qt[1].data_ptr() if out_q else None,
                             _DTYPE_CODE[pdt] if pdt is not None else _DTYPE_CODE[torch.float32], rng[0], rng[1], rng[2], rng[3],
                             _DTYPE_CODE[mid_dtype], eps)
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_norm_w8, ctypes.byref(LsqNormW8Geom(R, C, _KINDS[kind], _LEVEL_CODE[lx.dtype])), ctypes.byref(consts),
                    lx.data_ptr(), y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_norm_w8", lib, _ERR)
    return y


def norm_w8_layer_q(x_levels, x_scale, x_zero, weight, bias, eps, out_scale, out_shift, quant_min, quant_max, type_min, type_max, mid_dtype,
                    out=None):
    """LayerNorm over the last axis of x's levels -> the output quantizer's levels in x's shape (uint8 or int8, dense).  `out` (not
    an argument of the op): a tensor like the result to write into, at any byte offset."""
    return _norm("layer", "lsq_layer_norm_w8_q8_q", x_levels, x_scale, x_zero, weight, bias, eps,
                 (out_scale, out_shift, quant_min, quant_max, type_min, type_max), mid_dtype, out)


def norm_w8_layer(x_levels, x_scale, x_zero, weight, bias, eps, out_dtype, out=None):
    """the same -> the normalised values as `out_dtype` floats in x's shape."""
    return _norm("layer", "lsq_layer_norm_w8_q8", x_levels, x_scale, x_zero, weight, bias, eps, None, out_dtype, out)


def norm_w8_rms_q(x_levels, x_scale, x_zero, weight, bias, eps, out_scale, out_shift, quant_min, quant_max, type_min, type_max, mid_dtype,
                  out=None):
    """RMSNorm over the last axis of x's levels -> the output quantizer's levels in x's shape."""
    return _norm("rms", "lsq_rms_norm_w8_q8_q", x_levels, x_scale, x_zero, weight, bias, eps,
                 (out_scale, out_shift, quant_min, quant_max, type_min, type_max), mid_dtype, out)


def norm_w8_rms(x_levels, x_scale, x_zero, weight, bias, eps, out_dtype, out=None):
    """the same -> the normalised values as `out_dtype` floats in x's shape."""
    return _norm("rms", "lsq_rms_norm_w8_q8", x_levels, x_scale, x_zero, weight, bias, eps, None, out_dtype, out)


# -------------------------------------------------------------------------------------------------
# the plan: host only, nothing is launched
# -------------------------------------------------------------------------------------------------
def norm_w8_plan(R, C, aligned=True, has_weight=True, has_bias=True, kind="layer", x_dtype=torch.uint8):
    """The launch liblsq_hip_norm_w8.so makes for R rows of C levels whose buffers are (not) 16-byte aligned: family "packets" /
    "generic", grid, block, lanes_per_row (L), packets_per_lane (P), rows_per_workgroup, params ("none" / "registers" / "lds": where
    a lane's w and bias values live) and lds_bytes."""
    out = _plan(norm_w8_library(), "lsq_norm_w8_plan", R, C, kind, x_dtype, aligned, has_weight, has_bias)
    return dict(family=_FAMILIES[out[0]], grid=out[1], block=out[2], lanes_per_row=out[3], packets_per_lane=out[4],
                rows_per_workgroup=out[5], params=_PARAMS[out[6]], lds_bytes=out[7])
