"""Host layer of the gated product of a gated MLP on 8-bit LEVELS (include/lsq_hip_glu_w8.h states the contract): act(gate) * up
with the activation as a 256-entry float table on the gate byte, what keeps a converted Llama-style MLP in levels between its
gate_up linear and its down linear.

    a = table[gate byte]                                              a value of mid_dtype, stored as float32
    d = float(round_to(mid, (float(l_u) - float(z_u)) * s_u))         LevelsTensor.dequantize(mid)
    t = float(round_to(mid, a * d))                                   one rounded fp32 multiply
    y = level(t) of (out_scale, out_shift, range), one byte -- or t itself, stored as mid_dtype

Two ops: `lsq_glu_w8_q8_q` (levels out) and `lsq_glu_w8_q8` (floats out).  gate and up are level tensors of one shape [.., C];
each is read IN PLACE where its innermost stride is 1 and its leading axes collapse to one row stride >= C -- the halves
`gu[..., :C]` and `gu[..., C:]` of a fused linear's output do -- and is made dense first otherwise.  The result is a new dense
tensor of that shape.

The CPU path IS the definition: the existing ops composed -- the table gathered with the gate bytes, `.to(mid_dtype)`, torch's
float32 arithmetic and multiply in `mid_dtype`, and the existing `cpu_levels`.  Every op first calls the library's plan function
(host only, it runs without a GPU and enqueues nothing), which refuses an illegal shape with the library's message.  The GPU path
is then ONE ctypes call that enqueues one launch; nothing is read back, and it equals the CPU path bit for bit for the same table.
"""
import ctypes

import torch

from ._abi import _DTYPE_CODE, LsqGluW8Consts, LsqGluW8Shape, _assert_has_ops, glu_w8_library
from ._hip_host import _check, _on_device, _stream_of
from ._w8_host_common import _LEVEL_CODE, _check_out_q, _cpu_finish, _name, _on_one_device, _one, _status, _take_out

_FAMILIES = ("generic", "packets")
_ERR = "lsq_glu_w8_last_error"


def _rows(t):
    """(t or a dense copy of it, rows, row stride): t [.., C] as rows of C bytes one row stride apart"""
    C = int(t.shape[-1])
    rows = t.numel() // max(C, 1)
    lead = [(int(n), int(s)) for n, s in zip(t.shape[:-1], t.stride()[:-1]) if n != 1]
    if rows <= 1 or C == 0:
        ok, ld = (C <= 1 or t.stride(-1) == 1), C
    else:
        ld = lead[-1][1]
        ok = (C == 1 or t.stride(-1) == 1) and ld >= C and all(lead[i][1] == lead[i + 1][1] * lead[i + 1][0] for i in range(len(lead) - 1))
    if not ok:
        t, ld = t.contiguous(), C
    return t, rows, ld


def cpu_glu_value(gate_levels, up_levels, s_u, z_u, table, mid_dtype):
    """t of the definition, a `mid_dtype` tensor of gate's shape: the table gathered with the gate bytes, up's
    `LevelsTensor.dequantize(mid_dtype)` and torch's multiply"""
    a = table.to(mid_dtype)[gate_levels.contiguous().view(torch.uint8).long()]
    d = ((up_levels.to(torch.float32) - z_u.to(torch.float32).reshape(())) * s_u.reshape(())).to(mid_dtype)
    return a * d


def _glu(what, gate_levels, up_levels, s_u, z_u, table, out_q, mid_dtype, out):
    _assert_has_ops()
    for name, lv in (("gate_levels", gate_levels), ("up_levels", up_levels)):
        _check(lv.dtype in _LEVEL_CODE, "%s: %s must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, name, _name(lv.dtype)))
    _check(gate_levels.dim() >= 1 and tuple(gate_levels.shape) == tuple(up_levels.shape),
           "%s: gate and up must be level tensors of one shape [.., C], got %s and %s" % (what, tuple(gate_levels.shape), tuple(up_levels.shape)))
    _check(_one(s_u, torch.float32) and _one(z_u, torch.int32),
           "%s: up_scale must be one float32 value and up_zero one int32 value (tensors on the levels' device)" % what)
    _check(table.dtype == torch.float32 and table.dim() == 1 and table.numel() == 256 and table.is_contiguous(),
           "%s: the table must be a dense float32 tensor of 256 entries, got '%s' %s" % (what, _name(table.dtype), tuple(table.shape)))
    ydt, rng, qt = _check_out_q(what, out_q, mid_dtype)
    on_gpu = _on_one_device(what, (gate_levels, up_levels, s_u, z_u, table) + qt)
    shape = tuple(gate_levels.shape)
    if gate_levels.numel() == 0:
        return torch.empty(shape, dtype=ydt, device=gate_levels.device)
    lg, rows, gs = _rows(gate_levels)
    lu, _, us = _rows(up_levels)
    C = shape[-1]
    lib = glu_w8_library()
    sh = LsqGluW8Shape(rows, C, gs, us)
    plan = (ctypes.c_int32 * 8)()
    _status(lib.lsq_glu_w8_plan(ctypes.byref(sh), 1, ctypes.byref(plan)), what, lib, _ERR)
    if not on_gpu:
        t = cpu_glu_value(gate_levels, up_levels, s_u, z_u, table, mid_dtype)
        return _cpu_finish(t, out_q, rng, ydt).contiguous()
    y = _take_out(what, out, shape, ydt, lg.device)
    consts = LsqGluW8Consts(s_u.data_ptr(), z_u.data_ptr(), qt[0].data_ptr() if out_q else None, qt[1].data_ptr() if out_q else None,
                            rng[0], rng[1], rng[2], rng[3], _DTYPE_CODE[mid_dtype])
    idx = lg.device.index
    rc = _on_device(idx, lib.lsq_glu_w8, _LEVEL_CODE[lg.dtype], lg.data_ptr(), _LEVEL_CODE[lu.dtype], lu.data_ptr(), table.data_ptr(),
                    ctypes.byref(sh), ctypes.byref(consts), y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_glu_w8", lib, _ERR)
    return y


def glu_w8_q(gate_levels, up_levels, up_scale, up_zero, table, out_scale, out_shift, quant_min, quant_max, type_min, type_max, mid_dtype,
             out=None):
    """gate levels [.., C] and up levels [.., C] (each read in place through one row stride where it has one) -> the output
    quantizer's levels of table[gate byte] * up, a new dense uint8 or int8 tensor of that shape.  `out` (not an argument of the op,
    GPU only): a dense tensor like the result to write into, at any byte offset."""
    return _glu("lsq_glu_w8_q8_q", gate_levels, up_levels, up_scale, up_zero, table,
                (out_scale, out_shift, quant_min, quant_max, type_min, type_max), mid_dtype, out)


def glu_w8(gate_levels, up_levels, up_scale, up_zero, table, out_dtype, out=None):
    """the same -> the products as `out_dtype` floats."""
    return _glu("lsq_glu_w8_q8", gate_levels, up_levels, up_scale, up_zero, table, None, out_dtype, out)


def glu_w8_plan(rows, C, gate_row_stride=None, up_row_stride=None, aligned=True):
    """The launch liblsq_hip_glu_w8.so makes for gate and up of [rows, C] with these row strides in bytes (default: C, dense)
    whose buffers are (not) 16-byte aligned; host only, nothing is launched: family "packets" (C % 16 == 0, both row strides
    % 16 == 0, aligned) / "generic", grid, block, packets_per_lane, lds_bytes (packets: the table, 1024) and packets (rows * C / 16)."""
    lib = glu_w8_library()
    out = (ctypes.c_int32 * 8)()
    sh = LsqGluW8Shape(int(rows), int(C), int(C if gate_row_stride is None else gate_row_stride),
                       int(C if up_row_stride is None else up_row_stride))
    _status(lib.lsq_glu_w8_plan(ctypes.byref(sh), 1 if aligned else 0, ctypes.byref(out)), "lsq_glu_w8_plan", lib, _ERR)
    return dict(family=_FAMILIES[out[0]], grid=out[1], block=out[2], packets_per_lane=out[3], lds_bytes=out[4], packets=out[5])
