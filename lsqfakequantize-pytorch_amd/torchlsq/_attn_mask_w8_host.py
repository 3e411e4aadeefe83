"""Host layer of the MASKED softmax on 8-bit LEVELS (include/lsq_hip_attn_mask_w8.h states the contract): the integer-table softmax of
`_attn_w8_host.py` over a PREFIX of every row.  x is [.., Tq, Tk] levels; row r (t = r mod Tq inside its matrix) sees its first

    n_r = min(Tk,  t + 1 + causal_offset  where causal,  max(key_lengths[leading index of r], 0)  where lengths are given)

keys: m, E = table[m - b] and the exact integer S are taken over the prefix, p_i = float(E_i) * (1.0f / float(S)) for i < n_r and
p_i = +0.0f beyond it, then the output side as everywhere.  A row with n_r = 0 is all zeros and nothing is divided (ATen: NaN).
`key_lengths` is an int32 tensor [x.shape[0]] on x's device; it is read in the kernel, never on the host.

Two ops: `lsq_softmax_mask_w8_q8_q` (levels out) and `lsq_softmax_mask_w8_q8` (floats out).  x is read in place under
`_attn_w8_host.py`'s rules.  The CPU path IS the definition: vectorised int64 torch ops (a masked max, E masked to 0, S set to 1 only
where n_r = 0), torch float32 ops one at a time, `.to(mid_dtype)` and the existing `cpu_levels`.  Every op first calls the library's
plan function (host only: it runs without a GPU and enqueues nothing), which refuses an illegal shape with the library's message; the
GPU path is then ONE ctypes call that enqueues, nothing is read back, and it equals the CPU path bit for bit for the same table.
"""
import ctypes

import torch

from ._abi import LsqSoftmaxMaskW8Geom, _assert_has_ops, attn_mask_w8_library
from ._attn_w8_host import _FAMILIES_SOFTMAX, _out_struct, _softmax_rows
from ._cpu_host import _require_cpu
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._w8_host_common import _LEVEL_CODE, _check_out_q, _cpu_finish, _name, _status

_ERR = "lsq_attn_mask_w8_last_error"


def cpu_prefix_lengths(R, C, Tq, causal, causal_offset, key_lengths, rows_per_length):
    """n_r of the definition for the R rows, int64 [R] on the CPU"""
    n = torch.full((R,), C, dtype=torch.int64)
    if causal:
        n = torch.minimum(n, torch.arange(R, dtype=torch.int64) % Tq + 1 + int(causal_offset))
    if key_lengths is not None:
        n = torch.minimum(n, key_lengths.to(torch.int64).clamp_min(0).repeat_interleave(rows_per_length))
    return n


def cpu_softmax_mask_value(x_rows, table, n, mid_dtype):
    """u of the definition for x_rows [R, C] and the prefix lengths n [R], a `mid_dtype` tensor [R, C]"""
    b = x_rows.to(torch.int64)
    n = n.reshape(-1, 1)
    valid = torch.arange(b.shape[-1], dtype=torch.int64).reshape(1, -1) < n
    zero = torch.zeros((), dtype=torch.int64)
    m = torch.where(valid, b, torch.full((), -129, dtype=torch.int64)).amax(-1, keepdim=True)       # below every level
    E = torch.where(valid, table.to(torch.int64)[torch.where(valid, m - b, zero)], zero)
    S = E.sum(-1, keepdim=True)
    S = torch.where(n == 0, torch.ones((), dtype=torch.int64), S)      # only there: no division by zero, and E = 0 gives p = 0
    r = torch.ones((), dtype=torch.float32) / S.to(torch.float32)
    return (E.to(torch.float32) * r).to(mid_dtype)


def _mask_args(what, x, causal, causal_offset, key_lengths):
    """(causal 0 / 1, the offset, rows_per_length) after the checks the host can make"""
    causal, causal_offset = bool(causal), int(causal_offset)
    _check(x.dim() >= 2, "%s: the levels need at least 2 axes [.., Tq, Tk], got %s" % (what, tuple(x.shape)))
    _check(not causal or causal_offset >= 0, "%s: causal_offset = %d must be at least 0" % (what, causal_offset))
    rpl = 1
    if key_lengths is not None:
        _check(x.dim() >= 3, "%s: key_lengths needs levels of at least 3 axes [B, .., Tq, Tk], got %s" % (what, tuple(x.shape)))
        _check(key_lengths.dtype == torch.int32 and tuple(key_lengths.shape) == (int(x.shape[0]),) and key_lengths.is_contiguous(),
               "%s: key_lengths must be a dense int32 tensor of [%d], one entry per leading index of the levels, got '%s' %s"
               % (what, int(x.shape[0]), _name(key_lengths.dtype), tuple(key_lengths.shape)))
        _check(key_lengths.device == x.device, "%s: key_lengths must be on the levels' device (%s), got %s"
               % (what, x.device, key_lengths.device))
        rpl = x.numel() // max(int(x.shape[-1]), 1) // max(int(x.shape[0]), 1)
    return (1 if causal else 0), (causal_offset if causal else 0), rpl


def _softmax_mask(what, x, table, out_q, mid_dtype, causal, causal_offset, key_lengths, row_pad, out):
    _assert_has_ops()
    _check(x.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x.dtype)))
    _check(table.dtype == torch.int32 and tuple(table.shape) == (256,) and table.is_contiguous(),
           "%s: the table must be a dense int32 tensor of [256] (lsq_softmax_table), got '%s' %s" % (what, _name(table.dtype), tuple(table.shape)))
    causal, causal_offset, rpl = _mask_args(what, x, causal, causal_offset, key_lengths)
    row_pad = int(row_pad)
    _check(row_pad >= 1, "%s: row_pad = %d must be at least 1" % (what, row_pad))
    ydt, rng, qt = _check_out_q(what, out_q, mid_dtype)
    tensors = (x, table) + qt + (() if key_lengths is None else (key_lengths,)) + (() if out is None else (out,))
    on_gpu = any(t.is_cuda for t in tensors)
    Tq = int(x.shape[-2])
    lib = attn_mask_w8_library()
    y, yr, xr, R, C, ldx, ldy = _softmax_rows(what, x, ydt, row_pad, out, on_gpu)       # x, `row_pad` and `out` as the unmasked op takes them
    plan = (ctypes.c_int32 * 8)()
    geom = LsqSoftmaxMaskW8Geom(max(R, 1), C, ldx, ldy, _LEVEL_CODE[x.dtype], Tq if R else 1, rpl if R else 1, causal, causal_offset)
    _status(lib.lsq_softmax_mask_w8_plan(ctypes.byref(geom), 1, 1 if key_lengths is not None and R else 0, ctypes.byref(plan)),
            what, lib, _ERR)       # the shape's checks
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    if R == 0:
        return y
    if not on_gpu:
        n = cpu_prefix_lengths(R, C, Tq, causal, causal_offset, key_lengths, rpl)
        yr.copy_(_cpu_finish(cpu_softmax_mask_value(xr, table, n, mid_dtype), out_q, rng, ydt))
        return y
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_softmax_mask_w8, ctypes.byref(geom), ctypes.byref(_out_struct(out_q, rng, mid_dtype)), table.data_ptr(),
                    None if key_lengths is None else key_lengths.data_ptr(), xr.data_ptr(), yr.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_softmax_mask_w8", lib, _ERR)
    return y


def attn_mask_w8_softmax_q(x_levels, table, out_scale, out_shift, quant_min, quant_max, type_min, type_max, mid_dtype, causal=False,
                           causal_offset=0, key_lengths=None, row_pad=1, out=None):
    """softmax over the first n_r bytes of every row of x's levels [.., Tq, Tk] through the integer `table` -> the output quantizer's
    levels in x's shape, its level of 0 beyond n_r.  `causal`: row t of a matrix sees t + 1 + `causal_offset` keys; `key_lengths`:
    int32 [x.shape[0]] on x's device.  `row_pad` and `out` (not an argument of the op) as in `attn_w8_softmax_q`."""
    return _softmax_mask("lsq_softmax_mask_w8_q8_q", x_levels, table, (out_scale, out_shift, quant_min, quant_max, type_min, type_max),
                         mid_dtype, causal, causal_offset, key_lengths, row_pad, out)


def attn_mask_w8_softmax(x_levels, table, out_dtype, causal=False, causal_offset=0, key_lengths=None, out=None):
    """the same -> the probabilities as `out_dtype` floats in x's shape, +0.0 beyond n_r."""
    return _softmax_mask("lsq_softmax_mask_w8_q8", x_levels, table, None, out_dtype, causal, causal_offset, key_lengths, 1, out)


def attn_mask_w8_plan_softmax(R, C, Tq=1, ldx=None, ldy=None, aligned=True, x_dtype=torch.uint8, causal=False, causal_offset=0,
                              rows_per_length=None):
    """The launch liblsq_hip_attn_mask_w8.so makes for the masked softmax of R rows of C levels (matrices of Tq rows) with row strides
    ldx, ldy (C by default); `rows_per_length`: the rows that share one entry of key_lengths, None for a call without lengths.
    The keys and, for the same C, strides and alignment, the values of `attn_w8_plan_softmax`: family "packets" / "generic", grid,
    block, lanes_per_row (L), packets_per_lane (P), rows_per_workgroup and lds_bytes."""
    geom = LsqSoftmaxMaskW8Geom(int(R), int(C), int(C if ldx is None else ldx), int(C if ldy is None else ldy), _LEVEL_CODE[x_dtype],
                                int(Tq), int(rows_per_length or 1), int(causal), int(causal_offset))
    out = (ctypes.c_int32 * 8)()
    lib = attn_mask_w8_library()
    _status(lib.lsq_softmax_mask_w8_plan(ctypes.byref(geom), 1 if aligned else 0, 0 if rows_per_length is None else 1, ctypes.byref(out)),
            "lsq_softmax_mask_w8_plan", lib, _ERR)
    return dict(family=_FAMILIES_SOFTMAX[out[0]], grid=out[1], block=out[2], lanes_per_row=out[3], packets_per_lane=out[4],
                rows_per_workgroup=out[5], lds_bytes=out[6])
