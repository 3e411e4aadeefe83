"""Host layer of the attention core on 8-bit LEVELS (include/lsq_hip_attn_w8.h states the contract): a strided batched matmul of
two per-tensor level tensors and a softmax whose exponential is a 256-entry integer table.

    bmm       I = sum_k (la - za) (lb - zb), exact;  v = (s_b * float(I)) * s_a, two rounded float32 multiplies
              u = round_to(mid_dtype, v);  y = level(u) of (out_scale, out_shift, range), one byte -- or u itself
    softmax   m = max b;  E_i = table[m - b_i];  S = sum E (an exact integer);  r = 1.0f / float(S);  p_i = float(E_i) * r
              u = round_to(mid_dtype, p);  y = level(u) -- or u itself

Four ops: `lsq_bmm_w8_q8_q` / `lsq_softmax_w8_q8_q` (levels out) and `lsq_bmm_w8_q8` / `lsq_softmax_w8_q8` (floats out).  The
operands are read IN PLACE where their innermost stride is 1 (a q, k or v view of a qkv buffer, probabilities with padded rows);
only a view without unit innermost stride, one whose rows overlap (a row stride below the row: an expanded or sliding-window view),
or one whose last padded packet lies outside its storage, is made dense first; the strides handed to the library are the tensor's own.

The CPU path IS the definition: one int64 `torch.matmul` / int64 table sums, torch float32 ops one at a time, `.to(mid_dtype)` and
the existing `cpu_levels`.  Every op first calls the library's plan function (host only, it runs without a GPU and enqueues
nothing), which refuses an illegal shape with the library's message.  The GPU path is then ONE ctypes call that enqueues; nothing
is read back, and it equals the CPU path bit for bit (the softmax: for the same table).
"""
import ctypes

import torch

from ._abi import (_DTYPE_CODE, LsqAttnW8Out, LsqAttnW8Strides, LsqBmmW8Consts, LsqBmmW8Geom, LsqSoftmaxW8Geom, _assert_has_ops,
                   attn_w8_library)
from ._cpu_host import _require_cpu
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._w8_host_common import _LEVEL_CODE, _check_out_q, _cpu_finish, _name, _one, _status

_FAMILIES_BMM = ("generic", "mfma")
_FAMILIES_SOFTMAX = ("generic", "packets")
_FORMS = ("nn", "nt")
_STORES = ("elements", "packets")
_ERR = "lsq_attn_w8_last_error"


def _out_struct(out_q, rng, mid_dtype):
    return LsqAttnW8Out(out_q[0].data_ptr() if out_q else None, out_q[1].data_ptr() if out_q else None, rng[0], rng[1], rng[2], rng[3],
                        _DTYPE_CODE[mid_dtype])


def _readable(t):
    """the whole 16-byte packets of every row lie inside t's storage (the packet kernels read them and mask the tail)"""
    cols = int(t.shape[-1])
    last = sum((int(n) - 1) * int(s) for n, s in zip(t.shape[:-1], t.stride()[:-1]))
    return (int(t.storage_offset()) + last + (cols + 15) // 16 * 16) * t.element_size() <= t.untyped_storage().nbytes()


def _rows_apart(t):
    """the rows of t [.., rows, cols] do not overlap: one row, or a row stride of at least the row"""
    return t.shape[-2] == 1 or t.stride(-2) >= t.shape[-1]


def _in_place(t, on_gpu):
    """t as the kernels read it: itself where its innermost stride is 1, its rows lie at least a row apart (not an expanded or a
    sliding-window view) and its padded packets are readable, else a dense copy"""
    if (t.shape[-1] != 1 and t.stride(-1) != 1) or not _rows_apart(t):
        return t.contiguous()
    if on_gpu and t.shape[-1] % 16 and t.dim() >= 2 and t.stride(-2) % 16 == 0 and not _readable(t):
        return t.contiguous()
    return t


def _strides4(t):
    """(s0, s1, ld) of a tensor of 2 to 4 axes as [B0, B1, rows, cols], the strides as they are; an axis of one element has no
    stride to speak of (a single row: ld = cols).  The callers have made sure of `_rows_apart`."""
    st = [int(s) if int(n) > 1 else 0 for n, s in zip(t.shape[:-1], t.stride()[:-1])]
    st = [0] * (3 - len(st)) + st
    if int(t.shape[-2]) == 1:
        st[2] = int(t.shape[-1])
    return LsqAttnW8Strides(st[0], st[1], st[2])


# -------------------------------------------------------------------------------------------------
# batched matmul
# -------------------------------------------------------------------------------------------------
def _bmm_geom(a, b, y_strides, transpose_b):
    lead = [1] * (4 - a.dim()) + [int(n) for n in a.shape[:-2]]
    N = int(b.shape[-2] if transpose_b else b.shape[-1])
    return LsqBmmW8Geom(lead[0], lead[1], int(a.shape[-2]), N, int(a.shape[-1]), 1 if transpose_b else 0, _LEVEL_CODE[a.dtype],
                        _LEVEL_CODE[b.dtype], _strides4(a), _strides4(b), y_strides)


def _dense_strides(lead, M, N):
    return LsqAttnW8Strides(lead[1] * M * N if lead[0] > 1 else 0, M * N if lead[1] > 1 else 0, N)


def cpu_bmm_value(a_levels, s_a, z_a, b_levels, s_b, z_b, transpose_b, mid_dtype):
    """u of the definition, a `mid_dtype` tensor [..., M, N]"""
    f32 = torch.float32
    da = a_levels.to(torch.int64) - z_a.reshape(()).to(torch.int64)
    db = b_levels.to(torch.int64) - z_b.reshape(()).to(torch.int64)
    I = torch.matmul(da, db.transpose(-1, -2) if transpose_b else db)
    v = (s_b.detach().reshape(()) * I.to(f32)) * s_a.detach().reshape(())
    return v.to(mid_dtype)


def _bmm(what, a, s_a, z_a, b, s_b, z_b, transpose_b, out_q, mid_dtype, out):
    _assert_has_ops()
    for name, t in (("a", a), ("b", b)):
        _check(t.dtype in _LEVEL_CODE, "%s: the levels of %s must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, name, _name(t.dtype)))
    _check(2 <= a.dim() <= 4 and a.dim() == b.dim(), "%s: a and b must have the same 2 to 4 axes, got %s and %s" % (what, tuple(a.shape), tuple(b.shape)))
    _check(tuple(a.shape[:-2]) == tuple(b.shape[:-2]), "%s: a and b must have the same batch axes (they are not broadcast), got %s and %s"
           % (what, tuple(a.shape), tuple(b.shape)))
    kb = int(b.shape[-1] if transpose_b else b.shape[-2])
    _check(int(a.shape[-1]) == kb, "%s: a is [.., M, K = %d] and b is %s with K = %d" % (what, int(a.shape[-1]), "[.., N, K]" if transpose_b else "[.., K, N]", kb))
    for name, s, z in (("a", s_a, z_a), ("b", s_b, z_b)):
        _check(_one(s, torch.float32) and _one(z, torch.int32),
               "%s: %s's scale must be one float32 value and its zero point one int32 value (tensors on the levels' device)" % (what, name))
    ydt, rng, qt = _check_out_q(what, out_q, mid_dtype)
    tensors = (a, b, s_a, z_a, s_b, z_b) + qt + (() if out is None else (out,))
    on_gpu = any(t.is_cuda for t in tensors)
    M, K = int(a.shape[-2]), int(a.shape[-1])
    N = int(b.shape[-2] if transpose_b else b.shape[-1])
    shape = tuple(a.shape[:-2]) + (M, N)
    lead = [1] * (4 - a.dim()) + [int(n) for n in a.shape[:-2]]
    if out is not None:
        _check(out.dtype == ydt and tuple(out.shape) == shape and (N == 1 or out.stride(-1) == 1) and _rows_apart(out),
               "%s: `out` must be a %s tensor of shape %s whose innermost stride is 1 and whose rows do not overlap"
               % (what, _name(ydt), shape))
    lib = attn_w8_library()
    empty = 0 in shape or K == 0
    if not empty:
        a, b = _in_place(a, on_gpu), _in_place(b, on_gpu)
        geom = _bmm_geom(a, b, _dense_strides(lead, M, N) if out is None else _strides4(out), transpose_b)
        plan = (ctypes.c_int32 * 8)()
        _status(lib.lsq_bmm_w8_plan(ctypes.byref(geom), 1, 1, 1 if out_q else 0, ctypes.byref(plan)), what, lib, _ERR)     # the shape's checks
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    if empty:
        _check(K > 0 or 0 in shape, "%s: K = 0 is not served" % what)
        return out if out is not None else torch.empty(shape, dtype=ydt, device=a.device)
    if not on_gpu:
        u = _cpu_finish(cpu_bmm_value(a, s_a, z_a, b, s_b, z_b, transpose_b, mid_dtype), out_q, rng, ydt)
        if out is not None:
            out.copy_(u)
            return out
        return u.contiguous()
    y = torch.empty(shape, dtype=ydt, device=a.device) if out is None else out
    consts = LsqBmmW8Consts(s_a.data_ptr(), z_a.data_ptr(), s_b.data_ptr(), z_b.data_ptr())
    idx = a.device.index
    rc = _on_device(idx, lib.lsq_bmm_w8, ctypes.byref(geom), ctypes.byref(consts), ctypes.byref(_out_struct(out_q, rng, mid_dtype)),
                    a.data_ptr(), b.data_ptr(), y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_bmm_w8", lib, _ERR)
    return y


def attn_w8_bmm_q(a_levels, a_scale, a_zero, b_levels, b_scale, b_zero, transpose_b, out_scale, out_shift, quant_min, quant_max, type_min,
                  type_max, mid_dtype, out=None):
    """a [.., M, K] times b [.., K, N] (or [.., N, K] with `transpose_b`) per batch -> the output quantizer's levels [.., M, N] (uint8
    or int8, dense).  `out` (not an argument of the op): a tensor of that shape to write into, any row and batch strides."""
    return _bmm("lsq_bmm_w8_q8_q", a_levels, a_scale, a_zero, b_levels, b_scale, b_zero, bool(transpose_b),
                (out_scale, out_shift, quant_min, quant_max, type_min, type_max), mid_dtype, out)


def attn_w8_bmm(a_levels, a_scale, a_zero, b_levels, b_scale, b_zero, transpose_b, out_dtype, out=None):
    """the same -> the products as `out_dtype` floats [.., M, N]."""
    return _bmm("lsq_bmm_w8_q8", a_levels, a_scale, a_zero, b_levels, b_scale, b_zero, bool(transpose_b), None, out_dtype, out)


# -------------------------------------------------------------------------------------------------
# softmax
# -------------------------------------------------------------------------------------------------
def _rows(t):
    """t [.., C] as [R, C] with one row stride: a view where the leading axes collapse, else None"""
    C = int(t.shape[-1])
    if C != 1 and t.stride(-1) != 1:
        return None
    try:
        r = t.view(-1, C)
    except RuntimeError:
        return None
    return r if (C == 1 or r.stride(1) == 1) and (r.shape[0] == 1 or r.stride(0) >= C) else None


def cpu_softmax_value(x_levels, table, mid_dtype):
    """u of the definition, a `mid_dtype` tensor of x's shape"""
    b = x_levels.to(torch.int64)
    E = table.to(torch.int64)[b.amax(-1, keepdim=True) - b]
    S = E.sum(-1, keepdim=True)
    r = torch.ones((), dtype=torch.float32) / S.to(torch.float32)
    return (E.to(torch.float32) * r).to(mid_dtype)


def _softmax_rows(what, x, ydt, row_pad, out, on_gpu):
    """What the softmax and the masked softmax (_attn_mask_w8_host.py) do with x, `row_pad` and `out` before they plan: (y, the result
    as the caller gets it -- `out`, or a new tensor whose rows are padded to a multiple of `row_pad` --; yr and xr, y and x as [R, C]
    rows one stride apart, x made dense where it does not collapse or its padded packets are not readable; R; C; ldx; ldy).  With
    R = 0 yr and xr are None and the strides those of one dense row."""
    C = int(x.shape[-1])
    R = x.numel() // max(C, 1)
    if out is not None:
        _check(out.dtype == ydt and tuple(out.shape) == tuple(x.shape) and _rows(out) is not None,
               "%s: `out` must be a %s tensor of shape %s whose innermost stride is 1 and whose rows lie one row stride apart"
               % (what, _name(ydt), tuple(x.shape)))
        y, yr = out, _rows(out)
    else:
        Cp = (C + row_pad - 1) // row_pad * row_pad
        full = torch.empty(tuple(x.shape[:-1]) + (Cp,), dtype=ydt, device=x.device)
        y = full[..., :C] if Cp != C else full
        yr = full.view(-1, Cp)[:, :C] if R else None
    if not R:
        return y, None, None, 0, C, C, C
    xr = _rows(x)
    if xr is None or (on_gpu and C % 16 and xr.stride(0) % 16 == 0 and not _readable(xr)):
        xr = x.contiguous().view(-1, C)
    return y, yr, xr, R, C, (max(int(xr.stride(0)), C) if R > 1 else C), (max(int(yr.stride(0)), C) if R > 1 else C)


def _softmax(what, x, table, out_q, mid_dtype, row_pad, out):
    _assert_has_ops()
    _check(x.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x.dtype)))
    _check(x.dim() >= 1, "%s: the levels need at least one axis" % what)
    _check(table.dtype == torch.int32 and tuple(table.shape) == (256,) and table.is_contiguous(),
           "%s: the table must be a dense int32 tensor of [256] (lsq_softmax_table), got '%s' %s" % (what, _name(table.dtype), tuple(table.shape)))
    row_pad = int(row_pad)
    _check(row_pad >= 1, "%s: row_pad = %d must be at least 1" % (what, row_pad))
    ydt, rng, qt = _check_out_q(what, out_q, mid_dtype)
    tensors = (x, table) + qt + (() if out is None else (out,))
    on_gpu = any(t.is_cuda for t in tensors)
    lib = attn_w8_library()
    y, yr, xr, R, C, ldx, ldy = _softmax_rows(what, x, ydt, row_pad, out, on_gpu)
    plan = (ctypes.c_int32 * 8)()
    geom = LsqSoftmaxW8Geom(max(R, 1), C, ldx, ldy, _LEVEL_CODE[x.dtype])
    _status(lib.lsq_softmax_w8_plan(ctypes.byref(geom), 1, ctypes.byref(plan)), what, lib, _ERR)       # the shape's checks
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    if R == 0:
        return y
    if not on_gpu:
        yr.copy_(_cpu_finish(cpu_softmax_value(xr, table, mid_dtype), out_q, rng, ydt))
        return y
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_softmax_w8, ctypes.byref(geom), ctypes.byref(_out_struct(out_q, rng, mid_dtype)), table.data_ptr(),
                    xr.data_ptr(), yr.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_softmax_w8", lib, _ERR)
    return y


def attn_w8_softmax_q(x_levels, table, out_scale, out_shift, quant_min, quant_max, type_min, type_max, mid_dtype, row_pad=1, out=None):
    """softmax over the last axis of x's levels through the integer `table` -> the output quantizer's levels in x's shape.  The
    result is dense, or the [.., :C] view of a tensor whose rows are padded to a multiple of `row_pad` bytes.  `out` (not an
    argument of the op): a tensor of x's shape to write into, rows one stride apart."""
    return _softmax("lsq_softmax_w8_q8_q", x_levels, table, (out_scale, out_shift, quant_min, quant_max, type_min, type_max), mid_dtype,
                    row_pad, out)


def attn_w8_softmax(x_levels, table, out_dtype, out=None):
    """the same -> the probabilities as `out_dtype` floats in x's shape."""
    return _softmax("lsq_softmax_w8_q8", x_levels, table, None, out_dtype, 1, out)


# -------------------------------------------------------------------------------------------------
# the plans: host only, nothing is launched
# -------------------------------------------------------------------------------------------------
def attn_w8_plan_bmm(B, M, N, K, transpose_b=False, a_strides=None, b_strides=None, y_strides=None, aligned=True, y_aligned=True,
                     levels_out=True, a_dtype=torch.uint8, b_dtype=torch.int8):
    """The launch liblsq_hip_attn_w8.so makes for a [B0, B1, M, K] by [B0, B1, N, K] (`transpose_b`) or [B0, B1, K, N] matmul; `B` is
    B0 * B1 or the pair.  `*_strides`: (s0, s1, ld) in elements, dense by default.  Returns family "mfma" / "generic", form "nt" /
    "nn", grid, block, tile_rows, tile_cols, lds_bytes and store ("packets" / "elements")."""
    B0, B1 = (1, int(B)) if isinstance(B, int) else (int(B[0]), int(B[1]))
    rows_b, cols_b = (N, K) if transpose_b else (K, N)

    def dense(rows, cols):
        return (B1 * rows * cols, rows * cols, cols)

    st = [LsqAttnW8Strides(*(int(v) for v in (s if s is not None else dense(r, c))))
          for s, r, c in ((a_strides, M, K), (b_strides, rows_b, cols_b), (y_strides, M, N))]
    geom = LsqBmmW8Geom(B0, B1, int(M), int(N), int(K), 1 if transpose_b else 0, _LEVEL_CODE[a_dtype], _LEVEL_CODE[b_dtype], *st)
    out = (ctypes.c_int32 * 8)()
    lib = attn_w8_library()
    _status(lib.lsq_bmm_w8_plan(ctypes.byref(geom), 1 if aligned else 0, 1 if y_aligned else 0, 1 if levels_out else 0, ctypes.byref(out)),
            "lsq_bmm_w8_plan", lib, _ERR)
    return dict(family=_FAMILIES_BMM[out[0]], form=_FORMS[out[1]], grid=out[2], block=out[3], tile_rows=out[4], tile_cols=out[5],
                lds_bytes=out[6], store=_STORES[out[7]])


def attn_w8_plan_softmax(R, C, ldx=None, ldy=None, aligned=True, x_dtype=torch.uint8):
    """The launch liblsq_hip_attn_w8.so makes for the softmax of R rows of C levels with row strides ldx, ldy (C by default): family
    "packets" / "generic", grid, block, lanes_per_row (L), packets_per_lane (P), rows_per_workgroup and lds_bytes."""
    geom = LsqSoftmaxW8Geom(int(R), int(C), int(C if ldx is None else ldx), int(C if ldy is None else ldy), _LEVEL_CODE[x_dtype])
    out = (ctypes.c_int32 * 8)()
    lib = attn_w8_library()
    _status(lib.lsq_softmax_w8_plan(ctypes.byref(geom), 1 if aligned else 0, ctypes.byref(out)), "lsq_softmax_w8_plan", lib, _ERR)
    return dict(family=_FAMILIES_SOFTMAX[out[0]], grid=out[1], block=out[2], lanes_per_row=out[3], packets_per_lane=out[4],
                rows_per_workgroup=out[5], lds_bytes=out[6])
