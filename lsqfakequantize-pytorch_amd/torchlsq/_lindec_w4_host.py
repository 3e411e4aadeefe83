"""Host layer of the DECODE SHAPE of the W4A8 / W2A8 linears with an 8-bit output (include/lsq_hip_lindec_w4.h): the ops
`lsq_linear_packed_q8_q` and `lsq_linear_packed_q8_add_q` take activation levels and a packed 4- / 2-bit group-wise weight and
return the output quantizer's levels, with an optional residual given as levels.  Nothing new is defined: the result is the
composition of existing ops --

    y = lsq_linear_packed_q8(..., out_dtype=mid_dtype)                 the float-output op
    p = pre ? lsq(y; pre) : y                                          the layer's own output fake-quantizer, in mid_dtype
    t = p + ((float(l_r) - float(z_r)) * s_r).to(mid_dtype)            with a residual; torch's add in mid_dtype
    r = relu ? where(t < 0, 0, t) : t                                  a select
    levels = lsq_levels_per_tensor(r; out_scale, out_shift, range)

-- and on the GPU a call with `decode` that liblsq_hip_lindec_w4.so serves (at most 16 rows, a format of the matrix-core form, 16-byte
aligned codes and levels) is ONE ctypes call into it, with the same bytes: the kernel keeps the float-output kernel's order of the
fp32 sum.  With 17 to 64 rows it is ONE call into liblsq_hip_linmid_w4.so (_linmid_w4_host.py: the same order, the weight streamed
once), and up to `qgemm_a8_min_rows()` rows one launch per block of 64 rows into row slices of one output (`_row_blocks`); with
`measured` (`decode=None` of the functionals, the GLU and rotary fallbacks) a block takes that library only where it was measured
faster than liblsq_hip_lindec_w4.so called per 16 rows into the same slices, and those calls elsewhere.  Every
other GPU call (from that many rows on, the generic formats, misaligned codes, decode off) runs that composition from the existing
GPU ops; CPU tensors run it from `_cpu_levels_linear`, `_cpu_resadd` / `_cpu_requant`.  (The CPU path sums the groups in ascending
order, the GPU kernels in their waves' order: the two agree bit for bit when the fp32 steps are exact, and within the float-output
op's bound otherwise.)
"""
import contextlib
import ctypes
import threading

import torch

from ._abi import _DTYPE_CODE, LINDEC_W4_MAX_ROWS, LINMID_W4_MAX_ROWS, _assert_has_ops, lindec_w4_library
from ._cpu_host import _require_cpu
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._linmid_w4_host import _launch as _linmid_launch, _served as _linmid_served, linmid_w4_plan
from ._qgemm_a8_host import qgemm_a8_min_rows
from ._qlinear_a8_host import _LEVEL_CODE, _check_a8_args, _cpu_levels_linear
from ._requant_w8_host import _STORES, _check_out, _cpu_requant, _out_struct
from ._resadd_w8_host import _check_pre, _check_res, _cpu_resadd, _pre_ref, _res_struct
from ._w8_host_common import _name, _status, _take_out

_ERR = "lsq_lindec_w4_last_error"
_ROUTE = threading.local()      # .measured: set by `measured_routes` for the calls that reach this module through the torch ops


def _served(M, N, K, group_size, bits, *operands):
    """what liblsq_hip_lindec_w4.so serves: its own plan's answer (host only, no launch)"""
    return M <= LINDEC_W4_MAX_ROWS and lindec_w4_plan(M, N, K, group_size, bits, all(t.data_ptr() % 16 == 0 for t in operands))["served"]


def _composed(x_levels, s_x, zx, w, out_scale, out_shift, rng, relu, mid_dtype, res, pre, ldt):
    """the definition from the existing ops, on whichever device the tensors are"""
    ops = torch.ops.torchlsq
    y = ops.lsq_linear_packed_q8(x_levels, s_x, zx, *w, mid_dtype)
    if res is not None:
        pre_scale, pre_shift, pre_rng = pre
        if pre_scale is not None:
            y = ops.lsq(y, pre_scale, pre_shift, *pre_rng, 1, True, 1.0, True, False, True, False)
        y = y + ((res[0].to(torch.float32) - res[2].to(torch.float32)) * res[1]).to(mid_dtype)
    if relu:
        y = torch.where(y < 0, torch.zeros_like(y), y)
    lv = ops.lsq_levels_per_tensor(y, out_scale, out_shift, *rng, 0)
    return lv.view(torch.uint8) if ldt == torch.uint8 else lv


def _lindec(what, x_levels, s_x, zx, codes, qscale, qzero, bias, group_size, bits, out_scale, out_shift, rng, relu, mid_dtype, decode,
            res, pre, out, measured=False):
    """`res`: None or (res_levels, res_scale, res_zero); `pre`: (pre_scale, pre_shift, pre_rng), used with a residual only"""
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    ldt = _check_out(what, out_scale, out_shift, *rng, mid_dtype)
    N, K = _check_a8_args(what, x_levels, codes, qscale, qzero, bias, group_size, bits, mid_dtype)
    _check(s_x.dtype == torch.float32 and s_x.numel() == 1 and zx.dtype == torch.int32 and zx.numel() == 1,
           "%s: s_x must be one float32 value and zx one int32 value (tensors on x's device)" % what)
    out_shape = x_levels.shape[:-1] + (N,)
    tensors = (x_levels, s_x, zx, codes, qscale, qzero, out_scale, out_shift) + ((bias,) if bias is not None else ())
    pre_scale, pre_shift, pre_rng = pre
    if res is not None:
        _check_res(what, *res, out_shape)
        has_pre = _check_pre(what, pre_scale, pre_shift, pre_rng)
        tensors += tuple(res) + ((pre_scale, pre_shift) if has_pre else ())
    lx = x_levels.reshape(-1, K)
    M = lx.size(0)
    if not any(t.is_cuda for t in tensors):
        _require_cpu(what, *tensors)
        _check(out is None, "%s: `out` is served for GPU tensors only" % what)
        if M == 0 or N == 0:
            return torch.empty(out_shape, dtype=ldt)
        y = _cpu_levels_linear(lx, s_x, zx, codes, qscale, qzero, bias, group_size, bits, mid_dtype, N, K)
        if res is None:
            return _cpu_requant(y, out_scale, out_shift, rng, relu, ldt).reshape(out_shape)
        return _cpu_resadd(y, res[0].reshape(M, N), res[1], res[2], pre_scale, pre_shift, pre_rng, out_scale, out_shift, rng, relu,
                           ldt).reshape(out_shape)
    _require_gpu(what, *tensors)
    if M == 0 or N == 0:
        return torch.empty(out_shape, dtype=ldt, device=x_levels.device)
    lx, cd = lx.contiguous(), codes.contiguous()
    measured = measured or getattr(_ROUTE, "measured", False)
    blocks = _row_blocks(M, N, K, group_size, bits, lx, cd, measured) if decode else None
    if blocks is None:                                                  # every other legal call: the existing ops composed
        lv = _composed(x_levels, s_x, zx, (codes, qscale, qzero, bias, group_size, bits), out_scale, out_shift, rng, relu, mid_dtype,
                       res, pre, ldt)
        if out is None:
            return lv
        _take_out(what, out, (M, N), ldt, lx.device).copy_(lv.reshape(M, N))
        return out.reshape(out_shape)
    lib = lindec_w4_library()
    qs, qz = qscale.contiguous(), qzero.contiguous()
    bd = None if bias is None else bias.contiguous()
    y = _take_out(what, out, (M, N), ldt, lx.device)
    oq = _out_struct(out_scale, out_shift, rng, relu, mid_dtype)
    rl = None if res is None else res[0].reshape(M, N).contiguous()
    pre_struct, pre_arg = (None, None) if res is None else _pre_ref(pre_scale, pre_shift, pre_rng)
    idx = lx.device.index
    for m0, m1 in blocks:               # one launch per block of rows, into row slices of one output: no float intermediate
        rs = None if res is None else _res_struct(rl[m0:m1], res[1], res[2])
        res_arg = None if res is None else ctypes.byref(rs)
        if m1 - m0 > LINDEC_W4_MAX_ROWS:
            _linmid_launch(lx[m0:m1], s_x, zx, cd, qs, qz, bd, group_size, bits, ctypes.byref(oq), res_arg, pre_arg, y[m0:m1])
            continue
        rc = _on_device(idx, lib.lsq_lindec_w4_linear_levels, _LEVEL_CODE[lx.dtype], lx[m0:m1].data_ptr(), m1 - m0, s_x.data_ptr(),
                        zx.data_ptr(), cd.data_ptr(), N, K, group_size, bits, qs.data_ptr(), qz.data_ptr(),
                        None if bd is None else bd.data_ptr(), 0 if bd is None else _DTYPE_CODE[bd.dtype], ctypes.byref(oq), res_arg,
                        pre_arg, y[m0:m1].data_ptr(), _stream_of(idx))
        _status(rc, "lsq_lindec_w4_linear_levels", lib, _ERR)
    return y.reshape(out_shape)


def _row_blocks(M, N, K, group_size, bits, lx, cd, measured=False):
    """The (first row, end row) blocks a `decode` call is launched in, or None when it composes.  Up to 16 rows: one launch of
    liblsq_hip_lindec_w4.so.  Up to qgemm_a8_min_rows() rows: blocks of 64 rows, the last one by its size, each ONE launch of
    liblsq_hip_linmid_w4.so where that serves it -- and, with `measured`, where `_linmid_wins` -- else liblsq_hip_lindec_w4.so per 16
    rows.  Every launch writes a row slice of one output: no float intermediate on any of these routes.  From qgemm_a8_min_rows() rows
    on, and for what both libraries' plans refuse, the composition."""
    if M <= LINDEC_W4_MAX_ROWS:
        return [(0, M)] if _served(M, N, K, group_size, bits, lx, cd) else None
    if M >= qgemm_a8_min_rows():
        return None
    blocks = []                                 # (a block of rows of an aligned x is aligned: K is a multiple of 16)
    for m0 in range(0, M, LINMID_W4_MAX_ROWS):
        m1 = min(m0 + LINMID_W4_MAX_ROWS, M)
        if _linmid_served(m1 - m0, N, K, group_size, bits, lx, cd) and not (measured and not _linmid_wins(m1 - m0, N, K, group_size, bits)):
            blocks.append((m0, m1))
        else:
            blocks += [(r0, min(r0 + LINDEC_W4_MAX_ROWS, m1)) for r0 in range(m0, m1, LINDEC_W4_MAX_ROWS)]
    sizes = {m1 - m0 for m0, m1 in blocks if m1 - m0 <= LINDEC_W4_MAX_ROWS}
    return blocks if all(_served(n, N, K, group_size, bits, lx, cd) for n in sizes) else None


def _linmid_wins(M, N, K, group_size, bits):
    """Where ONE launch of liblsq_hip_linmid_w4.so on M rows (17 to 64, served) beat liblsq_hip_lindec_w4.so called per 16 rows in
    profiles/r41_linmid_w4_ab.txt: where a workgroup stages x ONCE.  With three or four sub-tiles of rows: K is one
    chunk and every workgroup has one tile (measured at 48 and 64 rows: 0.82 to 0.93 of the blocks' time).  With two: K is one chunk
    that stays in LDS across the tiles and the second block of 16 rows would be at most half full (measured at 17 rows: 0.88 to 0.99;
    at 32 rows the blocks win; 18 to 31 rows are NOT measured, the bound of 24 is the half-full block).  Everywhere else the
    blocks won: 1.01 to 1.73."""
    mid, dec = linmid_w4_plan(M, N, K, group_size, bits), lindec_w4_plan(LINDEC_W4_MAX_ROWS, N, K, group_size, bits)
    if dec["chunks"] != 1:
        return False
    if mid["subs"] >= 3:
        return -(-N // 16) <= mid["grid"]
    return mid["stages"] == 1 and M <= 24


@contextlib.contextmanager
def measured_routes():
    """Within the block, on this thread, a `decode` call beyond 16 rows takes per block of rows whichever library the A/B found faster
    (`_row_blocks(measured=True)`) rather than liblsq_hip_linmid_w4.so wherever it is served.  For callers that reach this module through
    the torch ops, whose one `decode` flag cannot say it: the functionals with `decode=None`."""
    before = getattr(_ROUTE, "measured", False)
    _ROUTE.measured = True
    try:
        yield
    finally:
        _ROUTE.measured = before


def fallback_decode(x_levels):
    """The `decode` an op that composes these linears as ITS fallback passes, with `measured=True` (_linglu_w4_host, _linrope_w4_host):
    up to 16 rows liblsq_hip_lindec_w4.so as ever, beyond that `functional.W4A8_MID_DEFAULT` -- nobody opted in there."""
    from . import functional
    return x_levels.numel() // max(1, x_levels.size(-1)) <= LINDEC_W4_MAX_ROWS or functional.W4A8_MID_DEFAULT


def lindec_w4_linear_levels(x_levels, s_x, zx, codes, qscale, qzero, bias, group_size, bits, out_scale, out_shift, quant_min, quant_max,
                            type_min, type_max, relu, mid_dtype, decode=True, out=None, measured=False):
    """x_levels [..., K] bytes on packed codes [N, K * bits / 8] -> the output quantizer's levels [..., N] (uint8 or int8).
    `decode`: False never takes liblsq_hip_lindec_w4.so or liblsq_hip_linmid_w4.so (the bytes are the same).  `out` (not an argument of the
    op): a dense [M, N] level tensor to write into, at any byte offset.  `measured` (nor this): beyond 16 rows the faster library per
    block of rows (`_row_blocks`), not liblsq_hip_linmid_w4.so wherever it is served.  Inference only."""
    rng = (int(quant_min), int(quant_max), int(type_min), int(type_max))
    return _lindec("lsq_linear_packed_q8_q", x_levels, s_x, zx, codes, qscale, qzero, bias, int(group_size), int(bits), out_scale,
                   out_shift, rng, relu, mid_dtype, decode, None, (None, None, (0, 255, 0, 255)), out, measured)


def lindec_w4_linear_levels_add(x_levels, s_x, zx, codes, qscale, qzero, bias, group_size, bits, out_scale, out_shift, quant_min,
                                quant_max, type_min, type_max, relu, mid_dtype, res_levels, res_scale, res_zero, pre_scale=None,
                                pre_shift=None, pre_quant_min=0, pre_quant_max=255, pre_type_min=0, pre_type_max=255, decode=True,
                                out=None, measured=False):
    """The same with residual levels [..., N] added before the ReLU, after the layer's own optional pre-quantizer.  Inference only."""
    rng = (int(quant_min), int(quant_max), int(type_min), int(type_max))
    pre_rng = (int(pre_quant_min), int(pre_quant_max), int(pre_type_min), int(pre_type_max))
    return _lindec("lsq_linear_packed_q8_add_q", x_levels, s_x, zx, codes, qscale, qzero, bias, int(group_size), int(bits), out_scale,
                   out_shift, rng, relu, mid_dtype, decode, (res_levels, res_scale, res_zero), (pre_scale, pre_shift, pre_rng), out, measured)


def lindec_w4_plan(M, N, K, group_size, bits, aligned=True, y_aligned=True, res_aligned=True):
    """The launch liblsq_hip_lindec_w4.so makes for (M, N, K, G, bits), host only: `served` (False: the host layer composes the
    existing ops, every other field is 0), grid, block, lds_bytes, chunks (of at most 4096 k, whole spans), x_resident (one chunk
    holds all of K: x stays in LDS across a workgroup's tiles), store and res_load ("packets": N % 16 == 0 and a 16-byte aligned y /
    residual, or "bytes")."""
    lib = lindec_w4_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_lindec_w4_plan(int(M), int(N), int(K), int(group_size), int(bits), 1 if aligned else 0, 1 if y_aligned else 0,
                                1 if res_aligned else 0, ctypes.byref(out))
    _status(rc, "lsq_lindec_w4_plan", lib, _ERR)
    return dict(served=bool(out[0]), grid=out[1], block=out[2], lds_bytes=out[3], chunks=out[4], x_resident=bool(out[5]),
                store=_STORES[out[6]], res_load=_STORES[out[7]])
