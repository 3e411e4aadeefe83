"""Host layer of the gate and up linears of a gated MLP's DECODE STEP with the gated product in their epilogue
(include/lsq_hip_linglu_w8.h): the op `lsq_linear_w8_q8_dec_glu_q` is, bit for bit,

    lsq_glu_w8_q8_q(lsq_linear_w8_q8_dec_q(x, gate ...), lsq_linear_w8_q8_dec_q(x, up ...), up_scale, up_zero, table, out ...)

-- nothing new is defined.  What differs is what a GPU call runs: when the flattened x has at most 16 rows, K % 16 == 0, K <= 65536
and the levels and both weights are 16-byte aligned, ONE ctypes call into liblsq_hip_linglu_w8.so (one launch: 16 waves per
workgroup streaming both weight strips, the product formed in LDS); every other legal call runs the ops above, one after the other
(ONE linear where gate and up are the two halves of one weight with one quantizer).  The CPU path is that composition too.
"""
import ctypes

import torch

from ._abi import _DTYPE_CODE, LINGLU_W8_MAX_ROWS, LsqGluW8Consts, LsqLingluW8Proj, _assert_has_ops, linglu_w8_library
from ._glu_w8_host import glu_w8_q
from ._hip_host import _check, _on_device, _stream_of
from ._lindec_w8_host import lindec_w8_linear_levels
from ._qlinear_w8_host import _LEVEL_CODE, _check_w8_args
from ._requant_w8_host import _STORES, _check_out, _out_struct
from ._w8_host_common import _check_out_q, _name, _one, _status, _take_out

_ERR = "lsq_linglu_w8_last_error"
_MAX_K = 65536


def _served(M, K, *operands):
    """what liblsq_hip_linglu_w8.so serves: the preconditions of its one kernel"""
    return 1 <= M <= LINGLU_W8_MAX_ROWS and 0 < K <= _MAX_K and K % 16 == 0 and all(t.data_ptr() % 16 == 0 for t in operands)


def _halves_of_one(g, u):
    """the tensors of the fused [2 C, K] linear of which `g` and `u` are the two halves -- every pair (levels, per-row constants,
    bias) two dense views of one storage, one behind the other -- or None"""
    parts = []
    for a, b in zip(g[:4], u[:4]):
        if a is None and b is None:
            parts.append(None)
            continue
        if a is None or b is None or not (a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype
                                          and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
                                          and b.storage_offset() == a.storage_offset() + a.numel()):
            return None
        parts.append(a.as_strided((2 * a.shape[0],) + tuple(a.shape[1:]), a.stride()))
    return parts


def _composed(x_levels, s_x, zx, g, u, g_rng, u_rng, up_scale, up_zero, table, out_q, mid_dtype, out=None):
    """the ops the new one composes, on either device: one linear on the fused weight where there is one, else two; the product
    (`out`, GPU only: where it is written)"""
    same_q = g_rng == u_rng and g[4].data_ptr() == u[4].data_ptr() and g[5].data_ptr() == u[5].data_ptr()
    fused = _halves_of_one(g, u) if same_q else None
    if fused is not None:
        C = g[0].shape[0]
        gu = lindec_w8_linear_levels(x_levels, s_x, zx, *fused, g[4], g[5], *g_rng, False, mid_dtype)
        gl, ul = gu[..., :C], gu[..., C:]
    else:
        gl = lindec_w8_linear_levels(x_levels, s_x, zx, *g[:4], g[4], g[5], *g_rng, False, mid_dtype)
        ul = lindec_w8_linear_levels(x_levels, s_x, zx, *u[:4], u[4], u[5], *u_rng, False, mid_dtype)
    return glu_w8_q(gl, ul, up_scale, up_zero, table, *out_q, mid_dtype, out=out)


def linglu_w8_q(x_levels, s_x, zx,
                gate_w_levels, gate_w_scale, gate_w_zero, gate_bias, gate_out_scale, gate_out_shift, gate_quant_min, gate_quant_max,
                gate_type_min, gate_type_max,
                up_w_levels, up_w_scale, up_w_zero, up_bias, up_out_scale, up_out_shift, up_quant_min, up_quant_max, up_type_min, up_type_max,
                up_scale, up_zero, table, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, mid_dtype, out=None):
    """x_levels [.., K] bytes -> the levels [.., C] of table[gate byte] * up under the output quantizer.  `out` (not an argument of
    the op, GPU only): a dense [M, C] level tensor to write into, at any byte offset, on either route.  Inference only."""
    what = "lsq_linear_w8_q8_dec_glu_q"
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    g = (gate_w_levels, gate_w_scale, gate_w_zero, gate_bias, gate_out_scale, gate_out_shift)
    u = (up_w_levels, up_w_scale, up_w_zero, up_bias, up_out_scale, up_out_shift)
    g_rng = (int(gate_quant_min), int(gate_quant_max), int(gate_type_min), int(gate_type_max))
    u_rng = (int(up_quant_min), int(up_quant_max), int(up_type_min), int(up_type_max))
    out_q = (out_scale, out_shift, int(out_quant_min), int(out_quant_max), int(out_type_min), int(out_type_max))
    _check_out(what + " (gate projection)", gate_out_scale, gate_out_shift, *g_rng, mid_dtype)
    _check_out(what + " (up projection)", up_out_scale, up_out_shift, *u_rng, mid_dtype)
    C, K = _check_w8_args(what + " (gate projection)", x_levels, *g[:4], mid_dtype)
    Cu, _ = _check_w8_args(what + " (up projection)", x_levels, *u[:4], mid_dtype)
    _check(C == Cu, "%s: the gate weight has %d rows and the up weight %d: one [C, K] shape is needed" % (what, C, Cu))
    _check(_one(s_x, torch.float32) and _one(zx, torch.int32),
           "%s: s_x must be one float32 value and zx one int32 value (tensors on x's device)" % what)
    _check(_one(up_scale, torch.float32) and _one(up_zero, torch.int32),
           "%s: up_scale must be one float32 value and up_zero one int32 value (tensors on x's device)" % what)
    _check(table.dtype == torch.float32 and table.dim() == 1 and table.numel() == 256 and table.is_contiguous(),
           "%s: the table must be a dense float32 tensor of 256 entries, got '%s' %s" % (what, _name(table.dtype), tuple(table.shape)))
    ydt, rng, _ = _check_out_q(what, out_q, mid_dtype)
    lx = x_levels.reshape(-1, K)
    M = lx.size(0)
    out_shape = x_levels.shape[:-1] + (C,)
    if x_levels.is_cuda and M > 0 and C > 0:
        lx, gw, uw = lx.contiguous(), gate_w_levels.contiguous(), up_w_levels.contiguous()
        if _served(M, K, lx, gw, uw):
            tensors = [t for t in g + u + (s_x, zx, up_scale, up_zero, table, out_scale, out_shift) if t is not None]
            _check(all(t.is_cuda and t.device == lx.device for t in tensors), "%s: every tensor must be on x's device" % what)
            lib = linglu_w8_library()
            keep, projs = [], []
            for (w, ws, wz, b, osc, osh), wl, r in ((g, gw, g_rng), (u, uw, u_rng)):
                ws, wz, b = ws.contiguous(), wz.contiguous(), None if b is None else b.contiguous()
                oq = _out_struct(osc, osh, r, False, mid_dtype)
                keep += [ws, wz, b, oq]
                projs.append(LsqLingluW8Proj(wl.data_ptr(), ws.data_ptr(), wz.data_ptr(), None if b is None else b.data_ptr(),
                                             ctypes.pointer(oq), _LEVEL_CODE[wl.dtype], 0 if b is None else _DTYPE_CODE[b.dtype]))
            y = _take_out(what, out, (M, C), ydt, lx.device)
            consts = LsqGluW8Consts(up_scale.data_ptr(), up_zero.data_ptr(), out_scale.data_ptr(), out_shift.data_ptr(), *rng,
                                    _DTYPE_CODE[mid_dtype])
            idx = lx.device.index
            rc = _on_device(idx, lib.lsq_linglu_w8, _LEVEL_CODE[lx.dtype], lx.data_ptr(), M, s_x.data_ptr(), zx.data_ptr(),
                            ctypes.byref(projs[0]), ctypes.byref(projs[1]), C, K, table.data_ptr(), ctypes.byref(consts), y.data_ptr(),
                            _stream_of(idx))
            _status(rc, "lsq_linglu_w8", lib, _ERR)
            return y.reshape(out_shape)
        if out is not None:             # the product of the composition lands where the one launch would have put it
            out = _take_out(what, out, (M, C), ydt, lx.device).view(out_shape)
        return _composed(x_levels, s_x, zx, g, u, g_rng, u_rng, up_scale, up_zero, table, out_q, mid_dtype, out)
    return _composed(x_levels, s_x, zx, g, u, g_rng, u_rng, up_scale, up_zero, table, out_q, mid_dtype)


def linglu_w8_plan(M, C, K, aligned=True, y_aligned=True):
    """The launch liblsq_hip_linglu_w8.so makes for (M, C, K), host only: `served` (False: the call runs the ops it composes, every
    other field is 0), grid, block, lds_bytes, chunks (of at most 4096 k), x_resident (one chunk holds all of K: x stays in LDS
    across a workgroup's tiles) and store ("packets": C % 16 == 0 and a 16-byte aligned y, or "bytes")."""
    lib = linglu_w8_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_linglu_w8_plan(int(M), int(C), int(K), 1 if aligned else 0, 1 if y_aligned else 0, ctypes.byref(out))
    _status(rc, "lsq_linglu_w8_plan", lib, _ERR)
    return dict(served=bool(out[0]), grid=out[1], block=out[2], lds_bytes=out[3], chunks=out[4], x_resident=bool(out[5]), store=_STORES[out[6]])
