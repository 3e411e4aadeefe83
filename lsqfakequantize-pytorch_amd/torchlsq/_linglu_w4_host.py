"""Host layer of the gate and up linears of a gated MLP's DECODE STEP on packed 4- / 2-bit group-wise weights with the gated
product in their epilogue (include/lsq_hip_linglu_w4.h): the op `lsq_linear_packed_q8_glu_q` is, bit for bit,

    lsq_glu_w8_q8_q(lsq_linear_packed_q8_q(x, gate ...), lsq_linear_packed_q8_q(x, up ...), up_scale, up_zero, table, out ...)

-- nothing new is defined.  What differs is what a GPU call runs: when the flattened x has at most 16 rows, the format is one of
the matrix-core form and the levels and both code strips are 16-byte aligned, ONE ctypes call into liblsq_hip_linglu_w4.so (one
launch: 16 waves per workgroup streaming both strips, x staged once for both, the product formed in LDS); every other legal call
runs the ops above, one after the other (ONE linear where gate and up are the two row halves of one packed weight with one
quantizer).  The CPU path is that composition too.
"""
import ctypes

import torch

from ._abi import _DTYPE_CODE, LINGLU_W4_MAX_ROWS, LsqGluW8Consts, LsqLingluW4Proj, _assert_has_ops, linglu_w4_library
from ._glu_w8_host import glu_w8_q
from ._hip_host import _check, _on_device, _stream_of
from ._lindec_w4_host import fallback_decode, lindec_w4_linear_levels
from ._linglu_w8_host import _halves_of_one
from ._qlinear_a8_host import _LEVEL_CODE, _check_a8_args
from ._requant_w8_host import _STORES, _check_out, _out_struct
from ._w8_host_common import _check_out_q, _name, _one, _status, _take_out

_ERR = "lsq_linglu_w4_last_error"


def _served(M, C, K, group_size, bits, *operands):
    """what liblsq_hip_linglu_w4.so serves: its own plan's answer (host only, no launch)"""
    return M <= LINGLU_W4_MAX_ROWS and linglu_w4_plan(M, C, K, group_size, bits, all(t.data_ptr() % 16 == 0 for t in operands))["served"]


def _composed(x_levels, s_x, zx, g, u, fmt, g_rng, u_rng, up_scale, up_zero, table, out_q, mid_dtype, out=None):
    """the ops the new one composes, on either device: one linear on the fused packed weight where there is one, else two; the
    product (`out`, GPU only: where it is written)"""
    same_q = g_rng == u_rng and g[4].data_ptr() == u[4].data_ptr() and g[5].data_ptr() == u[5].data_ptr()
    fused = _halves_of_one(g, u) if same_q else None
    dec = fallback_decode(x_levels)
    if fused is not None:
        C = g[0].shape[0]
        gu = lindec_w4_linear_levels(x_levels, s_x, zx, *fused, *fmt, g[4], g[5], *g_rng, False, mid_dtype, dec, measured=True)
        gl, ul = gu[..., :C], gu[..., C:]
    else:
        gl = lindec_w4_linear_levels(x_levels, s_x, zx, *g[:4], *fmt, g[4], g[5], *g_rng, False, mid_dtype, dec, measured=True)
        ul = lindec_w4_linear_levels(x_levels, s_x, zx, *u[:4], *fmt, u[4], u[5], *u_rng, False, mid_dtype, dec, measured=True)
    return glu_w8_q(gl, ul, up_scale, up_zero, table, *out_q, mid_dtype, out=out)


def linglu_w4_q(x_levels, s_x, zx,
                gate_codes, gate_scale, gate_zero_point, gate_bias, gate_out_scale, gate_out_shift, gate_quant_min, gate_quant_max,
                gate_type_min, gate_type_max,
                up_codes, up_wscale, up_zero_point, up_bias, up_out_scale, up_out_shift, up_quant_min, up_quant_max, up_type_min, up_type_max,
                group_size, bits, up_scale, up_zero, table, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max,
                mid_dtype, out=None):
    """x_levels [.., K] bytes on two packed strips [C, K * bits / 8] -> the levels [.., C] of table[gate byte] * up under the output
    quantizer.  `out` (not an argument of the op, GPU only): a dense [M, C] level tensor to write into, at any byte offset, on either
    route.  Inference only."""
    what = "lsq_linear_packed_q8_glu_q"
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    g = (gate_codes, gate_scale, gate_zero_point, gate_bias, gate_out_scale, gate_out_shift)
    u = (up_codes, up_wscale, up_zero_point, up_bias, up_out_scale, up_out_shift)
    fmt = (int(group_size), int(bits))
    g_rng = (int(gate_quant_min), int(gate_quant_max), int(gate_type_min), int(gate_type_max))
    u_rng = (int(up_quant_min), int(up_quant_max), int(up_type_min), int(up_type_max))
    out_q = (out_scale, out_shift, int(out_quant_min), int(out_quant_max), int(out_type_min), int(out_type_max))
    _check_out(what + " (gate projection)", gate_out_scale, gate_out_shift, *g_rng, mid_dtype)
    _check_out(what + " (up projection)", up_out_scale, up_out_shift, *u_rng, mid_dtype)
    C, K = _check_a8_args(what + " (gate projection)", x_levels, *g[:4], *fmt, mid_dtype)
    Cu, _ = _check_a8_args(what + " (up projection)", x_levels, *u[:4], *fmt, mid_dtype)
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
        lx, gc, uc = lx.contiguous(), gate_codes.contiguous(), up_codes.contiguous()
        if _served(M, C, K, *fmt, lx, gc, uc):
            tensors = [t for t in g + u + (s_x, zx, up_scale, up_zero, table, out_scale, out_shift) if t is not None]
            _check(all(t.is_cuda and t.device == lx.device for t in tensors), "%s: every tensor must be on x's device" % what)
            lib = linglu_w4_library()
            keep, projs = [], []
            for (_, qs, qz, b, osc, osh), cd, r in ((g, gc, g_rng), (u, uc, u_rng)):
                qs, qz, b = qs.contiguous(), qz.contiguous(), None if b is None else b.contiguous()
                oq = _out_struct(osc, osh, r, False, mid_dtype)
                keep += [qs, qz, b, oq]
                projs.append(LsqLingluW4Proj(cd.data_ptr(), qs.data_ptr(), qz.data_ptr(), None if b is None else b.data_ptr(),
                                             ctypes.pointer(oq), 0 if b is None else _DTYPE_CODE[b.dtype]))
            y = _take_out(what, out, (M, C), ydt, lx.device)
            consts = LsqGluW8Consts(up_scale.data_ptr(), up_zero.data_ptr(), out_scale.data_ptr(), out_shift.data_ptr(), *rng,
                                    _DTYPE_CODE[mid_dtype])
            idx = lx.device.index
            rc = _on_device(idx, lib.lsq_linglu_w4, _LEVEL_CODE[lx.dtype], lx.data_ptr(), M, s_x.data_ptr(), zx.data_ptr(),
                            ctypes.byref(projs[0]), ctypes.byref(projs[1]), C, K, *fmt, table.data_ptr(), ctypes.byref(consts), y.data_ptr(),
                            _stream_of(idx))
            _status(rc, "lsq_linglu_w4", lib, _ERR)
            return y.reshape(out_shape)
        if out is not None:             # the product of the composition lands where the one launch would have put it
            out = _take_out(what, out, (M, C), ydt, lx.device).view(out_shape)
        return _composed(x_levels, s_x, zx, g, u, fmt, g_rng, u_rng, up_scale, up_zero, table, out_q, mid_dtype, out)
    return _composed(x_levels, s_x, zx, g, u, fmt, g_rng, u_rng, up_scale, up_zero, table, out_q, mid_dtype)


def linglu_w4_plan(M, C, K, group_size, bits, aligned=True, y_aligned=True):
    """The launch liblsq_hip_linglu_w4.so makes for (M, C, K, G, bits), host only: `served` (False: the call runs the ops it
    composes, every other field is 0), grid, block, lds_bytes, chunks (of at most 4096 k, whole spans), x_resident (one chunk holds
    all of K: x and the group sums stay in LDS across a workgroup's tiles) and store ("packets": C % 16 == 0 and a 16-byte aligned
    y, or "bytes")."""
    lib = linglu_w4_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_linglu_w4_plan(int(M), int(C), int(K), int(group_size), int(bits), 1 if aligned else 0, 1 if y_aligned else 0,
                                ctypes.byref(out))
    _status(rc, "lsq_linglu_w4_plan", lib, _ERR)
    return dict(served=bool(out[0]), grid=out[1], block=out[2], lds_bytes=out[3], chunks=out[4], x_resident=bool(out[5]), store=_STORES[out[6]])
