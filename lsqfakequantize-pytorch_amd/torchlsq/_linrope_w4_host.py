"""Host layer of the qkv linear of an attention block's DECODE STEP on packed 4- / 2-bit group-wise weights with the rotary
embedding and the KV-cache append in its epilogue (include/lsq_hip_linrope_w4.h): with qkv = lsq_linear_packed_q8_q(x, codes ...)
viewed as [B, T, H + 2 Hkv, D] (q, then k, then v), the op `lsq_linear_packed_q8_rope_q` is, bit for bit,

    rq = lsq_rope_w8_q8_q(q, cos, sin, rot ..., positions)                                   returned, [B, T, H, D]
    dense:  lsq_rope_w8_q8_q(k ..., out=the cache, scatter=True);  lsq_kv_copy_w8(v, the cache, positions, scatter=True)
    paged:  lsq_kv_append_paged_w8(lsq_rope_w8_q8_q(k ..., positions), v, k_pool, v_pool, block_table, positions)

-- nothing new is defined, and `positions` is not advanced.  What differs is what a GPU call runs: what liblsq_hip_linrope_w4.so's
own plan calls served (B T <= 16, a format of the matrix-core form, D % 32 == 0, R % 32 == 0, 16-byte aligned buffers and strides)
is ONE ctypes call into it (one launch); every other legal call runs the ops above, one after the other.  The CPU path is that
composition too.  One difference, where the composition is undefined: a paged k whose position lies beyond the tables is NOT
written by the one launch (the composition appends a row of its temporary that the rotation left as allocated).
"""
import ctypes

import torch

from ._abi import (_DTYPE_CODE, LINROPE_W4_MAX_ROWS, LsqAttnPagedW8Pages, LsqLingluW4Proj, LsqLinropeW8Geom, LsqRopeW8In, LsqRopeW8Out,
                   _assert_has_ops, linrope_w4_library)
from ._attn_paged_w8_host import kv_append_paged_w8
from ._hip_host import _check, _on_device, _stream_of
from ._lindec_w4_host import fallback_decode, lindec_w4_linear_levels
from ._linrope_w8_host import _strides
from ._qlinear_a8_host import _LEVEL_CODE, _check_a8_args
from ._requant_w8_host import _check_out, _out_struct
from ._rope_w8_host import rope_w8_kv_copy, rope_w8_q
from ._w8_host_common import _check_out_q, _check_x_constants, _name, _status

_ERR = "lsq_linrope_w4_last_error"


def _geom(B, T, H, Hkv, D, R, P, interleaved, qs, paged, Tmax, ks, vs, pages):
    pg = LsqAttnPagedW8Pages(*pages) if paged else LsqAttnPagedW8Pages(0, 0, 0, 0)
    return LsqLinropeW8Geom(B, T, H, Hkv, D, R, P, 1 if interleaved else 0, *qs, 1 if paged else 0, 0 if paged else Tmax, *ks, *vs, pg)


def _plan(geom, K, group_size, bits, aligned):
    out = (ctypes.c_int32 * 9)()
    lib = linrope_w4_library()
    _status(lib.lsq_linrope_w4_plan(ctypes.byref(geom), int(K), int(group_size), int(bits), 1 if aligned else 0, ctypes.byref(out)),
            "lsq_linrope_w4_plan", lib, _ERR)
    return dict(served=bool(out[0]), grid=out[1], block=out[2], lds_bytes=out[3], chunks=out[4], x_resident=bool(out[5]), rotate_items=out[6],
                pass_items=out[7], copy_items=out[8])


def _composed(x_levels, s_x, zx, w, fmt, qkv_q, s_q, z_q, cos, sin, rot_q, mid_dtype, H, Hkv, D, k_cache, v_cache, positions, block_table, out):
    """the ops the new one composes, on either device"""
    B, T = int(x_levels.shape[0]), int(x_levels.shape[1])
    qkv = lindec_w4_linear_levels(x_levels, s_x, zx, *w, *fmt, *qkv_q, False, mid_dtype, fallback_decode(x_levels), measured=True).view(B, T, H + 2 * Hkv, D)
    q, k, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
    rq = rope_w8_q(q, s_q, z_q, cos, sin, *rot_q, mid_dtype, positions, False, out=out)
    if block_table is None:
        rope_w8_q(k, s_q, z_q, cos, sin, *rot_q, mid_dtype, positions, False, out=k_cache.permute(0, 2, 1, 3), scatter=True)
        rope_w8_kv_copy(v, v_cache.permute(0, 2, 1, 3), positions, True)
    else:
        kv_append_paged_w8(rope_w8_q(k, s_q, z_q, cos, sin, *rot_q, mid_dtype, positions, False), v, k_cache, v_cache, block_table, positions)
    return rq


def linrope_w4_q(x_levels, s_x, zx, codes, scale, zero_point, bias, group_size, bits, out_scale, out_shift, out_quant_min, out_quant_max,
                 out_type_min, out_type_max, qkv_scale, qkv_zero, cos, sin, rot_scale, rot_shift, rot_quant_min, rot_quant_max, rot_type_min,
                 rot_type_max, mid_dtype, heads, kv_heads, k_cache, v_cache, positions=None, block_table=None, out=None):
    """x_levels [B, T, K] bytes on packed codes [(heads + 2 kv_heads) D, K * bits / 8] -> the rotated q levels [B, T, heads, D]; the
    rotated k and the v levels are written into `k_cache` and `v_cache` at `positions[b] + t`: dense [B, kv_heads, Tmax, D], or with
    `block_table` (int32 [B, Mp]) the pools [Np, kv_heads, ps, D] (any view with unit innermost stride).  `qkv_scale` / `qkv_zero`:
    the constants of the qkv levels, as `lsq_rope_w8_q8_q` takes them.  `out` (not an argument of the op): a [B, T, heads, D] view
    with unit innermost stride to write rq into, on either route.  Inference only."""
    what = "lsq_linear_packed_q8_rope_q"
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    _check(x_levels.dim() == 3, "%s: the levels must be [B, T, K], got %s" % (what, tuple(x_levels.shape)))
    H, Hkv = int(heads), int(kv_heads)
    w, fmt = (codes, scale, zero_point, bias), (int(group_size), int(bits))
    qkv_q = (out_scale, out_shift, int(out_quant_min), int(out_quant_max), int(out_type_min), int(out_type_max))
    rot_q = (rot_scale, rot_shift, int(rot_quant_min), int(rot_quant_max), int(rot_type_min), int(rot_type_max))
    vdt = _check_out(what + " (qkv projection)", *qkv_q, mid_dtype)
    kdt, rot_rng, _ = _check_out_q(what + " (rotation)", rot_q, mid_dtype)
    N, K = _check_a8_args(what, x_levels, *w, *fmt, mid_dtype)
    _check_x_constants(what + " (the qkv levels)", qkv_scale, qkv_zero)
    _check(H >= 1 and Hkv >= 1 and N % (H + 2 * Hkv) == 0, "%s: the weight's %d rows are not (heads + 2 kv_heads) = %d heads of one size"
           % (what, N, H + 2 * Hkv))
    B, T, D = int(x_levels.shape[0]), int(x_levels.shape[1]), N // (H + 2 * Hkv)
    _check(k_cache.dim() == 4 and tuple(k_cache.shape) == tuple(v_cache.shape) and (int(k_cache.shape[1]), int(k_cache.shape[3])) == (Hkv, D),
           "%s: k_cache and v_cache must have one shape [.., %d, .., %d], got %s and %s" % (what, Hkv, D, tuple(k_cache.shape), tuple(v_cache.shape)))
    _check(k_cache.dtype == kdt and v_cache.dtype == vdt, "%s: k_cache must hold the rotation's levels ('%s') and v_cache the projection's "
           "('%s'), got '%s' and '%s'" % (what, _name(kdt), _name(vdt), _name(k_cache.dtype), _name(v_cache.dtype)))
    _check(cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.dim() == 2 and tuple(cos.shape) == tuple(sin.shape) and
           cos.is_contiguous() and sin.is_contiguous(), "%s: cos and sin must be dense float32 tensors of one shape [P, R / 2]" % what)
    P, R = int(cos.shape[0]), 2 * int(cos.shape[1])
    paged = block_table is not None
    _check(paged or int(k_cache.shape[0]) == B, "%s: the dense caches must be [%d, %d, Tmax, %d], got %s" % (what, B, Hkv, D, tuple(k_cache.shape)))
    if x_levels.is_cuda and B * T > 0 and k_cache.numel() > 0:
        lx, cd = x_levels.reshape(-1, K).contiguous(), codes.contiguous()
        rq = torch.empty((B, T, H, D), dtype=kdt, device=lx.device) if out is None else out
        dests = ((rq, (0, 1, 2)), (k_cache, (0, 2, 1)), (v_cache, (0, 2, 1)))
        st = [_strides(t, axes) for t, axes in dests]
        shaped = (B * T <= LINROPE_W4_MAX_ROWS and 2 <= R <= D and R % 2 == 0
                  and tuple(rq.shape) == (B, T, H, D) and rq.dtype == kdt and all(D == 1 or t.stride(-1) == 1 for t, _ in dests)
                  and (not paged or (block_table.dtype == torch.int32 and block_table.dim() == 2 and int(block_table.shape[0]) == B
                                     and (block_table.shape[1] == 1 or block_table.stride(1) == 1)))
                  and (positions is None or (positions.dtype == torch.int32 and tuple(positions.shape) == (B,) and positions.is_contiguous())))
        if shaped:
            Mp = int(block_table.shape[1]) if paged else 0
            pages = (int(k_cache.shape[0]), int(k_cache.shape[2]), Mp, int(block_table.stride(0)) if B > 1 else Mp) if paged else None
            geom = _geom(B, T, H, Hkv, D, R, P, False, st[0], paged, int(k_cache.shape[2]), st[1], st[2], pages)
            aligned = all(t.data_ptr() % 16 == 0 for t in (lx, cd, cos, sin, rq, k_cache, v_cache))
            if _plan(geom, K, *fmt, aligned)["served"]:
                tensors = [t for t in w + (s_x, zx, out_scale, out_shift, qkv_scale, qkv_zero, cos, sin, rot_scale, rot_shift, k_cache, v_cache,
                                           positions, block_table, rq) if t is not None]
                _check(all(t.is_cuda and t.device == lx.device for t in tensors), "%s: every tensor must be on x's device" % what)
                lib = linrope_w4_library()
                qs, qz, b = scale.contiguous(), zero_point.contiguous(), None if bias is None else bias.contiguous()
                oq = _out_struct(out_scale, out_shift, qkv_q[2:], False, mid_dtype)
                proj = LsqLingluW4Proj(cd.data_ptr(), qs.data_ptr(), qz.data_ptr(), None if b is None else b.data_ptr(), ctypes.pointer(oq),
                                       0 if b is None else _DTYPE_CODE[b.dtype])
                side = LsqRopeW8In(qkv_scale.data_ptr(), qkv_zero.data_ptr())
                ro = LsqRopeW8Out(rot_scale.data_ptr(), rot_shift.data_ptr(), *rot_rng, _DTYPE_CODE[mid_dtype])
                idx = lx.device.index
                rc = _on_device(idx, lib.lsq_linrope_w4, _LEVEL_CODE[lx.dtype], lx.data_ptr(), s_x.data_ptr(), zx.data_ptr(), ctypes.byref(proj), N,
                                K, *fmt, ctypes.byref(geom), ctypes.byref(side), ctypes.byref(ro), cos.data_ptr(), sin.data_ptr(),
                                None if positions is None else positions.data_ptr(), block_table.data_ptr() if paged else None, rq.data_ptr(),
                                k_cache.data_ptr(), v_cache.data_ptr(), _stream_of(idx))
                _status(rc, "lsq_linrope_w4", lib, _ERR)
                return rq
    return _composed(x_levels, s_x, zx, w, fmt, qkv_q, qkv_scale, qkv_zero, cos, sin, rot_q, mid_dtype, H, Hkv, D, k_cache, v_cache, positions,
                     block_table, out)


def linrope_w4_plan(B, T, H, Hkv, D, K, group_size, bits, R=None, P=1, Tmax=1, pages=None, q_strides=None, k_strides=None, v_strides=None,
                    aligned=True, interleaved=False):
    """The launch liblsq_hip_linrope_w4.so makes, host only: x [B, T, K] on the packed codes of a [(H + 2 Hkv) D, K] weight of
    `group_size` and `bits`, the rotary dimension R (D by default), tables of P positions, dense caches of `Tmax` tokens or `pages` =
    (num_pages, page_size, max_pages); `*_strides`: rq's (batch, token, head) and the caches' (batch or page, token or slot, head)
    strides, dense by default; `aligned`: every buffer is 16-byte aligned.  Returns `served` (False: the call runs the ops it
    composes, every other field is 0), grid, block, lds_bytes (exact), chunks (of at most 4096 k, whole spans), x_resident and the
    item counts rotate_items, pass_items, copy_items."""
    B, T, H, Hkv, D = (int(n) for n in (B, T, H, Hkv, D))
    toks = int(pages[1]) if pages is not None else int(Tmax)
    qs = (T * H * D, H * D, D) if q_strides is None else tuple(int(v) for v in q_strides)
    ks, vs = ((Hkv * toks * D, D, toks * D) if s is None else tuple(int(v) for v in s) for s in (k_strides, v_strides))
    pg = None if pages is None else (int(pages[0]), int(pages[1]), int(pages[2]), int(pages[2]))
    geom = _geom(B, T, H, Hkv, D, int(D if R is None else R), int(P), interleaved, qs, pages is not None, int(Tmax), ks, vs, pg)
    return _plan(geom, K, group_size, bits, aligned)
