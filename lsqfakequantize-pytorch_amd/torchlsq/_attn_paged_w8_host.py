"""Host layer of the PAGED KV cache on 8-bit LEVELS (include/lsq_hip_attn_paged_w8.h states the contract).  A pool is levels
[Np, Hkv, ps, D] -- Np pages of ps slots per kv head, any view with unit innermost stride, so both storage orders [Np, Hkv, ps, D] and
[Np, ps, Hkv, D] --, `block_table` is int32 [B, Mp] on the pools' device (rows `stride(0)` >= Mp apart), read in the kernels and
never on the host, and key j of batch entry b lies in page clamp(block_table[b, j // ps], 0, Np - 1) at slot j % ps:

    kv_gather_paged_w8(pool, block_table)[b, hkv, j, :] = pool[clamp(block_table[b, j // ps]), hkv, j % ps, :]        j < Mp ps

THE DECODE's definition is `_attn_decode_w8_host`'s on (q, gather(k_pool), gather(v_pool)); the CPU path is exactly that: the gather in
torch ops, then `_attn_decode_w8_host._compose`.  No new arithmetic, no tolerance.  On the GPU a call asks the library's plan (host
only).  Family "paged": ONE `torch.empty` of the reported workspace -- the caching allocator, so the call can be captured in a graph
-- and ONE ctypes call that enqueues the three kernels of the split-key decode reading the pools through the table; no page is
copied.  Everything else legal ("composition": ps not a power of two or below 16, G Tq > 16, D not a multiple of 16 or beyond 128, a
base or a stride that is not a multiple of 16) gathers and composes on the GPU, with the same bytes.  READS CLAMP.

THE APPEND writes a step's k and v [B, T, Hkv, D] (views of a qkv buffer are read in place) into the pools in one launch: token
(b, t) at p = positions[b] + t goes to page block_table[b, p // ps], slot p % ps (any ps).  WRITES SKIP: a token with p < 0,
p >= Mp ps or an entry outside [0, Np) is not written at all.  Two tokens of one call that name the same physical slot are the
caller's error.  The CPU path is plain index assignment.
"""
import ctypes

import torch

from . import _attn_decode_w8_host as _dec
from ._abi import (LsqAttnDecodeW8Consts, LsqAttnPagedW8Pages, LsqAttnW8Strides, LsqAttnDecodeW8Geom, LsqKvAppendPagedW8Geom, _assert_has_ops,
                   attn_paged_w8_library)
from ._attn_w8_host import _STORES, _out_struct
from ._cpu_host import _require_cpu
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._rope_w8_host import _span, _strides3
from ._w8_host_common import _LEVEL_CODE, _act_constants, _name, _status

_FAMILIES = ("composition", "paged")
_APPEND_FAMILIES = ("generic", "packets")
_APPEND_KERNELS = ("append_generic", "append_packets")
_ERR = "lsq_attn_paged_w8_last_error"


def _pool_strides(pool):
    """(page, head, slot) strides of a pool [Np, Hkv, ps, D] in elements; an axis of one element has no stride to speak of (a single
    slot: the row itself)"""
    st = [int(s) if int(n) > 1 else 0 for n, s in zip(pool.shape[:3], pool.stride()[:3])]
    if int(pool.shape[2]) == 1:
        st[2] = int(pool.shape[3])
    return tuple(st)


def _check_pool(what, name, pool):
    _check(pool.dtype in _LEVEL_CODE, "%s: the levels of %s must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, name, _name(pool.dtype)))
    _check(pool.dim() == 4 and pool.numel() > 0 and (pool.shape[3] == 1 or pool.stride(3) == 1),
           "%s: %s must be a non-empty [Np, Hkv, ps, D] tensor (or view) whose innermost stride is 1, got %s with strides %s"
           % (what, name, tuple(pool.shape), tuple(pool.stride())))


def _check_table(what, block_table, B, device):
    _check(block_table.dtype == torch.int32 and block_table.dim() == 2 and int(block_table.shape[0]) == B and block_table.shape[1] >= 1 and
           (block_table.shape[1] == 1 or block_table.stride(1) == 1) and (B == 1 or block_table.stride(0) >= block_table.shape[1]),
           "%s: block_table must be an int32 tensor of [%d, Mp] with unit innermost stride and rows at least Mp apart, got '%s' %s with "
           "strides %s" % (what, B, _name(block_table.dtype), tuple(block_table.shape), tuple(block_table.stride())))
    _check(block_table.device == device, "%s: block_table must be on the pools' device (%s), got %s" % (what, device, block_table.device))
    Mp = int(block_table.shape[1])
    return Mp, (int(block_table.stride(0)) if B > 1 else Mp)


def kv_gather_paged_w8(pool, block_table):
    """pool [Np, Hkv, ps, D] and block_table int32 [B, Mp] -> the dense cache [B, Hkv, Mp ps, D] the table names, entries clamped to
    0 .. Np - 1, dense: torch ops on the pool's device, nothing is read back.  The definition of the paged layout."""
    what = "lsq_kv_gather_paged_w8"
    _check_pool(what, "the pool", pool)
    _check(block_table.dim() == 2, "%s: block_table must be [B, Mp], got %s" % (what, tuple(block_table.shape)))
    B = int(block_table.shape[0])
    _check_table(what, block_table, B, pool.device)
    Np, Hkv, ps, D = (int(n) for n in pool.shape)
    idx = block_table.to(torch.int64).clamp(0, Np - 1)
    return pool[idx].permute(0, 2, 1, 3, 4).reshape(B, Hkv, int(block_table.shape[1]) * ps, D).contiguous()


def _plan_dict(out, ws_bytes):
    splits = out[5]
    return dict(family=_FAMILIES[out[0]], grid=out[1], reduce_grid=out[1] // splits if splits else 0, threads=out[2], rows=out[3],
                chunk=out[4], splits=splits, lds_bytes=out[6], store=_STORES[out[7]], workspace_bytes=int(ws_bytes))


def _splits_arg(what, splits):
    _check(isinstance(splits, int) and not isinstance(splits, bool) and splits >= 0,
           "%s: splits must be an int: 0 (the library's choice) or 1 .. ceil(Mp ps / 64), got %r" % (what, splits))
    return splits


def _plan_call(lib, geom, pages, qkv_aligned, y_aligned, splits, what):
    out, ws = (ctypes.c_int32 * 8)(), ctypes.c_int64(0)
    _status(lib.lsq_attn_paged_w8_plan(ctypes.byref(geom), ctypes.byref(pages), qkv_aligned, y_aligned, splits, ctypes.byref(out)), what, lib, _ERR)
    if out[0]:
        _status(lib.lsq_attn_paged_w8_workspace(ctypes.byref(geom), ctypes.byref(pages), splits, ctypes.byref(ws)), what, lib, _ERR)
    return _plan_dict(out, ws.value)


def attn_paged_w8_q(q_levels, q_scale, q_zero, k_pool, k_scale, k_zero, v_pool, v_scale, v_zero, block_table, table, scores_scale,
                    scores_shift, scores_quant_min, scores_quant_max, scores_type_min, scores_type_max, probs_scale, probs_shift,
                    probs_quant_min, probs_quant_max, probs_type_min, probs_type_max, out_scale, out_shift, out_quant_min, out_quant_max,
                    out_type_min, out_type_max, mid_dtype, causal=False, causal_offset=0, key_lengths=None, splits=0, out=None):
    """q [B, H, Tq, D] levels, the pools [Np, Hkv, ps, D] with their constants, `block_table` int32 [B, Mp], the softmax `table`, the
    three output quantizers, the mask and `splits` (as `attn_decode_split_w8_q`) -> the context's levels [B, Tq, H D]: those of
    `attn_decode_w8_q` on the gathered caches.  `out` (not an argument of the op) as there."""
    _assert_has_ops()
    what = "lsq_attention_decode_paged_w8_q8_q"
    splits = _splits_arg(what, splits)
    _check_pool(what, "k_pool", k_pool)
    _check_pool(what, "v_pool", v_pool)
    _check(tuple(k_pool.shape) == tuple(v_pool.shape), "%s: the pools must have one shape [Np, Hkv, ps, D], got %s and %s"
           % (what, tuple(k_pool.shape), tuple(v_pool.shape)))
    _check(q_levels.dim() == 4 and q_levels.shape[3] == k_pool.shape[3], "%s: q must be [B, H, Tq, D] with the pools' D = %d, got %s"
           % (what, int(k_pool.shape[3]), tuple(q_levels.shape)))
    B = int(q_levels.shape[0])
    Np, Hkv, ps, D = (int(n) for n in k_pool.shape)
    Mp, bt_ld = _check_table(what, block_table, B, k_pool.device)
    Tk = Mp * ps
    sides = ((scores_scale, scores_shift, scores_quant_min, scores_quant_max, scores_type_min, scores_type_max),
             (probs_scale, probs_shift, probs_quant_min, probs_quant_max, probs_type_min, probs_type_max),
             (out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max))
    # the operand checks of the decode op on stand-ins of ONE key per kv head (views of the pools: nothing is copied); the geometry
    # they give is then rewritten for the pools
    st = _dec._checked(what, q_levels, q_scale, q_zero, k_pool[:1, :, :1].expand(B, Hkv, 1, D), k_scale, k_zero,
                       v_pool[:1, :, :1].expand(B, Hkv, 1, D), v_scale, v_zero, table, *sides, mid_dtype, causal, causal_offset, key_lengths, out)
    if st.geom is None:
        return st.buf
    st.geom.Tk = Tk
    st.geom.k, st.geom.v = LsqAttnW8Strides(*_pool_strides(k_pool)), LsqAttnW8Strides(*_pool_strides(v_pool))
    pages = LsqAttnPagedW8Pages(Np, ps, Mp, bt_ld)
    lib = attn_paged_w8_library()
    plan = _plan_call(lib, st.geom, pages, _dec._aligned(st.q, k_pool, v_pool) if st.on_gpu else 1, _dec._aligned(st.yv) if st.on_gpu else 1,
                      splits, what)                                 # the shape's and the splits' checks, and the family
    if not st.on_gpu or plan["family"] != "paged":
        q_s, q_z, k_s, k_z, v_s, v_z = st.consts                    # the definition: the gather, then the existing ops composed
        _dec._compose(st.q, q_s, q_z, kv_gather_paged_w8(k_pool, block_table), k_s, k_z, kv_gather_paged_w8(v_pool, block_table), v_s, v_z,
                      st.table, st.s_side, st.p_side, st.o_side, st.mid_dtype, st.sdt, st.causal, st.causal_offset, st.key_lengths, st.yv)
        return st.buf
    ws = torch.empty(plan["workspace_bytes"], dtype=torch.uint8, device=st.q.device)       # the allocator's blocks are 16-byte aligned
    p_s, p_z = _act_constants(st.p_side[0], st.p_side[1], st.p_rng[2], st.p_rng[3])
    consts = LsqAttnDecodeW8Consts(q_scale.data_ptr(), q_zero.data_ptr(), k_scale.data_ptr(), k_zero.data_ptr(), v_scale.data_ptr(),
                                   v_zero.data_ptr(), p_s.data_ptr(), p_z.data_ptr())
    idx = st.q.device.index
    rc = _on_device(idx, lib.lsq_attn_paged_w8_decode, ctypes.byref(st.geom), ctypes.byref(pages), ctypes.byref(consts),
                    ctypes.byref(_out_struct(st.s_side, st.s_rng, st.mid_dtype)), ctypes.byref(_out_struct(st.p_side, st.p_rng, st.mid_dtype)),
                    ctypes.byref(_out_struct(st.o_side, st.o_rng, st.mid_dtype)), st.table.data_ptr(),
                    None if st.key_lengths is None else st.key_lengths.data_ptr(), block_table.data_ptr(), st.q.data_ptr(),
                    k_pool.data_ptr(), v_pool.data_ptr(), st.yv.data_ptr(), ws.data_ptr(), ws.numel(), splits, _stream_of(idx))
    _status(rc, "lsq_attn_paged_w8_decode", lib, _ERR)
    return st.buf


def attn_paged_w8_plan(B, H, Hkv, Tq, D, num_pages, page_size, max_pages, splits=0, bt_ld=None, q_strides=None, k_strides=None,
                       v_strides=None, y_strides=None, qkv_aligned=True, y_aligned=True, q_dtype=torch.uint8, k_dtype=torch.uint8,
                       v_dtype=torch.uint8, causal=False, causal_offset=0, has_lengths=True):
    """What liblsq_hip_attn_paged_w8.so does with q [B, H, Tq, D], pools [num_pages, Hkv, page_size, D] and a block table
    [B, max_pages] (rows `bt_ld` apart, max_pages by default); `k_strides`, `v_strides`: the pools' (page, head, slot) strides in
    elements, [Np, Hkv, ps, D] dense by default; the rest as `attn_decode_split_w8_plan`.  Host only.  Returns family "paged" /
    "composition", grid (= B Hkv splits), reduce_grid (= B Hkv), threads (256), rows (R = G Tq), chunk (keys, a multiple of 64), splits
    (= ceil(max_pages page_size / chunk)), lds_bytes (3840 + 160 D), store and workspace_bytes (= B Hkv R max_pages page_size +
    8 B Hkv splits R D); for "composition" the rest is 0."""
    what = "lsq_attn_paged_w8_plan"
    B, H, Hkv, Tq, D, Np, ps, Mp = (int(n) for n in (B, H, Hkv, Tq, D, num_pages, page_size, max_pages))
    splits = _splits_arg(what, splits)
    qs = LsqAttnW8Strides(*(int(n) for n in (q_strides if q_strides is not None else (H * Tq * D, Tq * D, D))))
    ks, vs = (LsqAttnW8Strides(*(int(n) for n in (s if s is not None else (Hkv * ps * D, ps * D, D)))) for s in (k_strides, v_strides))
    ys = LsqAttnW8Strides(*(int(n) for n in (y_strides if y_strides is not None else (Tq * H * D, D, H * D))))
    geom = LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Mp * ps, D, _LEVEL_CODE[q_dtype], _LEVEL_CODE[k_dtype], _LEVEL_CODE[v_dtype], 1 if causal else 0,
                               int(causal_offset), 1 if has_lengths else 0, qs, ks, vs, ys)
    pages = LsqAttnPagedW8Pages(Np, ps, Mp, Mp if bt_ld is None else int(bt_ld))
    return _plan_call(attn_paged_w8_library(), geom, pages, 1 if qkv_aligned else 0, 1 if y_aligned else 0, splits, what)


# -------------------------------------------------------------------------------------------------
# the append
# -------------------------------------------------------------------------------------------------
def _append_plan_dict(out):
    return dict(family=_APPEND_FAMILIES[out[0]], grid=out[1], threads=out[2], units=out[3], kernel=_APPEND_KERNELS[out[7]])


def cpu_place_paged(pool, x, block_table, positions):
    """the placement of the definition by plain index assignment: x [B, T, Hkv, D] into pool [Np, Hkv, ps, D]"""
    B, T = int(x.shape[0]), int(x.shape[1])
    Np, ps, Mp = int(pool.shape[0]), int(pool.shape[2]), int(block_table.shape[1])
    t = torch.arange(T, dtype=torch.int64)
    for b in range(B):
        p = t + (0 if positions is None else int(positions[b]))
        ok = (p >= 0) & (p < Mp * ps)
        e = block_table[b].to(torch.int64)[(p // ps).clamp(0, Mp - 1)]
        ok &= (e >= 0) & (e < Np)
        pool[e[ok], :, (p % ps)[ok]] = x[b, ok]


def kv_append_paged_w8(k_levels, v_levels, k_pool, v_pool, block_table, positions=None):
    """k and v [B, T, Hkv, D] levels into the pools [Np, Hkv, ps, D] (the same dtypes) through `block_table` int32 [B, Mp] at the
    positions `positions[b] + t` (int32 [B] on the device; None: zeros).  Returns nothing: the pools are written."""
    what = "lsq_kv_append_paged_w8"
    _assert_has_ops()
    _check_pool(what, "k_pool", k_pool)
    _check_pool(what, "v_pool", v_pool)
    _check(tuple(k_pool.shape) == tuple(v_pool.shape), "%s: the pools must have one shape [Np, Hkv, ps, D], got %s and %s"
           % (what, tuple(k_pool.shape), tuple(v_pool.shape)))
    Np, Hkv, ps, D = (int(n) for n in k_pool.shape)
    k, v = k_levels, v_levels
    _check(k.dim() == 4 and tuple(k.shape) == tuple(v.shape) and (int(k.shape[2]), int(k.shape[3])) == (Hkv, D),
           "%s: k and v must be [B, T, %d, %d], got %s and %s" % (what, Hkv, D, tuple(k.shape), tuple(v.shape)))
    _check(k.dtype == k_pool.dtype and v.dtype == v_pool.dtype, "%s: k and v must have their pools' level dtypes ('%s', '%s'), got '%s' and '%s'"
           % (what, _name(k_pool.dtype), _name(v_pool.dtype), _name(k.dtype), _name(v.dtype)))
    B, T = int(k.shape[0]), int(k.shape[1])
    Mp, bt_ld = _check_table(what, block_table, B, k_pool.device)
    if positions is not None:
        _check(positions.dtype == torch.int32 and tuple(positions.shape) == (B,) and positions.is_contiguous(),
               "%s: positions must be a dense int32 tensor of [%d], one entry per batch, got '%s' %s"
               % (what, B, _name(positions.dtype), tuple(positions.shape)))
    k, v = (x if D == 1 or x.stride(-1) == 1 else x.contiguous() for x in (k, v))
    tensors = (k, v, k_pool, v_pool, block_table) + (() if positions is None else (positions,))
    on_gpu = any(t.is_cuda for t in tensors)
    for name, pool in (("k_pool", k_pool), ("v_pool", v_pool)):     # what the library refuses on the GPU holds on both devices
        lo, hi = _span(pool)
        for other, t in (("k", k), ("v", v), ("block_table", block_table), ("positions", positions)) + ((("k_pool", k_pool),) if pool is v_pool else ()):
            if t is not None and t.numel() and t.device == pool.device:
                a, b = _span(t)
                _check(not (lo < b and a < hi), "%s: %s overlaps %s" % (what, name, other))
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    if not k.numel():
        return
    lib = attn_paged_w8_library()
    geom = LsqKvAppendPagedW8Geom(B, T, Hkv, D, LsqAttnPagedW8Pages(Np, ps, Mp, bt_ld), *_strides3(k), *_strides3(v), *_pool_strides(k_pool),
                                  *_pool_strides(v_pool))
    plan = (ctypes.c_int32 * 8)()
    _status(lib.lsq_kv_append_paged_w8_plan(ctypes.byref(geom), 1, ctypes.byref(plan)), what, lib, _ERR)       # the shape's checks
    if not on_gpu:
        cpu_place_paged(k_pool, k, block_table, positions)
        cpu_place_paged(v_pool, v, block_table, positions)
        return
    idx = k.device.index
    rc = _on_device(idx, lib.lsq_kv_append_paged_w8, ctypes.byref(geom), block_table.data_ptr(),
                    None if positions is None else positions.data_ptr(), k.data_ptr(), v.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(),
                    _stream_of(idx))
    _status(rc, what, lib, _ERR)


def kv_append_paged_w8_plan(B, T, Hkv, D, num_pages, page_size, max_pages, bt_ld=None, k_strides=None, v_strides=None, k_pool_strides=None,
                            v_pool_strides=None, aligned=True):
    """The launch liblsq_hip_attn_paged_w8.so makes for the append of k, v [B, T, Hkv, D] into pools [num_pages, Hkv, page_size, D];
    `k_strides`, `v_strides`: the sources' three outer strides, `*_pool_strides`: (page, head, slot), all in elements and dense by
    default; `aligned`: the four bases are 16-byte aligned.  Returns family "packets" / "generic", grid, threads (256), units (work
    units per token and head of one of k and v: D / 16 packets or D bytes) and kernel ("append_packets" / "append_generic")."""
    B, T, Hkv, D, Np, ps, Mp = (int(n) for n in (B, T, Hkv, D, num_pages, page_size, max_pages))
    xs = [tuple(int(n) for n in s) if s is not None else (T * Hkv * D, Hkv * D, D) for s in (k_strides, v_strides)]
    pls = [tuple(int(n) for n in s) if s is not None else (Hkv * ps * D, ps * D, D) for s in (k_pool_strides, v_pool_strides)]
    geom = LsqKvAppendPagedW8Geom(B, T, Hkv, D, LsqAttnPagedW8Pages(Np, ps, Mp, Mp if bt_ld is None else int(bt_ld)), *xs[0], *xs[1],
                                  *pls[0], *pls[1])
    out = (ctypes.c_int32 * 8)()
    lib = attn_paged_w8_library()
    _status(lib.lsq_kv_append_paged_w8_plan(ctypes.byref(geom), 1 if aligned else 0, ctypes.byref(out)), "lsq_kv_append_paged_w8_plan", lib, _ERR)
    return _append_plan_dict(out)
