"""Host layer of CHUNKED PREFILL attention on 8-bit LEVELS (include/lsq_hip_attn_chunk_w8.h states the contract): the definition, the
operand checks (`_checked`) and the arithmetic are `_attn_decode_w8_host`'s, word for word -- q [B, H, Tq, D] against k, v
[B, Hkv, Tk, D] with H = G Hkv, or against the POOLS of a paged cache through a block table (`_attn_paged_w8_host`'s layout and checks),
every row bounded by its key count n(b, t), nothing at or beyond n takes part or is read -- for ANY number of query rows, with
`causal` an int MODE:

    0   n = min(Tk, max(key_lengths[b], 0) where given)
    1   n = min(Tk, t + 1 + causal_offset, max(key_lengths[b], 0) where given)
    2   n = max(0, L_b - (Tq - 1 - t)),  L_b = min(Tk, max(key_lengths[b], 0))          needs key_lengths; causal_offset must be 0

Mode 2 counts every row's keys back from the length AFTER a prompt chunk was appended, on the device: the last row sees L_b keys, the
row before it one fewer, a row whose count would be negative none.  No host read-back, so one captured graph serves every chunk.

The CPU path is the definition: the existing ops composed as in `_attn_decode_w8_host._compose`, but on the key counts n [B, Tq] as a
DEVICE tensor -- the scores' padded buffer is read as [B H Tq, 1, Tk] rows and `lsq_softmax_mask_w8_q8_q` takes one length per row,
which covers all three modes without a host read.  For modes 0 and 1 the bytes are `attn_decode_w8_q`'s.

On the GPU a call asks the library's plan (host only).  Family "chunk": ONE `torch.empty` of the reported workspace

    bytes = B Hkv R ldw + 8 B Hkv S R D,      R = G Tq,  ldw = 16 ceil(Tk / 16)  (paged: Mp ps)

-- LARGE in R: 512 tokens x G 4 x Tk 32768 are 64 MB of score bytes per kv head -- and ONE ctypes call that enqueues the three
launches of the split-key decode with the rows of a kv head dealt to row tiles of 16.  Everything else legal ("composition": D not a
multiple of 16 or beyond 128, ps not a power of two or below 16, a base or a stride that is not a multiple of 16) composes on the
GPU, after a gather for pools, with the same bytes.
"""
import ctypes

import torch

from . import _attn_decode_w8_host as _dec
from . import _attn_paged_w8_host as _pg
from ._abi import LsqAttnDecodeW8Consts, LsqAttnDecodeW8Geom, LsqAttnPagedW8Pages, LsqAttnW8Strides, _assert_has_ops, attn_chunk_w8_library
from ._attn_mask_w8_host import attn_mask_w8_softmax_q
from ._attn_w8_host import _STORES, _out_struct, attn_w8_bmm_q
from ._hip_host import _check, _on_device, _stream_of
from ._w8_host_common import _LEVEL_CODE, _act_constants, _status

_FAMILIES = ("composition", "chunk")
_ERR = "lsq_attn_chunk_w8_last_error"
CAUSAL_LENGTHS = 2      # LSQ_ATTN_CHUNK_W8_CAUSAL_LENGTHS


def _plan_dict(out, ws_bytes):
    return dict(family=_FAMILIES[out[0]], grid=out[1], reduce_grid=out[1] // out[6] if out[6] else 0, threads=out[2], rows=out[3],
                tiles=out[4], chunk=out[5], splits=out[6], lds_bytes=out[7], store=_STORES[out[8]], workspace_bytes=int(ws_bytes))


def _mode(what, causal, causal_offset, key_lengths):
    """the checks of the mask mode that the library makes too, said before any tensor is touched"""
    _check(isinstance(causal, int) and not isinstance(causal, bool) and causal in (0, 1, 2),
           "%s: causal must be the int 0 (off), 1 (t + 1 + causal_offset keys) or 2 (counted back from key_lengths), got %r" % (what, causal))
    _check(causal != CAUSAL_LENGTHS or key_lengths is not None,
           "%s: causal = 2 counts every row's keys back from key_lengths and needs them" % what)
    _check(causal != CAUSAL_LENGTHS or int(causal_offset) == 0, "%s: causal = 2 takes no offset, causal_offset = %d must be 0" % (what, int(causal_offset)))
    return causal


def key_counts(B, Tq, Tk, mode, causal_offset, key_lengths, device):
    """n(b, t) of the definition for the three modes, int64 [B, Tq] on `device`, from tensor ops alone"""
    if mode != CAUSAL_LENGTHS:
        return _dec.key_counts(B, Tq, Tk, mode == 1, causal_offset, key_lengths, device)
    L = key_lengths.to(torch.int64).clamp(0, Tk).reshape(B, 1)
    return (L - (Tq - 1 - torch.arange(Tq, dtype=torch.int64, device=device)).reshape(1, Tq)).clamp_min(0)


def _compose(q, q_s, q_z, k, k_s, k_z, v, v_s, v_z, table, s_side, p_side, o_side, mid_dtype, sdt, n, yv):
    """the definition on q's device for the key counts `n` (int64 [B, Tq] on that device, never read back): the decode host's
    composition with the softmax taken row by row -- the padded score buffer as [B H Tq, 1, Tk] and one length per row"""
    B, H, Tq, _ = (int(x) for x in q.shape)
    Tk, G = int(k.shape[-2]), H // int(k.shape[1])
    if G > 1:
        k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    Tkp = (Tk + 15) // 16 * 16
    scores = torch.empty((B, H, Tq, Tkp), dtype=sdt, device=q.device)
    attn_w8_bmm_q(q, q_s, q_z, k, k_s, k_z, True, *s_side, mid_dtype, out=scores[..., :Tk])
    lens = n.reshape(B, 1, Tq).expand(B, H, Tq).reshape(-1).to(torch.int32)
    p = attn_mask_w8_softmax_q(scores.view(B * H * Tq, 1, Tkp)[..., :Tk], table, *p_side, mid_dtype, False, 0, lens, 16)
    p = p.unflatten(0, (B, H, Tq)).squeeze(3)                              # [B, H, Tq, Tk] on the padded rows
    p_s, p_z = _act_constants(p_side[0], p_side[1], p_side[4], p_side[5])
    beyond = torch.arange(Tk, dtype=torch.int64, device=q.device).reshape(1, 1, 1, Tk) >= n.reshape(B, 1, Tq, 1)
    p.copy_(torch.where(beyond, p_z.to(torch.int64).to(p.dtype), p))       # a key at or beyond n: the byte z_p, which contributes 0
    attn_w8_bmm_q(p, p_s, p_z, v, v_s, v_z, False, *o_side, mid_dtype, out=yv)


def _sides(a):
    return tuple(a[0:6]), tuple(a[6:12]), tuple(a[12:18])


def _plan_call(lib, geom, pages, qkv_aligned, y_aligned, splits, what):
    out, ws = (ctypes.c_int32 * 9)(), ctypes.c_int64(0)
    if pages is None:
        _status(lib.lsq_attn_chunk_w8_plan(ctypes.byref(geom), qkv_aligned, y_aligned, splits, ctypes.byref(out)), what, lib, _ERR)
        if out[0]:
            _status(lib.lsq_attn_chunk_w8_workspace(ctypes.byref(geom), splits, ctypes.byref(ws)), what, lib, _ERR)
    else:
        _status(lib.lsq_attn_chunk_paged_w8_plan(ctypes.byref(geom), ctypes.byref(pages), qkv_aligned, y_aligned, splits, ctypes.byref(out)),
                what, lib, _ERR)
        if out[0]:
            _status(lib.lsq_attn_chunk_paged_w8_workspace(ctypes.byref(geom), ctypes.byref(pages), splits, ctypes.byref(ws)), what, lib, _ERR)
    return _plan_dict(out, ws.value)


def _run(what, st, mode, splits, pages, k, v, block_table):
    """a checked call: the library's three launches where its plan says "chunk" on the GPU, the composition elsewhere; `k`, `v`: the
    caches, or with `pages` the pools"""
    st.geom.causal = mode
    lib = attn_chunk_w8_library()
    plan = _plan_call(lib, st.geom, pages, _dec._aligned(st.q, k, v) if st.on_gpu else 1, _dec._aligned(st.yv) if st.on_gpu else 1, splits,
                      what)                                         # the shape's, the mode's and the splits' checks, and the family
    if not st.on_gpu or plan["family"] != "chunk":
        q_s, q_z, k_s, k_z, v_s, v_z = st.consts                    # the definition: (the gather, then) the existing ops composed
        if pages is not None:
            k, v = _pg.kv_gather_paged_w8(k, block_table), _pg.kv_gather_paged_w8(v, block_table)
        B, Tq, Tk = int(st.q.shape[0]), int(st.q.shape[2]), int(k.shape[2])
        n = key_counts(B, Tq, Tk, mode, st.causal_offset, st.key_lengths, st.q.device)
        _compose(st.q, q_s, q_z, k, k_s, k_z, v, v_s, v_z, st.table, st.s_side, st.p_side, st.o_side, st.mid_dtype, st.sdt, n, st.yv)
        return st.buf
    ws = torch.empty(plan["workspace_bytes"], dtype=torch.uint8, device=st.q.device)       # the allocator's blocks are 16-byte aligned
    p_s, p_z = _act_constants(st.p_side[0], st.p_side[1], st.p_rng[2], st.p_rng[3])
    q_scale, q_zero, k_scale, k_zero, v_scale, v_zero = st.consts
    consts = LsqAttnDecodeW8Consts(q_scale.data_ptr(), q_zero.data_ptr(), k_scale.data_ptr(), k_zero.data_ptr(), v_scale.data_ptr(),
                                   v_zero.data_ptr(), p_s.data_ptr(), p_z.data_ptr())
    sides = (ctypes.byref(_out_struct(st.s_side, st.s_rng, st.mid_dtype)), ctypes.byref(_out_struct(st.p_side, st.p_rng, st.mid_dtype)),
             ctypes.byref(_out_struct(st.o_side, st.o_rng, st.mid_dtype)))
    lens = None if st.key_lengths is None else st.key_lengths.data_ptr()
    tail = (st.q.data_ptr(), k.data_ptr(), v.data_ptr(), st.yv.data_ptr(), ws.data_ptr(), ws.numel(), splits)
    idx = st.q.device.index
    if pages is None:
        rc = _on_device(idx, lib.lsq_attn_chunk_w8, ctypes.byref(st.geom), ctypes.byref(consts), *sides, st.table.data_ptr(), lens, *tail,
                        _stream_of(idx))
        _status(rc, "lsq_attn_chunk_w8", lib, _ERR)
    else:
        rc = _on_device(idx, lib.lsq_attn_chunk_paged_w8, ctypes.byref(st.geom), ctypes.byref(pages), ctypes.byref(consts), *sides,
                        st.table.data_ptr(), lens, block_table.data_ptr(), *tail, _stream_of(idx))
        _status(rc, "lsq_attn_chunk_paged_w8", lib, _ERR)
    return st.buf


def attn_chunk_w8_q(q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table, scores_scale, scores_shift,
                    scores_quant_min, scores_quant_max, scores_type_min, scores_type_max, probs_scale, probs_shift, probs_quant_min,
                    probs_quant_max, probs_type_min, probs_type_max, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min,
                    out_type_max, mid_dtype, causal=0, causal_offset=0, key_lengths=None, splits=0, out=None):
    """The arguments and the result of `attn_decode_split_w8_q` for any number of query rows, `causal` being the int mode of this
    module: q [B, H, Tq, D], k and v [B, Hkv, Tk, D] levels (Hkv divides H) with their constants, the softmax `table`, the three output
    quantizers, the mask and `splits` -> the context's levels [B, Tq, H D], written through their [B, H, Tq, D] view; `out` (not an
    argument of the op) as there.  The same bytes for every `splits`.  The workspace of a served call is
    B Hkv R 16 ceil(Tk / 16) + 8 B Hkv splits R D bytes, R = (H / Hkv) Tq."""
    _assert_has_ops()
    what = "lsq_attention_chunk_w8_q8_q"
    splits = _dec_splits(what, splits)
    mode = _mode(what, causal, causal_offset, key_lengths)
    sides = _sides((scores_scale, scores_shift, scores_quant_min, scores_quant_max, scores_type_min, scores_type_max, probs_scale, probs_shift,
                    probs_quant_min, probs_quant_max, probs_type_min, probs_type_max, out_scale, out_shift, out_quant_min, out_quant_max,
                    out_type_min, out_type_max))
    st = _dec._checked(what, q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table, *sides, mid_dtype,
                       mode == 1, causal_offset, key_lengths, out)
    if st.geom is None:
        return st.buf
    return _run(what, st, mode, splits, None, st.k, st.v, None)


def attn_chunk_paged_w8_q(q_levels, q_scale, q_zero, k_pool, k_scale, k_zero, v_pool, v_scale, v_zero, block_table, table, scores_scale,
                          scores_shift, scores_quant_min, scores_quant_max, scores_type_min, scores_type_max, probs_scale, probs_shift,
                          probs_quant_min, probs_quant_max, probs_type_min, probs_type_max, out_scale, out_shift, out_quant_min, out_quant_max,
                          out_type_min, out_type_max, mid_dtype, causal=0, causal_offset=0, key_lengths=None, splits=0, out=None):
    """The same against the pools [Np, Hkv, ps, D] of a paged cache through `block_table` int32 [B, Mp] (the arguments of
    `attn_paged_w8_q`): `attn_chunk_w8_q`'s result on the gathered caches, without gathering them where the plan says "chunk".  The
    workspace of a served call is B Hkv R Mp ps + 8 B Hkv splits R D bytes."""
    _assert_has_ops()
    what = "lsq_attention_chunk_paged_w8_q8_q"
    splits = _dec_splits(what, splits)
    mode = _mode(what, causal, causal_offset, key_lengths)
    _pg._check_pool(what, "k_pool", k_pool)
    _pg._check_pool(what, "v_pool", v_pool)
    _check(tuple(k_pool.shape) == tuple(v_pool.shape), "%s: the pools must have one shape [Np, Hkv, ps, D], got %s and %s"
           % (what, tuple(k_pool.shape), tuple(v_pool.shape)))
    _check(q_levels.dim() == 4 and q_levels.shape[3] == k_pool.shape[3], "%s: q must be [B, H, Tq, D] with the pools' D = %d, got %s"
           % (what, int(k_pool.shape[3]), tuple(q_levels.shape)))
    B = int(q_levels.shape[0])
    Np, Hkv, ps, D = (int(n) for n in k_pool.shape)
    Mp, bt_ld = _pg._check_table(what, block_table, B, k_pool.device)
    sides = _sides((scores_scale, scores_shift, scores_quant_min, scores_quant_max, scores_type_min, scores_type_max, probs_scale, probs_shift,
                    probs_quant_min, probs_quant_max, probs_type_min, probs_type_max, out_scale, out_shift, out_quant_min, out_quant_max,
                    out_type_min, out_type_max))
    # the operand checks of the decode op on stand-ins of ONE key per kv head (views of the pools: nothing is copied); the geometry
    # they give is then rewritten for the pools
    st = _dec._checked(what, q_levels, q_scale, q_zero, k_pool[:1, :, :1].expand(B, Hkv, 1, D), k_scale, k_zero,
                       v_pool[:1, :, :1].expand(B, Hkv, 1, D), v_scale, v_zero, table, *sides, mid_dtype, mode == 1, causal_offset, key_lengths, out)
    if st.geom is None:
        return st.buf
    st.geom.Tk = Mp * ps
    st.geom.k, st.geom.v = LsqAttnW8Strides(*_pg._pool_strides(k_pool)), LsqAttnW8Strides(*_pg._pool_strides(v_pool))
    return _run(what, st, mode, splits, LsqAttnPagedW8Pages(Np, ps, Mp, bt_ld), k_pool, v_pool, block_table)


def _dec_splits(what, splits):
    _check(isinstance(splits, int) and not isinstance(splits, bool) and splits >= 0,
           "%s: splits must be an int: 0 (the library's choice) or 1 .. ceil(Tk / 64), got %r" % (what, splits))
    return splits


def _plan_geom(B, H, Hkv, Tq, Tk, D, q_strides, k_strides, v_strides, y_strides, q_dtype, k_dtype, v_dtype, causal, causal_offset, has_lengths):
    qs = LsqAttnW8Strides(*(int(n) for n in (q_strides if q_strides is not None else (H * Tq * D, Tq * D, D))))
    ys = LsqAttnW8Strides(*(int(n) for n in (y_strides if y_strides is not None else (Tq * H * D, D, H * D))))
    mode = CAUSAL_LENGTHS if causal == "lengths" else int(causal)
    return LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, _LEVEL_CODE[q_dtype], _LEVEL_CODE[k_dtype], _LEVEL_CODE[v_dtype], mode, int(causal_offset),
                               1 if has_lengths else 0, qs, LsqAttnW8Strides(*(int(n) for n in k_strides)),
                               LsqAttnW8Strides(*(int(n) for n in v_strides)), ys)


def attn_chunk_w8_plan(B, H, Hkv, Tq, Tk, D, splits=0, q_strides=None, k_strides=None, v_strides=None, y_strides=None, qkv_aligned=True,
                       y_aligned=True, q_dtype=torch.uint8, k_dtype=torch.uint8, v_dtype=torch.uint8, causal=False, causal_offset=0,
                       has_lengths=True):
    """What liblsq_hip_attn_chunk_w8.so does with q [B, H, Tq, D], k, v [B, Hkv, Tk, D] and y [B, H, Tq, D]; the arguments are
    `attn_decode_split_w8_plan`'s, `causal` False / True (0 / 1), 2 or "lengths".  Host only.  Returns family "chunk" / "composition",
    grid (= B Hkv tiles splits, the workgroups of each of the first two launches), reduce_grid (= B Hkv tiles, the third's), threads
    (256), rows (R = G Tq), tiles (= ceil(R / 16)), chunk (keys, a multiple of 64), splits (= ceil(Tk / chunk)), lds_bytes (the second
    launch's, 3840 + 160 D), store and workspace_bytes (= B Hkv R 16 ceil(Tk / 16) + 8 B Hkv splits R D); for "composition" the rest is 0."""
    what = "lsq_attn_chunk_w8_plan"
    B, H, Hkv, Tq, Tk, D = (int(n) for n in (B, H, Hkv, Tq, Tk, D))
    splits = _dec_splits(what, splits)
    dense = (Hkv * Tk * D, Tk * D, D)
    geom = _plan_geom(B, H, Hkv, Tq, Tk, D, q_strides, k_strides if k_strides is not None else dense,
                      v_strides if v_strides is not None else dense, y_strides, q_dtype, k_dtype, v_dtype, causal, causal_offset, has_lengths)
    return _plan_call(attn_chunk_w8_library(), geom, None, 1 if qkv_aligned else 0, 1 if y_aligned else 0, splits, what)


def attn_chunk_paged_w8_plan(B, H, Hkv, Tq, D, num_pages, page_size, max_pages, splits=0, bt_ld=None, q_strides=None, k_strides=None,
                             v_strides=None, y_strides=None, qkv_aligned=True, y_aligned=True, q_dtype=torch.uint8, k_dtype=torch.uint8,
                             v_dtype=torch.uint8, causal=False, causal_offset=0, has_lengths=True):
    """The same for pools [num_pages, Hkv, page_size, D] and a block table [B, max_pages]; the arguments are `attn_paged_w8_plan`'s.
    workspace_bytes = B Hkv R max_pages page_size + 8 B Hkv splits R D."""
    what = "lsq_attn_chunk_paged_w8_plan"
    B, H, Hkv, Tq, D, Np, ps, Mp = (int(n) for n in (B, H, Hkv, Tq, D, num_pages, page_size, max_pages))
    splits = _dec_splits(what, splits)
    dense = (Hkv * ps * D, ps * D, D)
    geom = _plan_geom(B, H, Hkv, Tq, Mp * ps, D, q_strides, k_strides if k_strides is not None else dense,
                      v_strides if v_strides is not None else dense, y_strides, q_dtype, k_dtype, v_dtype, causal, causal_offset, has_lengths)
    pages = LsqAttnPagedW8Pages(Np, ps, Mp, Mp if bt_ld is None else int(bt_ld))
    return _plan_call(attn_chunk_w8_library(), geom, pages, 1 if qkv_aligned else 0, 1 if y_aligned else 0, splits, what)
