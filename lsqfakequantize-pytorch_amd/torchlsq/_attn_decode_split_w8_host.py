"""Host layer of SPLIT-KEY decode attention on 8-bit LEVELS (include/lsq_hip_attn_decode_split_w8.h states the contract): the definition,
the operand checks (`_checked`) and the CPU path (`_compose`) are `_attn_decode_w8_host`'s, word for word -- q [B, H, Tq, D] against k, v
[B, Hkv, Tk, D] with H = G Hkv, every row bounded by its key count n(b, t), nothing at or beyond n takes part or is read -- and so are
the bytes: every intermediate of the definition is a defined byte or an exact integer without a summation order, so dealing one kv
head's keys to several workgroups changes none of them.

On the GPU a call asks the library's plan (host only: it runs without a GPU and enqueues nothing).  Family "split": ONE `torch.empty`
of the size `lsq_attn_decode_split_w8_workspace` reports on q's device -- the caching allocator, so the call can be captured in a graph
-- and ONE ctypes call that enqueues three kernels: the chunks' scores, the chunks' exact context integers, their sum and the levels.
Everything else legal ("composition": G Tq > 16, D not a multiple of 16 or beyond 128, a base or a stride that is not a multiple of
16) runs the decode host's composition, with the same bytes.  `splits`: 0 = the library's own choice of the chunk; s >= 1 = at most s
splits (1 .. ceil(Tk / 64); the plan reports the chunk and the splits that result).  `key_lengths` is read in the kernels, never on
the host.

`auto_splits` is the rule behind `torchlsq.functional.lsq_attention_decode_w8_q(..., split="auto")`.
"""
import ctypes

import torch

from . import _attn_decode_w8_host as _dec
from ._abi import LsqAttnDecodeW8Consts, LsqAttnDecodeW8Geom, LsqAttnW8Strides, _assert_has_ops, attn_decode_split_w8_library
from ._attn_w8_host import _STORES, _out_struct
from ._hip_host import _check, _on_device, _stream_of
from ._w8_host_common import _LEVEL_CODE, _act_constants, _status

_FAMILIES = ("composition", "split")
_ERR = "lsq_attn_decode_split_w8_last_error"
# `split="auto"`: the CU count assumed without a device (the MI355X's, as in the library), and the largest grid B Hkv of the
# single-launch kernel, in workgroups per CU, up to which the split form is taken: the largest at which it was measured to win beyond
# the run's spread (profiles/r30_attn_decode_split_w8_ab.txt: 256 workgroups on 256 CUs)
ASSUMED_CUS = 256
AUTO_MAX_GRID_PER_CU = 1.0
AUTO_MIN_CHUNKS = 2


def _plan_dict(out, ws_bytes):
    splits = out[5]
    return dict(family=_FAMILIES[out[0]], grid=out[1], reduce_grid=out[1] // splits if splits else 0, threads=out[2], rows=out[3],
                chunk=out[4], splits=splits, lds_bytes=out[6], store=_STORES[out[7]], workspace_bytes=int(ws_bytes))


def _splits_arg(what, splits):
    _check(isinstance(splits, int) and not isinstance(splits, bool) and splits >= 0,
           "%s: splits must be an int: 0 (the library's choice) or 1 .. ceil(Tk / 64), got %r" % (what, splits))
    return splits


def _plan_of(st, lib, splits, what):
    """the plan and the workspace size for a checked call (host only; both refuse an illegal shape or `splits` with the library's message)"""
    out, ws = (ctypes.c_int32 * 8)(), ctypes.c_int64(0)
    _status(lib.lsq_attn_decode_split_w8_plan(ctypes.byref(st.geom), _dec._aligned(st.q, st.k, st.v) if st.on_gpu else 1,
                                              _dec._aligned(st.yv) if st.on_gpu else 1, splits, ctypes.byref(out)), what, lib, _ERR)
    if out[0]:
        _status(lib.lsq_attn_decode_split_w8_workspace(ctypes.byref(st.geom), splits, ctypes.byref(ws)), what, lib, _ERR)
    return _plan_dict(out, ws.value)


def attn_decode_split_w8_q(q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table, scores_scale, scores_shift,
                           scores_quant_min, scores_quant_max, scores_type_min, scores_type_max, probs_scale, probs_shift, probs_quant_min,
                           probs_quant_max, probs_type_min, probs_type_max, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min,
                           out_type_max, mid_dtype, causal=False, causal_offset=0, key_lengths=None, splits=0, out=None):
    """The arguments and the result of `attn_decode_w8_q` plus `splits` (0: the library's choice; s >= 1: at most s splits of a kv
    head's keys): q [B, H, Tq, D], k and v [B, Hkv, Tk, D] levels (Hkv divides H) with their constants, the softmax `table`, the three
    output quantizers and the mask -> the context's levels [B, Tq, H D] (uint8 or int8), written through their [B, H, Tq, D] view; `out`
    (not an argument of the op) as there.  The same bytes for every `splits`."""
    _assert_has_ops()
    what = "lsq_attention_decode_split_w8_q8_q"
    splits = _splits_arg(what, splits)
    st = _dec._checked(what, q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table,
                       (scores_scale, scores_shift, scores_quant_min, scores_quant_max, scores_type_min, scores_type_max),
                       (probs_scale, probs_shift, probs_quant_min, probs_quant_max, probs_type_min, probs_type_max),
                       (out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max), mid_dtype, causal, causal_offset,
                       key_lengths, out)
    if st.geom is None:
        return st.buf
    lib = attn_decode_split_w8_library()
    plan = _plan_of(st, lib, splits, what)                  # the shape's and the splits' checks, and the family
    if not st.on_gpu or plan["family"] != "split":
        q_s, q_z, k_s, k_z, v_s, v_z = st.consts            # the definition: the existing ops composed
        _dec._compose(st.q, q_s, q_z, st.k, k_s, k_z, st.v, v_s, v_z, st.table, st.s_side, st.p_side, st.o_side, st.mid_dtype, st.sdt,
                      st.causal, st.causal_offset, st.key_lengths, st.yv)
        return st.buf
    ws = torch.empty(plan["workspace_bytes"], dtype=torch.uint8, device=st.q.device)       # the allocator's blocks are 16-byte aligned
    p_s, p_z = _act_constants(st.p_side[0], st.p_side[1], st.p_rng[2], st.p_rng[3])
    q_scale, q_zero, k_scale, k_zero, v_scale, v_zero = st.consts
    consts = LsqAttnDecodeW8Consts(q_scale.data_ptr(), q_zero.data_ptr(), k_scale.data_ptr(), k_zero.data_ptr(), v_scale.data_ptr(),
                                   v_zero.data_ptr(), p_s.data_ptr(), p_z.data_ptr())
    idx = st.q.device.index
    rc = _on_device(idx, lib.lsq_attn_decode_split_w8, ctypes.byref(st.geom), ctypes.byref(consts),
                    ctypes.byref(_out_struct(st.s_side, st.s_rng, st.mid_dtype)), ctypes.byref(_out_struct(st.p_side, st.p_rng, st.mid_dtype)),
                    ctypes.byref(_out_struct(st.o_side, st.o_rng, st.mid_dtype)), st.table.data_ptr(),
                    None if st.key_lengths is None else st.key_lengths.data_ptr(), st.q.data_ptr(), st.k.data_ptr(), st.v.data_ptr(),
                    st.yv.data_ptr(), ws.data_ptr(), ws.numel(), splits, _stream_of(idx))
    _status(rc, "lsq_attn_decode_split_w8", lib, _ERR)
    return st.buf


def auto_splits(B, H, Hkv, Tq, Tk, D, cu_count=None, qkv_aligned=True, **plan_kwargs):
    """The rule of `split="auto"`: True where the split family is taken.  It is where the split plan says "split" and either the
    single-launch decode kernel does not serve the shape (Tk > 8192), or that kernel's grid B Hkv is at most `AUTO_MAX_GRID_PER_CU`
    workgroups per CU (`cu_count`: the device's, `ASSUMED_CUS` without one) and Tk is at least `AUTO_MIN_CHUNKS` of the library's
    chunks.  Host only."""
    cus = ASSUMED_CUS if cu_count is None else int(cu_count)
    plan = attn_decode_split_w8_plan(B, H, Hkv, Tq, Tk, D, qkv_aligned=qkv_aligned, **plan_kwargs)
    if plan["family"] != "split":
        return False
    if _dec.attn_decode_w8_plan(B, H, Hkv, Tq, Tk, D, qkv_aligned=qkv_aligned, **plan_kwargs)["family"] != "decode":
        return True
    return int(B) * int(Hkv) <= AUTO_MAX_GRID_PER_CU * cus and int(Tk) >= AUTO_MIN_CHUNKS * plan["chunk"]


def attn_decode_split_w8_plan(B, H, Hkv, Tq, Tk, D, splits=0, q_strides=None, k_strides=None, v_strides=None, y_strides=None, qkv_aligned=True,
                              y_aligned=True, q_dtype=torch.uint8, k_dtype=torch.uint8, v_dtype=torch.uint8, causal=False, causal_offset=0,
                              has_lengths=True, cu_count=None):
    """What liblsq_hip_attn_decode_split_w8.so does with q [B, H, Tq, D], k, v [B, Hkv, Tk, D] and y [B, H, Tq, D]; the arguments are
    `attn_decode_w8_plan`'s plus `splits`: 0 (the library's choice), s >= 1 (at most s splits), or "auto" -- the rule of
    `lsq_attention_decode_w8_q(split="auto")` (`auto_splits`, with `cu_count`): where it takes the split family the plan of `splits=0`,
    elsewhere `attn_decode_w8_plan`'s dict with `splits=0` added.  Returns family "split" / "composition", grid (= B Hkv splits,
    the workgroups of each of the first two launches), reduce_grid (= B Hkv, the third's), threads (256), rows (R = G Tq), chunk (keys,
    a multiple of 64), splits (= ceil(Tk / chunk)), lds_bytes (the second launch's, 3840 + 160 D), store ("packets" / "elements") and
    workspace_bytes (= B Hkv R 16 ceil(Tk / 16) + 8 B Hkv splits R D); for "composition" the rest is 0."""
    B, H, Hkv, Tq, Tk, D = (int(n) for n in (B, H, Hkv, Tq, Tk, D))
    kw = dict(q_strides=q_strides, k_strides=k_strides, v_strides=v_strides, y_strides=y_strides, y_aligned=y_aligned, q_dtype=q_dtype,
              k_dtype=k_dtype, v_dtype=v_dtype, causal=causal, causal_offset=causal_offset, has_lengths=has_lengths)
    if splits == "auto":
        if auto_splits(B, H, Hkv, Tq, Tk, D, cu_count, qkv_aligned, **kw):
            return attn_decode_split_w8_plan(B, H, Hkv, Tq, Tk, D, 0, qkv_aligned=qkv_aligned, **kw)
        return dict(_dec.attn_decode_w8_plan(B, H, Hkv, Tq, Tk, D, qkv_aligned=qkv_aligned, **kw), splits=0)
    splits = _splits_arg("lsq_attn_decode_split_w8_plan", splits)

    def st(s, heads, T):
        return LsqAttnW8Strides(*(int(n) for n in (s if s is not None else (heads * T * D, T * D, D))))

    ys = LsqAttnW8Strides(*(int(n) for n in (y_strides if y_strides is not None else (Tq * H * D, D, H * D))))
    geom = LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, _LEVEL_CODE[q_dtype], _LEVEL_CODE[k_dtype], _LEVEL_CODE[v_dtype], 1 if causal else 0,
                               int(causal_offset), 1 if has_lengths else 0, st(q_strides, H, Tq), st(k_strides, Hkv, Tk),
                               st(v_strides, Hkv, Tk), ys)
    out, ws = (ctypes.c_int32 * 8)(), ctypes.c_int64(0)
    lib = attn_decode_split_w8_library()
    _status(lib.lsq_attn_decode_split_w8_plan(ctypes.byref(geom), 1 if qkv_aligned else 0, 1 if y_aligned else 0, splits, ctypes.byref(out)),
            "lsq_attn_decode_split_w8_plan", lib, _ERR)
    if out[0]:
        _status(lib.lsq_attn_decode_split_w8_workspace(ctypes.byref(geom), splits, ctypes.byref(ws)), "lsq_attn_decode_split_w8_workspace",
                lib, _ERR)
    return _plan_dict(out, ws.value)
