"""Host layer of DECODE attention on 8-bit LEVELS against a grouped-query KV cache (include/lsq_hip_attn_decode_w8.h states the contract):
q [B, H, Tq, D] against k, v [B, Hkv, Tk, D] with H = G Hkv -- query head h reads kv head h // G --, every row bounded by its key count

    n(b, t) = min(Tk,  t + 1 + causal_offset  where causal,  max(key_lengths[b], 0)  where given)

and NOTHING of k, v or the probabilities at or beyond n takes part.  The CPU path is the definition, a composition of existing
ops plus one `torch.where`:

    k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)                      where G > 1
    s = lsq_bmm_w8_q(q, k, transpose_b=True, <the scores' side>, mid_dtype)
    p = lsq_masked_softmax_w8_q(s, table, <the probabilities' side>, mid_dtype, causal, key_lengths)
    p = where(j >= n, the byte z_p, p)                                               n from tensor ops, nothing is read back
    y = lsq_bmm_w8_q(p, v, False, <the context's side>, mid_dtype, out=<the [B, H, Tq, D] view of a [B, Tq, H D] buffer>)

with (s_p, z_p) = `_act_constants` of the probabilities' quantizer: a key at or beyond n contributes (z_p - z_p)(lv - z_v) = 0
whatever lv is.  Without the `where` this is `AttentionCoreW8Q`'s masked route, which writes the probabilities quantizer's level of
0.0 there: the two agree bit for bit whenever that level equals z_p (every quantizer with shift 0), and where it does not the
masked route depends on cache slots nobody wrote and this op, by definition, does not.

Every call first asks the library's plan function (host only, it runs without a GPU and enqueues nothing), which refuses an illegal
shape with the library's message and names the family: "decode" is ONE ctypes call that enqueues one kernel -- one workgroup per
(b, kv head), the G heads share the k and v reads, every key loop ends at the largest n of the workgroup --; everything else legal
("composition": G Tq > 16, D not a multiple of 16 or beyond 128, Tk beyond 8192, a base or a stride that is not a multiple of 16)
runs the composition above on the GPU, with the same bytes.  `key_lengths` is read in the kernel, never on the host.
"""
import ctypes

import torch

from ._abi import LsqAttnDecodeW8Consts, LsqAttnDecodeW8Geom, LsqAttnW8Strides, _assert_has_ops, attn_decode_w8_library
from ._attn_mask_w8_host import attn_mask_w8_softmax_q
from ._attn_w8_host import _STORES, _in_place, _out_struct, _rows_apart, _strides4, attn_w8_bmm_q
from ._hip_host import _check, _on_device, _stream_of
from ._w8_host_common import _LEVEL_CODE, _act_constants, _check_out_q, _name, _on_one_device, _one, _status

_FAMILIES = ("composition", "decode")
_ERR = "lsq_attn_decode_w8_last_error"


def _plan_dict(out, families=_FAMILIES):
    return dict(family=families[out[0]], grid=out[1], threads=out[2], rows=out[3], lds_row_stride=out[4], lds_bytes=out[5],
                lds_dynamic=bool(out[6]), store=_STORES[out[7]])


def _aligned(*ts):
    return 1 if all(t.data_ptr() % 16 == 0 for t in ts) else 0


def key_counts(B, Tq, Tk, causal, causal_offset, key_lengths, device):
    """n(b, t) of the definition, int64 [B, Tq] on `device`, from tensor ops alone"""
    n = torch.full((B, Tq), Tk, dtype=torch.int64, device=device)
    if causal:
        n = torch.minimum(n, (torch.arange(Tq, dtype=torch.int64, device=device) + (1 + int(causal_offset))).reshape(1, Tq))
    if key_lengths is not None:
        n = torch.minimum(n, key_lengths.to(torch.int64).clamp_min(0).reshape(B, 1))
    return n


def _compose(q, q_s, q_z, k, k_s, k_z, v, v_s, v_z, table, s_side, p_side, o_side, mid_dtype, sdt, causal, causal_offset, key_lengths, yv):
    """the definition on q's device: the existing ops and one `torch.where`, the scores' and the probabilities' rows padded to 16
    bytes as `AttentionCoreW8Q` pads them (the padding changes no byte of the result), the context written into `yv`"""
    B, H, Tq, _ = (int(n) for n in q.shape)
    Tk, G = int(k.shape[-2]), H // int(k.shape[1])
    if G > 1:
        k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    scores = torch.empty((B, H, Tq, (Tk + 15) // 16 * 16), dtype=sdt, device=q.device)
    s = attn_w8_bmm_q(q, q_s, q_z, k, k_s, k_z, True, *s_side, mid_dtype, out=scores[..., :Tk])
    p = attn_mask_w8_softmax_q(s, table, *p_side, mid_dtype, causal, causal_offset, key_lengths, 16)
    p_s, p_z = _act_constants(p_side[0], p_side[1], p_side[4], p_side[5])
    n = key_counts(B, Tq, Tk, causal, causal_offset, key_lengths, q.device)
    beyond = torch.arange(Tk, dtype=torch.int64, device=q.device).reshape(1, 1, 1, Tk) >= n.reshape(B, 1, Tq, 1)
    p.copy_(torch.where(beyond, p_z.to(torch.int64).to(p.dtype), p))       # a key at or beyond n: the byte z_p, which contributes 0
    attn_w8_bmm_q(p, p_s, p_z, v, v_s, v_z, False, *o_side, mid_dtype, out=yv)


class _Call:
    """one checked call: the operands as the kernels read them, the sides, the mask, the geometry and where the result goes"""


def _checked(what, q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table, s_side, p_side, o_side,
             mid_dtype, causal, causal_offset, key_lengths, out):
    """the operand checks of `attn_decode_w8_q`, which `_attn_prefill_w8_host.attn_prefill_w8_q` makes too (`what` names the op in
    the messages), and the result's buffer -> a `_Call`; its `geom` is None where the result is empty"""
    q, k, v = q_levels, k_levels, v_levels
    for name, t in (("q", q), ("k", k), ("v", v)):
        _check(t.dtype in _LEVEL_CODE, "%s: the levels of %s must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, name, _name(t.dtype)))
    _check(q.dim() == 4 and k.dim() == 4 and v.dim() == 4 and tuple(k.shape) == tuple(v.shape) and q.shape[0] == k.shape[0]
           and q.shape[3] == k.shape[3], "%s: q must be [B, H, Tq, D] and k, v [B, Hkv, Tk, D], got %s, %s and %s"
           % (what, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    B, H, Tq, D = (int(n) for n in q.shape)
    Hkv, Tk = int(k.shape[1]), int(k.shape[2])
    _check(Hkv >= 1 and H % Hkv == 0, "%s: H = %d query heads are not a multiple of Hkv = %d kv heads" % (what, H, Hkv))
    for name, s, z in (("q", q_scale, q_zero), ("k", k_scale, k_zero), ("v", v_scale, v_zero)):
        _check(_one(s, torch.float32) and _one(z, torch.int32),
               "%s: %s's scale must be one float32 value and its zero point one int32 value (tensors on the levels' device)" % (what, name))
    _check(table.dtype == torch.int32 and tuple(table.shape) == (256,) and table.is_contiguous(),
           "%s: the table must be a dense int32 tensor of [256] (lsq_softmax_table), got '%s' %s" % (what, _name(table.dtype), tuple(table.shape)))
    causal, causal_offset = bool(causal), int(causal_offset)
    _check(not causal or causal_offset >= 0, "%s: causal_offset = %d must be at least 0" % (what, causal_offset))
    causal_offset = causal_offset if causal else 0
    if key_lengths is not None:
        _check(key_lengths.dtype == torch.int32 and tuple(key_lengths.shape) == (B,) and key_lengths.is_contiguous(),
               "%s: key_lengths must be a dense int32 tensor of [%d], one entry per batch index, got '%s' %s"
               % (what, B, _name(key_lengths.dtype), tuple(key_lengths.shape)))
    st = _Call()
    st.s_side, st.p_side, st.o_side = (tuple(side[:2]) + tuple(int(n) for n in side[2:]) for side in (s_side, p_side, o_side))
    st.sdt, st.s_rng, _ = _check_out_q(what + " (scores)", st.s_side, mid_dtype)
    _, st.p_rng, _ = _check_out_q(what + " (probabilities)", st.p_side, mid_dtype)
    ydt, st.o_rng, _ = _check_out_q(what + " (context)", st.o_side, mid_dtype)
    tensors = (q, k, v, q_scale, q_zero, k_scale, k_zero, v_scale, v_zero, table) + st.s_side[:2] + st.p_side[:2] + st.o_side[:2] + \
        (() if key_lengths is None else (key_lengths,)) + (() if out is None else (out,))
    st.on_gpu = _on_one_device(what, tensors)
    if out is None:
        st.buf = torch.empty((B, Tq, H * D), dtype=ydt, device=q.device)
        st.yv = st.buf.view(B, Tq, H, D).permute(0, 2, 1, 3)
    else:
        _check(out.dtype == ydt and tuple(out.shape) == (B, H, Tq, D) and (D == 1 or out.stride(-1) == 1) and _rows_apart(out),
               "%s: `out` must be a %s tensor of shape %s whose innermost stride is 1 and whose rows do not overlap"
               % (what, _name(ydt), (B, H, Tq, D)))
        st.buf = st.yv = out
    st.geom = None
    if st.buf.numel() == 0:
        return st
    _check(Tk > 0, "%s: Tk = 0 is not served" % what)
    st.q, st.k, st.v = _in_place(q, st.on_gpu), _in_place(k, st.on_gpu), _in_place(v, st.on_gpu)
    st.consts = (q_scale, q_zero, k_scale, k_zero, v_scale, v_zero)
    st.table, st.mid_dtype, st.causal, st.causal_offset, st.key_lengths = table, mid_dtype, causal, causal_offset, key_lengths
    st.geom = LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, _LEVEL_CODE[st.q.dtype], _LEVEL_CODE[st.k.dtype], _LEVEL_CODE[st.v.dtype],
                                  1 if causal else 0, causal_offset, 0 if key_lengths is None else 1, _strides4(st.q), _strides4(st.k),
                                  _strides4(st.v), _strides4(st.yv))
    return st


def _family(st, lib, plan_entry, families, what, err):
    """the family the library's plan function names for a checked call (host only; it refuses an illegal shape with its message)"""
    plan = (ctypes.c_int32 * 8)()
    _status(getattr(lib, plan_entry)(ctypes.byref(st.geom), _aligned(st.q, st.k, st.v) if st.on_gpu else 1,
                                     _aligned(st.yv) if st.on_gpu else 1, ctypes.byref(plan)), what, lib, err)
    return families[plan[0]]


def _launch(st, lib, entry, err):
    """ONE ctypes call of a library's entry with lsq_attn_decode_w8's argument list on a checked call"""
    p_s, p_z = _act_constants(st.p_side[0], st.p_side[1], st.p_rng[2], st.p_rng[3])
    q_scale, q_zero, k_scale, k_zero, v_scale, v_zero = st.consts
    consts = LsqAttnDecodeW8Consts(q_scale.data_ptr(), q_zero.data_ptr(), k_scale.data_ptr(), k_zero.data_ptr(), v_scale.data_ptr(),
                                   v_zero.data_ptr(), p_s.data_ptr(), p_z.data_ptr())
    idx = st.q.device.index
    rc = _on_device(idx, getattr(lib, entry), ctypes.byref(st.geom), ctypes.byref(consts),
                    ctypes.byref(_out_struct(st.s_side, st.s_rng, st.mid_dtype)), ctypes.byref(_out_struct(st.p_side, st.p_rng, st.mid_dtype)),
                    ctypes.byref(_out_struct(st.o_side, st.o_rng, st.mid_dtype)), st.table.data_ptr(),
                    None if st.key_lengths is None else st.key_lengths.data_ptr(), st.q.data_ptr(), st.k.data_ptr(), st.v.data_ptr(),
                    st.yv.data_ptr(), _stream_of(idx))
    _status(rc, entry, lib, err)


def attn_decode_w8_q(q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table, scores_scale, scores_shift,
                     scores_quant_min, scores_quant_max, scores_type_min, scores_type_max, probs_scale, probs_shift, probs_quant_min,
                     probs_quant_max, probs_type_min, probs_type_max, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min,
                     out_type_max, mid_dtype, causal=False, causal_offset=0, key_lengths=None, out=None, what="lsq_attention_decode_w8_q8_q"):
    """q [B, H, Tq, D], k and v [B, Hkv, Tk, D] levels (Hkv divides H) with their constants, the softmax `table`, the three output
    quantizers and the mask -> the context's levels [B, Tq, H D] (uint8 or int8), written through their [B, H, Tq, D] view.  `out`
    (not an argument of the op): a tensor [B, H, Tq, D] with unit innermost stride and rows that do not overlap to write into and
    return instead; bytes outside it are not written.  `what` (not an argument of the op): the op named in the messages."""
    _assert_has_ops()
    st = _checked(what, q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table,
                  (scores_scale, scores_shift, scores_quant_min, scores_quant_max, scores_type_min, scores_type_max),
                  (probs_scale, probs_shift, probs_quant_min, probs_quant_max, probs_type_min, probs_type_max),
                  (out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max), mid_dtype, causal, causal_offset,
                  key_lengths, out)
    return _run(st, what)


def _run(st, what):
    """a checked call through the decode library: its kernel where its plan says "decode" on the GPU, the composition elsewhere"""
    if st.geom is None:
        return st.buf
    lib = attn_decode_w8_library()
    family = _family(st, lib, "lsq_attn_decode_w8_plan", _FAMILIES, what, _ERR)      # the shape's checks, and the family
    if not st.on_gpu or family != "decode":
        q_scale, q_zero, k_scale, k_zero, v_scale, v_zero = st.consts
        _compose(st.q, q_scale, q_zero, st.k, k_scale, k_zero, st.v, v_scale, v_zero, st.table, st.s_side, st.p_side, st.o_side,
                 st.mid_dtype, st.sdt, st.causal, st.causal_offset, st.key_lengths, st.yv)
        return st.buf
    _launch(st, lib, "lsq_attn_decode_w8", _ERR)
    return st.buf


def attn_decode_w8_plan(B, H, Hkv, Tq, Tk, D, q_strides=None, k_strides=None, v_strides=None, y_strides=None, qkv_aligned=True,
                        y_aligned=True, q_dtype=torch.uint8, k_dtype=torch.uint8, v_dtype=torch.uint8, causal=False, causal_offset=0,
                        has_lengths=True):
    """What liblsq_hip_attn_decode_w8.so does with q [B, H, Tq, D], k, v [B, Hkv, Tk, D] and y [B, H, Tq, D]; `*_strides`: (s0, s1, ld)
    in elements, by default q, k and v dense and y the [B, H, Tq, D] view of a [B, Tq, H D] buffer.  Returns family "decode" /
    "composition", grid (= B Hkv), threads, rows (R = G Tq), lds_row_stride, lds_bytes, lds_dynamic (above 64 KB) and store
    ("packets" / "elements"); for "composition" the rest is 0."""
    B, H, Hkv, Tq, Tk, D = (int(n) for n in (B, H, Hkv, Tq, Tk, D))

    def st(s, heads, T):
        return LsqAttnW8Strides(*(int(n) for n in (s if s is not None else (heads * T * D, T * D, D))))

    ys = LsqAttnW8Strides(*(int(n) for n in (y_strides if y_strides is not None else (Tq * H * D, D, H * D))))
    geom = LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, _LEVEL_CODE[q_dtype], _LEVEL_CODE[k_dtype], _LEVEL_CODE[v_dtype], 1 if causal else 0,
                               int(causal_offset), 1 if has_lengths else 0, st(q_strides, H, Tq), st(k_strides, Hkv, Tk),
                               st(v_strides, Hkv, Tk), ys)
    out = (ctypes.c_int32 * 8)()
    lib = attn_decode_w8_library()
    _status(lib.lsq_attn_decode_w8_plan(ctypes.byref(geom), 1 if qkv_aligned else 0, 1 if y_aligned else 0, ctypes.byref(out)),
            "lsq_attn_decode_w8_plan", lib, _ERR)
    return _plan_dict(out)
