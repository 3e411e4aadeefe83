"""Host layer of PREFILL attention on 8-bit LEVELS (include/lsq_hip_attn_prefill_w8.h states the contract): causal and key-length
masked, grouped-query attention over ANY number of query rows in one launch.  The definition is `_attn_decode_w8_host`'s, word for
word -- q [B, H, Tq, D] against k, v [B, Hkv, Tk, D] with H = G Hkv, every row bounded by its key count

    n(b, t) = min(Tk,  t + 1 + causal_offset  where causal,  max(key_lengths[b], 0)  where given)

and nothing of k, v or the probabilities at or beyond n takes part -- and so are the operand checks (`_checked`) and the CPU path
(`attn_decode_w8_q`, the composition of the existing ops plus one `torch.where`).

On the GPU a call goes, in this order:
  1  where the DECODE library's plan says "decode" (G Tq <= 16): `attn_decode_w8_q` unchanged -- the G heads share one workgroup there;
  2  else, where this library's plan says "prefill" (D % 16 == 0, 16 <= D <= 128, q, k, v 16-byte aligned with strides that are
     multiples of 16, and Tk_eff = min(Tk, Tq + causal_offset) where causal, else Tk, at most 2048): ONE ctypes call that enqueues
     one kernel -- a workgroup per (b, h, 64 query rows), the scores and the probabilities in LDS, every key loop ended at the
     largest n of its rows;
  3  else the existing composition (`attn_decode_w8_q`, which composes), with the same bytes.
Both plan functions are host only: they run without a GPU and enqueue nothing.  `key_lengths` is read in the kernel, never on the host.
"""
import ctypes

import torch

from . import _attn_decode_w8_host as _dec
from ._abi import LsqAttnDecodeW8Geom, LsqAttnW8Strides, _assert_has_ops, attn_decode_w8_library, attn_prefill_w8_library
from ._w8_host_common import _LEVEL_CODE, _status

_FAMILIES = ("composition", "prefill")
_ERR = "lsq_attn_prefill_w8_last_error"


def attn_prefill_w8_q(q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table, scores_scale, scores_shift,
                      scores_quant_min, scores_quant_max, scores_type_min, scores_type_max, probs_scale, probs_shift, probs_quant_min,
                      probs_quant_max, probs_type_min, probs_type_max, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min,
                      out_type_max, mid_dtype, causal=False, causal_offset=0, key_lengths=None, out=None):
    """The arguments and the result of `attn_decode_w8_q`: q [B, H, Tq, D], k and v [B, Hkv, Tk, D] levels (Hkv divides H) with
    their constants, the softmax `table`, the three output quantizers and the mask -> the context's levels [B, Tq, H D] (uint8 or
    int8), written through their [B, H, Tq, D] view; `out` (not an argument of the op) as there."""
    _assert_has_ops()
    what = "lsq_attention_prefill_w8_q8_q"
    st = _dec._checked(what, q_levels, q_scale, q_zero, k_levels, k_scale, k_zero, v_levels, v_scale, v_zero, table,
                       (scores_scale, scores_shift, scores_quant_min, scores_quant_max, scores_type_min, scores_type_max),
                       (probs_scale, probs_shift, probs_quant_min, probs_quant_max, probs_type_min, probs_type_max),
                       (out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max), mid_dtype, causal, causal_offset,
                       key_lengths, out)
    if st.geom is None or not st.on_gpu:
        return _dec._run(st, what)                      # empty, or the CPU path: the definition
    if _dec._family(st, attn_decode_w8_library(), "lsq_attn_decode_w8_plan", _dec._FAMILIES, what, _dec._ERR) == "decode":
        return _dec._run(st, what)
    lib = attn_prefill_w8_library()
    if _dec._family(st, lib, "lsq_attn_prefill_w8_plan", _FAMILIES, what, _ERR) != "prefill":
        return _dec._run(st, what)                      # the decode host composes
    _dec._launch(st, lib, "lsq_attn_prefill_w8", _ERR)
    return st.buf


def attn_prefill_w8_plan(B, H, Hkv, Tq, Tk, D, q_strides=None, k_strides=None, v_strides=None, y_strides=None, qkv_aligned=True,
                         y_aligned=True, q_dtype=torch.uint8, k_dtype=torch.uint8, v_dtype=torch.uint8, causal=False, causal_offset=0,
                         has_lengths=True):
    """What liblsq_hip_attn_prefill_w8.so does with q [B, H, Tq, D], k, v [B, Hkv, Tk, D] and y [B, H, Tq, D]; the arguments are
    `attn_decode_w8_plan`'s (`*_strides`: (s0, s1, ld) in elements, by default q, k and v dense and y the [B, H, Tq, D] view of a
    [B, Tq, H D] buffer).  Returns family "prefill" / "composition", grid (= B H ceil(Tq / 64)), threads (256), rows (64 per
    workgroup), lds_row_stride (16 n, n = ceil(Tk_eff / 16) made odd), lds_bytes (= 64 lds_row_stride + 1024 + 80 D), lds_dynamic
    (above 64 KB) and store ("packets" / "elements"); for "composition" the rest is 0.  Unlike the decode plan, the mask moves this
    one: Tk_eff = min(Tk, Tq + causal_offset) where causal, else Tk."""
    B, H, Hkv, Tq, Tk, D = (int(n) for n in (B, H, Hkv, Tq, Tk, D))

    def st(s, heads, T):
        return LsqAttnW8Strides(*(int(n) for n in (s if s is not None else (heads * T * D, T * D, D))))

    ys = LsqAttnW8Strides(*(int(n) for n in (y_strides if y_strides is not None else (Tq * H * D, D, H * D))))
    geom = LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, _LEVEL_CODE[q_dtype], _LEVEL_CODE[k_dtype], _LEVEL_CODE[v_dtype], 1 if causal else 0,
                               int(causal_offset), 1 if has_lengths else 0, st(q_strides, H, Tq), st(k_strides, Hkv, Tk),
                               st(v_strides, Hkv, Tk), ys)
    out = (ctypes.c_int32 * 8)()
    lib = attn_prefill_w8_library()
    _status(lib.lsq_attn_prefill_w8_plan(ctypes.byref(geom), 1 if qkv_aligned else 0, 1 if y_aligned else 0, ctypes.byref(out)),
            "lsq_attn_prefill_w8_plan", lib, _ERR)
    return _dec._plan_dict(out, _FAMILIES)
