"""What tests/test_attn_prefill_w8_cpu.py and tests/test_attn_prefill_w8_gpu.py share.  The inputs, the fitted quantizers and the
DEFINITION are `attn_decode_w8_cases`' unchanged -- `definition(c)` is the CPU path of `lsq_attention_decode_w8_q`, code of the
parent commit and not the code under test --; this module adds the prefill op run on a device of choice, the direct call of the
prefill library's C entry (no Python host, so no fallback behind it) and the prefill plan of a case.
"""
import torch

import attn_decode_w8_cases as C
import attn_fused_w8_cases as F
import attn_w8_cases as A

U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
GUARD = C.GUARD
LSQ_EINVAL = -1
Z3 = (A.QKV_Z,) * 3
SIGNED_PV = (True, False, False)       # fitted int8 probabilities and context: many keys leave a quint8 probability few levels


def case(B, Hkv, G, Tq, Tk, D, seed=0, dtypes=C.ALL_U8, unsigned=None, mid=BF16, zeros=Z3, table=None, causal=0, lengths=None):
    """`attn_decode_w8_cases.case` (cached there, the definition computed once), SIGNED_PV from 1024 keys on unless given"""
    if unsigned is None:
        unsigned = SIGNED_PV if Tk >= 1024 else C.ALL_UNSIGNED
    return C.case(B, Hkv, G, Tq, Tk, D, seed, dtypes, unsigned, mid, zeros, table, causal, lengths)


def tk_eff(c):
    B, H, Hkv, Tq, Tk, D = c.shape
    on, off = C.causal_args(c)
    return min(Tk, Tq + min(off, Tk)) if on else Tk


def run(c, dev, shift=(0, 0, 0), k=None, v=None):
    """`lsq_attention_prefill_w8_q` of the case on `dev` -> the levels [B, Tq, H D]"""
    from torchlsq.functional import lsq_attention_prefill_w8_q
    q, k, v = (C.moved(x, dev, sh) for x, sh in zip((c.q, c.k if k is None else k, c.v if v is None else v), shift))
    return lsq_attention_prefill_w8_q(q, k, v, c.table.to(dev), *F.sides_on(c.sides, dev), c.mid, causal=c.causal,
                                      key_lengths=None if c.lengths is None else c.lengths.to(dev)).levels


def c_entry(c, dev, shift=(0, 0, 0), k=None, v=None):
    """`lsq_attn_prefill_w8` of liblsq_hip_attn_prefill_w8.so called directly on the case's operands on `dev` -> (status, the levels
    [B, Tq, H D], prefilled with 0x5A)"""
    import ctypes
    from torchlsq import extension as E
    from torchlsq._attn_w8_host import _DTYPE_CODE, _LEVEL_CODE
    from torchlsq.functional import _act_constants
    B, H, Hkv, Tq, Tk, D = c.shape
    q, k, v = (C.moved(x, dev, sh) for x, sh in zip((c.q, c.k if k is None else k, c.v if v is None else v), shift))
    sides, tab = F.sides_on(c.sides, dev), c.table.to(dev)
    lens = None if c.lengths is None else c.lengths.to(dev)
    y = torch.full((B, Tq, H * D), GUARD, dtype=U8, device=dev).view(c.want.dtype)
    S = E.LsqAttnW8Strides
    on, off = C.causal_args(c)
    geom = E.LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, *(_LEVEL_CODE[x.levels.dtype] for x in (q, k, v)), 1 if on else 0, off,
                                 0 if lens is None else 1, *(S(*F.strides(x.levels)) for x in (q, k, v)),
                                 S(*F.strides(y.view(B, Tq, H, D).permute(0, 2, 1, 3))))
    p_s, p_z = _act_constants(sides[1][0], sides[1][1], sides[1][4], sides[1][5])
    consts = E.LsqAttnDecodeW8Consts(q.scale.data_ptr(), q.zero_point.data_ptr(), k.scale.data_ptr(), k.zero_point.data_ptr(),
                                     v.scale.data_ptr(), v.zero_point.data_ptr(), p_s.data_ptr(), p_z.data_ptr())
    outs = [E.LsqAttnW8Out(s[0].data_ptr(), s[1].data_ptr(), *s[2:], _DTYPE_CODE[c.mid]) for s in sides]
    torch.cuda.synchronize()                            # the call below goes to the default stream
    rc = E.attn_prefill_w8_library().lsq_attn_prefill_w8(ctypes.byref(geom), ctypes.byref(consts), *(ctypes.byref(o) for o in outs),
                                                         tab.data_ptr(), None if lens is None else lens.data_ptr(), q.levels.data_ptr(),
                                                         k.levels.data_ptr(), v.levels.data_ptr(), y.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, y


def plan_of(c, qkv_aligned=True, y_aligned=True, y_strides=None, overrides=()):
    """the prefill plan for the case's operands as they lie on the CPU (the strides are what `moved` keeps)"""
    from torchlsq import extension as E
    B, H, Hkv, Tq, Tk, D = c.shape
    st = dict(q_strides=F.strides(c.q.levels), k_strides=F.strides(c.k.levels), v_strides=F.strides(c.v.levels), y_strides=y_strides)
    st.update(dict(overrides))
    on, off = C.causal_args(c)
    return E.attn_prefill_w8_plan(B, H, Hkv, Tq, Tk, D, qkv_aligned=qkv_aligned, y_aligned=y_aligned, q_dtype=c.q.levels.dtype,
                                  k_dtype=c.k.levels.dtype, v_dtype=c.v.levels.dtype, causal=on, causal_offset=off,
                                  has_lengths=c.lengths is not None, **st)


def ld_of(tk):
    return 16 * (((tk + 15) // 16) | 1)


def expected_plan(c, store="packets"):
    """the served plan by the header's formulas"""
    B, H, Hkv, Tq, Tk, D = c.shape
    ld = ld_of(tk_eff(c))
    lds = 64 * ld + 1024 + 80 * D
    return dict(family="prefill", grid=B * H * ((Tq + 63) // 64), threads=256, rows=64, lds_row_stride=ld, lds_bytes=lds,
                lds_dynamic=lds > 65536, store=store)


def poisoned_from(c, first, fill):
    """(k, v) of the case with every slot from `first` on filled with the byte `fill`"""
    out = []
    for x in (c.k, c.v):
        lv = x.levels.clone()
        lv.view(U8)[:, :, first:] = fill
        out.append(C.with_levels(x, lv))
    return out


def core(D, **kw):
    """an `AttentionCoreW8Q` with three quint8 quantizers of shift 0 fitted to full-range levels (test_attn_decode_w8_cpu's)"""
    from torchlsq.quantized import AttentionCoreW8Q
    span = 6.0 * A.QKV_S * A.QKV_S * 74 * 74 * D ** 0.5
    return AttentionCoreW8Q(A.trained(-span, span), A.trained(0.0, 1.0), A.trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16, **kw)


def core_sides(m):
    return m.scores._out("output"), m.softmax._out("output"), m.context._out("output")
