"""What tests/test_attn_decode_w8_cpu.py and tests/test_attn_decode_w8_gpu.py share: inputs of decode attention on 8-bit levels -- q as
the [B, H, Tq, D] view of a [B, Tq, H, D] buffer, k and v as two dense cache buffers [B, Hkv, Tk, D] whose last row ends with the
storage, full-range random levels --, the three output quantizers fitted as `attn_fused_w8_cases` fits them (on the unmasked
intermediates of the expanded k and v), the DEFINITION (the op's CPU path, computed once per case and shared; the CPU tests hold it
to plain integers, to the existing module and to poisoned slots) and the op run on a device of choice.  Everything is seeded;
tables are built once on the CPU and moved.
"""
import functools

import torch

import attn_fused_w8_cases as F
import attn_w8_cases as A

U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
ALL_U8, ALL_UNSIGNED, COMBOS = F.ALL_U8, F.ALL_UNSIGNED, F.COMBOS
GUARD = 0x5A


class Case:
    """q, k, v: LevelsTensors on the CPU; table; sides = (scores, probs, out) 6-tuples; mid; causal; lengths (int32 [B] or None);
    want: the definition's levels [B, Tq, H D]"""


def inputs(B, Hkv, G, Tq, Tk, D, seed, dtypes=ALL_U8, zeros=(A.QKV_Z,) * 3):
    H = Hkv * G
    raw = [A.levels((B, Tq, H, D), 80 + seed, U8).permute(0, 2, 1, 3), A.levels((B, Hkv, Tk, D), 81 + seed, U8),
           A.levels((B, Hkv, Tk, D), 82 + seed, U8)]
    return [F.level_tensor(t if dt == U8 else t.view(I8), z) for t, dt, z in zip(raw, dtypes, zeros)]


def with_levels(x, levels):
    from torchlsq.functional import LevelsTensor
    return LevelsTensor(levels, x.scale, x.zero_point, x.quant_min, x.quant_max, x.type_min, x.type_max)


def expanded(x, G):
    """k or v as the parent route needs it: every kv head repeated G times"""
    return x if G == 1 else with_levels(x, x.levels.repeat_interleave(G, dim=1))


def lens_tensor(lengths):
    return None if lengths is None else torch.tensor(list(lengths), dtype=torch.int32)


def key_counts(B, Tq, Tk, causal, lengths):
    """n(b, t) by plain Python: a list of B lists of Tq counts"""
    off = None if causal is None or causal is False else (Tk - Tq if causal is True else int(causal))
    return [[min([Tk] + ([t + 1 + off] if off is not None else []) + ([max(int(lengths[b]), 0)] if lengths is not None else []))
             for t in range(Tq)] for b in range(B)]


def definition(c, q=None, k=None, v=None):
    """the op's CPU path on the case (or on operands given instead) -> the levels [B, Tq, H D]"""
    from torchlsq.functional import lsq_attention_decode_w8_q
    q, k, v = (d if x is None else x for x, d in zip((q, k, v), (c.q, c.k, c.v)))
    return lsq_attention_decode_w8_q(q, k, v, c.table, *c.sides, c.mid, causal=c.causal, key_lengths=c.lengths).levels


@functools.lru_cache(maxsize=None)
def case(B, Hkv, G, Tq, Tk, D, seed=0, dtypes=ALL_U8, unsigned=ALL_UNSIGNED, mid=BF16, zeros=(A.QKV_Z,) * 3, table=None, causal=True,
         lengths=None):
    """`table` as in `attn_fused_w8_cases.case`; `lengths`: a tuple of B ints or None"""
    c = Case()
    c.shape, c.G = (B, Hkv * G, Hkv, Tq, Tk, D), G
    c.q, c.k, c.v = inputs(B, Hkv, G, Tq, Tk, D, seed, dtypes, zeros)
    c.mid, c.causal, c.lengths = mid, causal, lens_tensor(lengths)
    given = {None: None, "full": A.full_table(), "zeros": A.table_with_zeros()}[table]
    c.table, c.sides = F.fitted_sides(c.q, expanded(c.k, G), expanded(c.v, G), unsigned, mid, given)
    c.want = definition(c)
    return c


def finish(c):
    c.want = definition(c)
    return c


def check_not_degenerate(c):
    """for at least 16 keys in every row and at least 256 outputs: more than 16 distinct output levels"""
    B, H, Hkv, Tq, Tk, D = c.shape
    n = key_counts(B, Tq, Tk, c.causal, None if c.lengths is None else c.lengths.tolist())
    if min(min(r) for r in n) >= 16 and c.want.numel() >= 256:
        assert len(c.want.unique()) > 16, (c.shape, len(c.want.unique()))


def moved(x, dev, shift=0):
    return F.moved(x, dev, shift)


def run(c, dev, shift=(0, 0, 0), k=None, v=None):
    """`lsq_attention_decode_w8_q` of the case on `dev` -> the levels [B, Tq, H D]"""
    from torchlsq.functional import lsq_attention_decode_w8_q
    q, k, v = (moved(x, dev, sh) for x, sh in zip((c.q, c.k if k is None else k, c.v if v is None else v), shift))
    return lsq_attention_decode_w8_q(q, k, v, c.table.to(dev), *F.sides_on(c.sides, dev), c.mid, causal=c.causal,
                                     key_lengths=None if c.lengths is None else c.lengths.to(dev)).levels


def causal_args(c):
    B, H, Hkv, Tq, Tk, D = c.shape
    if c.causal is None or c.causal is False:
        return False, 0
    return True, (Tk - Tq if c.causal is True else int(c.causal))


def flat_args(c, dev, shift=(0, 0, 0)):
    """the arguments of torch.ops.torchlsq.lsq_attention_decode_w8_q8_q / extension.attn_decode_w8_q for the case on `dev`"""
    q, k, v = (moved(x, dev, sh) for x, sh in zip((c.q, c.k, c.v), shift))
    sides = F.sides_on(c.sides, dev)
    return (q.levels, q.scale, q.zero_point, k.levels, k.scale, k.zero_point, v.levels, v.scale, v.zero_point, c.table.to(dev),
            *sides[0], *sides[1], *sides[2], c.mid, *causal_args(c), None if c.lengths is None else c.lengths.to(dev))


def c_entry(c, dev, shift=(0, 0, 0)):
    """`lsq_attn_decode_w8` of liblsq_hip_attn_decode_w8.so called directly on the case's operands on `dev`: no Python host, so no
    fallback -> (status, the levels [B, Tq, H D], prefilled with 0x5A)"""
    import ctypes
    from torchlsq import extension as E
    from torchlsq._attn_w8_host import _DTYPE_CODE, _LEVEL_CODE
    from torchlsq.functional import _act_constants
    B, H, Hkv, Tq, Tk, D = c.shape
    q, k, v = (moved(x, dev, sh) for x, sh in zip((c.q, c.k, c.v), shift))
    sides, tab = F.sides_on(c.sides, dev), c.table.to(dev)
    lens = None if c.lengths is None else c.lengths.to(dev)
    y = torch.full((B, Tq, H * D), GUARD, dtype=U8, device=dev).view(c.want.dtype)
    S = E.LsqAttnW8Strides
    on, off = causal_args(c)
    geom = E.LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, *(_LEVEL_CODE[x.levels.dtype] for x in (q, k, v)), 1 if on else 0, off,
                                 0 if lens is None else 1, *(S(*F.strides(x.levels)) for x in (q, k, v)),
                                 S(*F.strides(y.view(B, Tq, H, D).permute(0, 2, 1, 3))))
    p_s, p_z = _act_constants(sides[1][0], sides[1][1], sides[1][4], sides[1][5])
    consts = E.LsqAttnDecodeW8Consts(q.scale.data_ptr(), q.zero_point.data_ptr(), k.scale.data_ptr(), k.zero_point.data_ptr(),
                                     v.scale.data_ptr(), v.zero_point.data_ptr(), p_s.data_ptr(), p_z.data_ptr())
    outs = [E.LsqAttnW8Out(s[0].data_ptr(), s[1].data_ptr(), *s[2:], _DTYPE_CODE[c.mid]) for s in sides]
    torch.cuda.synchronize()                            # the call below goes to the default stream
    rc = E.attn_decode_w8_library().lsq_attn_decode_w8(ctypes.byref(geom), ctypes.byref(consts), *(ctypes.byref(o) for o in outs),
                                                       tab.data_ptr(), None if lens is None else lens.data_ptr(), q.levels.data_ptr(),
                                                       k.levels.data_ptr(), v.levels.data_ptr(), y.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, y


def plan_of(c, qkv_aligned=True, y_aligned=True, y_strides=None, overrides=()):
    """the plan for the case's operands as they lie on the CPU (the strides are what `moved` keeps)"""
    from torchlsq import extension as E
    B, H, Hkv, Tq, Tk, D = c.shape
    st = dict(q_strides=F.strides(c.q.levels), k_strides=F.strides(c.k.levels), v_strides=F.strides(c.v.levels), y_strides=y_strides)
    st.update(dict(overrides))
    on, off = causal_args(c)
    return E.attn_decode_w8_plan(B, H, Hkv, Tq, Tk, D, qkv_aligned=qkv_aligned, y_aligned=y_aligned, q_dtype=c.q.levels.dtype,
                                 k_dtype=c.k.levels.dtype, v_dtype=c.v.levels.dtype, causal=on, causal_offset=off,
                                 has_lengths=c.lengths is not None, **st)


def poisoned(c, fill):
    """(k, v) of the case with every slot at or beyond max_t n(b, t) filled with the byte `fill`"""
    B, H, Hkv, Tq, Tk, D = c.shape
    n = key_counts(B, Tq, Tk, c.causal, None if c.lengths is None else c.lengths.tolist())
    out = []
    for x in (c.k, c.v):
        lv = x.levels.clone()
        for b in range(B):
            lv.view(U8)[b, :, max(n[b]):] = fill
        out.append(with_levels(x, lv))
    return out


# ---------------------------------------------------------------------------------------------------
# decode equals prefill with grouped-query heads: H = 4 on Hkv = 2 through KVCacheW8(2, 2, 16, 32)
# ---------------------------------------------------------------------------------------------------
_GQA = {}


def gqa_decode_case():
    """B 2, H 4, Hkv 2, T 7, D 32, Tmax 16: the q and kv levels, the modules, and the causal prefill's context [B, T, H D] through the
    existing core on expanded k and v, on the CPU -- computed once"""
    if not _GQA:
        from torchlsq.functional import LevelsTensor
        from torchlsq.quantized import AttentionCoreW8Q, RotaryW8Q
        B, H, Hkv, T, D = 2, 4, 2, 7, 32
        qb, kv = A.levels((B, T, H, D), 90, U8), A.levels((B, T, 2, Hkv, D), 91, U8)
        consts = (A.one(A.QKV_S), A.one(A.QKV_Z, torch.int32))
        rot = RotaryW8Q(A.trained(-4.0, 4.0), D, 16, mid_dtype=BF16)
        core = AttentionCoreW8Q(A.trained(-60.0, 60.0), A.trained(0.0, 1.0), A.trained(-3.0, 3.0), alpha=D ** -0.5, mid_dtype=BF16, causal=True)
        q, k, v = LevelsTensor(qb, *consts, 0, 255), LevelsTensor(kv[:, :, 0], *consts, 0, 255), LevelsTensor(kv[:, :, 1], *consts, 0, 255)
        rq, rk = rot(q), rot(k)

        def heads(lt, G=1):
            lv = lt.levels.permute(0, 2, 1, 3)
            return LevelsTensor(lv if G == 1 else lv.repeat_interleave(G, dim=1), lt.scale, lt.zero_point, lt.quant_min, lt.quant_max)
        prefill = core(heads(rq), heads(rk, H // Hkv), heads(v, H // Hkv)).levels
        _GQA.update(B=B, H=H, Hkv=Hkv, T=T, D=D, Tmax=16, q=qb, kv=kv, consts=consts, rot=rot, core=core, prefill=prefill)
    return _GQA


def gqa_decode_step(case, rot, core, cache, t, dev="cpu", tokens=None):
    """step t of the decode on `dev`: q and k of token t rotated at the cache's lengths, k and v appended, `core` (decode=True) on the
    cache as it is -> the context's levels [B, 1, H D].  `tokens`: (q, kv) device buffers [B, 1, ..] to read instead (a graph's)"""
    from torchlsq.functional import LevelsTensor
    qt, kvt = (case["q"][:, t:t + 1].to(dev), case["kv"][:, t:t + 1].to(dev)) if tokens is None else tokens
    consts = tuple(c.to(dev) for c in case["consts"])
    q, k, v = LevelsTensor(qt, *consts, 0, 255), LevelsTensor(kvt[:, :, 0], *consts, 0, 255), LevelsTensor(kvt[:, :, 1], *consts, 0, 255)
    rq = rot(q, positions=cache.lengths)
    kl, vl, lens = cache.append(k, v, rotary=rot)
    return core(LevelsTensor(rq.levels.permute(0, 2, 1, 3), rq.scale, rq.zero_point, rq.quant_min, rq.quant_max), kl, vl, key_lengths=lens).levels
