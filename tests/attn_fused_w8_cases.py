"""What tests/test_attn_fused_w8_cpu.py and tests/test_attn_fused_w8_gpu.py share: inputs of the fused attention core on 8-bit levels
(q, k, v as views of one qkv buffer where Tq == Tk, of a q and a kv buffer elsewhere; full-range random levels), the three output
quantizers -- `attn_w8_cases.core_case`'s, or `fit_quantizer`'s on the CPU intermediates for an int8 side --, the DEFINITION (the
three functional calls on the CPU, computed once per case and shared) and the op run on a device of choice.  Everything is seeded;
tables are built once on the CPU and moved.
"""
import functools

import torch

import attn_w8_cases as A

U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
ALL_U8 = (U8, U8, U8)
ALL_UNSIGNED = (True, True, True)
# two of the uint8 / int8 combinations of (q, k, v) and of the (scores, probabilities, context) sides for every shape
COMBOS = (((U8, I8, U8), (False, True, False)), ((I8, U8, I8), (True, False, True)))


class Case:
    """q, k, v: LevelsTensors on the CPU; table; sides = (scores, probs, out) 6-tuples; mid; s, p: the CPU intermediates' levels;
    want: the definition's levels [B, Tq, H D]"""


def level_tensor(levels, zero_u8):
    from torchlsq.functional import LevelsTensor
    rng = (0, 255) if levels.dtype == U8 else (-128, 127)
    return LevelsTensor(levels, A.one(A.QKV_S), A.zero_for(levels.dtype, zero_u8), *rng)


def inputs(B, H, Tq, Tk, D, seed, dtypes=ALL_U8, zeros=(A.QKV_Z,) * 3):
    """q [B, H, Tq, D], k, v [B, H, Tk, D]: views of one [B, T, 3, H, D] buffer where Tq == Tk, else of [B, Tq, H, D] and [B, Tk, 2, H, D]"""
    if Tq == Tk:
        buf = A.levels((B, Tq, 3, H, D), 50 + seed, U8)
        raw = [buf[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    else:
        qb, kv = A.levels((B, Tq, H, D), 50 + seed, U8), A.levels((B, Tk, 2, H, D), 51 + seed, U8)
        raw = [qb.permute(0, 2, 1, 3)] + [kv[:, :, i].permute(0, 2, 1, 3) for i in range(2)]
    return [level_tensor(t if dt == U8 else t.view(I8), z) for t, dt, z in zip(raw, dtypes, zeros)]


def definition(q, k, v, table, sides, mid):
    """(s levels, p levels, the result's levels [B, Tq, H D]): the three functional calls on the operands' device"""
    from torchlsq.functional import lsq_bmm_w8_q, lsq_softmax_w8_q
    B, H, Tq, D = (int(n) for n in q.shape)
    s = lsq_bmm_w8_q(q, k, True, *sides[0], mid)
    p = lsq_softmax_w8_q(s, table, *sides[1], mid)
    buf = torch.empty((B, Tq, H * D), dtype=U8 if max(sides[2][3], sides[2][5]) > 127 else I8, device=q.levels.device)
    lsq_bmm_w8_q(p, v, False, *sides[2], mid, out=buf.view(B, Tq, H, D).permute(0, 2, 1, 3))
    return s.levels, p.levels, buf


def core_sides(D):
    """the three sides of `attn_w8_cases.core_case`'s module (quint8 quantizers), alpha and the module's table"""
    core = A.core_case(1, 1, 16, D)[0]
    return (core.scores._out("output"), core.softmax._out("output"), core.context._out("output")), D ** -0.5, core.softmax.table


def fitted_sides(q, k, v, unsigned, mid, table=None):
    """(table, sides): a side that is not `unsigned` is `fit_quantizer(values, unsigned=False)` on the CPU intermediate it
    quantizes, an unsigned one is the core's quint8 quantizer; the table follows the scores' scale unless given"""
    from torchlsq.functional import lsq_bmm_w8, lsq_bmm_w8_q, lsq_softmax_table, lsq_softmax_w8, lsq_softmax_w8_q
    D = int(q.shape[-1])
    sides, alpha, tab = core_sides(D)
    sides = list(sides)
    if not unsigned[0]:
        sides[0] = A.fit_quantizer(lsq_bmm_w8(q, k, True, F32), False)
        tab = lsq_softmax_table(sides[0][0], alpha)
    if table is not None:
        tab = table
    if unsigned == ALL_UNSIGNED or (unsigned[1] and unsigned[2]):
        return tab, tuple(sides)
    s = lsq_bmm_w8_q(q, k, True, *sides[0], mid)
    if not unsigned[1]:
        sides[1] = A.fit_quantizer(lsq_softmax_w8(s, tab, F32), False)
    if not unsigned[2]:
        p = lsq_softmax_w8_q(s, tab, *sides[1], mid)
        sides[2] = A.fit_quantizer(lsq_bmm_w8(p, v, False, F32), False)
    return tab, tuple(sides)


@functools.lru_cache(maxsize=None)
def case(B, H, Tq, Tk, D, seed=0, dtypes=ALL_U8, unsigned=ALL_UNSIGNED, mid=BF16, zeros=(A.QKV_Z,) * 3, table=None):
    """`table`: None (of the scores' scale), "full" (`attn_w8_cases.full_table`) or "zeros" (`table_with_zeros`)"""
    c = Case()
    c.shape = (B, H, Tq, Tk, D)
    c.q, c.k, c.v = inputs(B, H, Tq, Tk, D, seed, dtypes, zeros)
    c.mid = mid
    given = {None: None, "full": A.full_table(), "zeros": A.table_with_zeros()}[table]
    c.table, c.sides = fitted_sides(c.q, c.k, c.v, unsigned, mid, given)
    c.s, c.p, c.want = definition(c.q, c.k, c.v, c.table, c.sides, mid)
    return c


def finish(c):
    """the definition of a case whose operands a test built or changed by hand"""
    c.s, c.p, c.want = definition(c.q, c.k, c.v, c.table, c.sides, c.mid)
    return c


def check_not_degenerate(c):
    """for Tk >= 16: more than 16 distinct output levels and more than 8 distinct probability levels"""
    assert c.shape[3] < 16 or (len(c.want.unique()) > 16 and len(c.p.unique()) > 8), \
        (c.shape, len(c.s.unique()), len(c.p.unique()), len(c.want.unique()))


def moved(x, dev, shift=0):
    """a LevelsTensor on `dev`: its whole storage copied (strides kept), `shift` bytes off the allocation's base"""
    from torchlsq.functional import LevelsTensor
    lv = x.levels if str(dev) == "cpu" else A.place(x.levels, dev, shift)
    return LevelsTensor(lv, x.scale.to(dev), x.zero_point.to(dev), x.quant_min, x.quant_max, x.type_min, x.type_max)


def sides_on(sides, dev):
    return tuple(A.to(dev, s) for s in sides)


def run(c, dev, shift=(0, 0, 0)):
    """`lsq_attention_w8_q` of the case on `dev` -> the levels [B, Tq, H D]"""
    from torchlsq.functional import lsq_attention_w8_q
    q, k, v = (moved(x, dev, sh) for x, sh in zip((c.q, c.k, c.v), shift))
    return lsq_attention_w8_q(q, k, v, c.table.to(dev), *sides_on(c.sides, dev), c.mid).levels


def flat_args(c, dev, shift=(0, 0, 0)):
    """the arguments of torch.ops.torchlsq.lsq_attention_w8_q8_q / extension.attn_fused_w8_q for the case on `dev`"""
    q, k, v = (moved(x, dev, sh) for x, sh in zip((c.q, c.k, c.v), shift))
    sides = sides_on(c.sides, dev)
    return (q.levels, q.scale, q.zero_point, k.levels, k.scale, k.zero_point, v.levels, v.scale, v.zero_point, c.table.to(dev),
            *sides[0], *sides[1], *sides[2], c.mid)


def c_entry(c, dev, shift=(0, 0, 0)):
    """`lsq_attn_fused_w8` of liblsq_hip_attn_fused_w8.so called directly on the case's operands on `dev`: no Python host, so no
    fallback -> (status, the levels [B, Tq, H D], prefilled with 0x5A)"""
    import ctypes
    from torchlsq import extension as E
    from torchlsq._attn_w8_host import _DTYPE_CODE, _LEVEL_CODE
    from torchlsq.functional import _act_constants
    B, H, Tq, Tk, D = c.shape
    q, k, v = (moved(x, dev, sh) for x, sh in zip((c.q, c.k, c.v), shift))
    sides, tab = sides_on(c.sides, dev), c.table.to(dev)
    y = torch.full((B, Tq, H * D), 0x5A, dtype=U8, device=dev).view(c.want.dtype)
    S = E.LsqAttnW8Strides
    geom = E.LsqAttnFusedW8Geom(B, H, Tq, Tk, D, *(_LEVEL_CODE[x.levels.dtype] for x in (q, k, v)),
                                *(S(*strides(x.levels)) for x in (q, k, v)), S(*strides(y.view(B, Tq, H, D).permute(0, 2, 1, 3))))
    p_s, p_z = _act_constants(sides[1][0], sides[1][1], sides[1][4], sides[1][5])
    consts = E.LsqAttnFusedW8Consts(q.scale.data_ptr(), q.zero_point.data_ptr(), k.scale.data_ptr(), k.zero_point.data_ptr(),
                                    v.scale.data_ptr(), v.zero_point.data_ptr(), p_s.data_ptr(), p_z.data_ptr())
    outs = [E.LsqAttnW8Out(s[0].data_ptr(), s[1].data_ptr(), *s[2:], _DTYPE_CODE[c.mid]) for s in sides]
    torch.cuda.synchronize()                            # the call below goes to the default stream
    rc = E.attn_fused_w8_library().lsq_attn_fused_w8(ctypes.byref(geom), ctypes.byref(consts), *(ctypes.byref(o) for o in outs),
                                                     tab.data_ptr(), q.levels.data_ptr(), k.levels.data_ptr(), v.levels.data_ptr(),
                                                     y.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, y


def strides(t):
    from torchlsq._attn_w8_host import _strides4
    s = _strides4(t)
    return (s.s0, s.s1, s.ld)


def plan_of(c, qkv_aligned=True, y_aligned=True, y_strides=None, overrides=()):
    """the plan for the case's operands as they lie on the CPU (the strides are what `moved` keeps)"""
    from torchlsq import extension as E
    B, H, Tq, Tk, D = c.shape
    st = dict(q_strides=strides(c.q.levels), k_strides=strides(c.k.levels), v_strides=strides(c.v.levels), y_strides=y_strides)
    st.update(dict(overrides))
    return E.attn_fused_w8_plan(B, H, Tq, Tk, D, qkv_aligned=qkv_aligned, y_aligned=y_aligned, q_dtype=c.q.levels.dtype,
                                k_dtype=c.k.levels.dtype, v_dtype=c.v.levels.dtype, **st)
