"""The checks of a `lsq_attn_decode_w8_geom` are ONE text (csrc/attn_w8/lsq_attn_decode_checks.hpp) for the four libraries that take
one: the `*_plan` entries of decode, prefill and split refuse an illegal geometry with the same message once the entry's name is
stripped, and the paged plan -- the same geometry on legal pages -- says the same wherever it does not word a refusal its own way
(D alone has a limit there, k and v are k_pool and v_pool, Tk is the table's capacity).  Host only: no entry reaches the runtime.
"""
import ctypes

import pytest

LSQ_EINVAL = -1
B, H, HKV, TQ, TK, D = 1, 2, 2, 8, 64, 16
NP, PS, MP = 8, 16, 4                                               # Mp ps = Tk


def _geom(E, **kw):
    S = E.LsqAttnW8Strides
    a = dict(B=B, H=H, Hkv=HKV, Tq=TQ, Tk=TK, D=D, dt=(0, 0, 0), causal=0, off=0, q=S(H * TQ * D, TQ * D, D), y=S(H * TQ * D, TQ * D, D),
             k=None, v=None)
    a.update(kw)
    return a


def _dense(E, a):
    kv = E.LsqAttnW8Strides(HKV * TK * D, TK * D, D)               # [B, Hkv, Tk, D]
    return E.LsqAttnDecodeW8Geom(a["B"], a["H"], a["Hkv"], a["Tq"], a["Tk"], a["D"], *a["dt"], a["causal"], a["off"], 0, a["q"], a["k"] or kv,
                                 a["v"] or kv, a["y"])


def _paged(E, a):
    kv = E.LsqAttnW8Strides(HKV * PS * D, PS * D, D)               # [Np, Hkv, ps, D]
    return E.LsqAttnDecodeW8Geom(a["B"], a["H"], a["Hkv"], a["Tq"], a["Tk"], a["D"], *a["dt"], a["causal"], a["off"], 0, a["q"], a["k"] or kv,
                                 a["v"] or kv, a["y"])


# (what is illegal, the common text's mark, what the paged plan says where it words the refusal its own way)
BIG = 1 << 17
CASES = [
    (dict(dt=(0, 2, 0)), "must be LSQ_ATTN_W8_U8 (0) or LSQ_ATTN_W8_I8 (1), got 0, 2 and 0", None),
    (dict(dt=(7, 0, 1)), "got 7, 0 and 1", None),
    (dict(B=0), "every extent must be at least 1", None),
    (dict(Tq=0), "every extent must be at least 1", None),
    (dict(Tk=0), "every extent must be at least 1", None),
    (dict(D=0), "every extent must be at least 1", None),
    (dict(H=3), "H = 3 query heads are not a multiple of Hkv = 2 kv heads", None),
    (dict(causal=1, off=-1), "causal_offset = -1 must be at least 0", None),
    (dict(D=65552, q=(0, 0, BIG), k=(0, 0, BIG), v=(0, 0, BIG), y=(0, 0, BIG)), "D = 65552 and Tk = 64, at most 65536 are served",
     "D = 65552, at most 65536 are served"),
    (dict(Tk=65537), "D = 16 and Tk = 65537, at most 65536 are served", "Tk = 65537 is not the table's capacity Mp ps = 4 x 16"),
    (dict(B=1 << 20), "Tq = 8 and B * H = 1048576 x 2 may each be 2^20 at most", None),
    (dict(Tq=(1 << 20) + 1), "Tq = 1048577 and B * H = 1 x 2 may each be 2^20 at most", None),
    (dict(q=(256, 128, 15)), "q's row stride 15 is smaller than its row of 16", None),
    (dict(k=(512, 256, 15)), "k's row stride 15 is smaller than its row of 16", "k_pool's row stride 15 is smaller than its row of 16"),
    (dict(y=(-16, 128, 16)), "y's batch strides (-16, 128) must not be negative", None),
    (dict(y=(256, 64, 16)), "y's rows or batches overlap each other (strides 256, 64, 16 for [1, 2, 8, 16])", None),
]


@pytest.mark.parametrize("bad,mark,paged_own", CASES, ids=[str(sorted(c[0])) + str(i) for i, c in enumerate(CASES)])
def test_one_text_for_an_illegal_geometry(bad, mark, paged_own):
    from torchlsq import extension as E
    S = E.LsqAttnW8Strides
    a = _geom(E, **{k: (S(*v) if k in "qkvy" else v) for k, v in bad.items()})
    out = (ctypes.c_int32 * 8)()
    dense = _dense(E, a)
    said = []
    for lib, name, extra in ((E.attn_decode_w8_library(), "lsq_attn_decode_w8", ()), (E.attn_prefill_w8_library(), "lsq_attn_prefill_w8", ()),
                             (E.attn_decode_split_w8_library(), "lsq_attn_decode_split_w8", (0,))):
        assert getattr(lib, name + "_plan")(ctypes.byref(dense), 1, 1, *extra, ctypes.byref(out)) == LSQ_EINVAL, name
        msg = getattr(lib, name + "_last_error")().decode()
        assert msg.startswith(name + "_plan: "), msg
        said.append(msg[len(name) + 7:])
    assert said[0] == said[1] == said[2] and mark in said[0], said
    lib = E.attn_paged_w8_library()
    pages = E.LsqAttnPagedW8Pages(NP, PS, MP, MP)
    assert lib.lsq_attn_paged_w8_plan(ctypes.byref(_paged(E, a)), ctypes.byref(pages), 1, 1, 0, ctypes.byref(out)) == LSQ_EINVAL
    msg = lib.lsq_attn_paged_w8_last_error().decode()
    assert msg.startswith("lsq_attn_paged_w8_plan: "), msg
    if paged_own is None:
        assert msg[len("lsq_attn_paged_w8_plan: "):] == said[0]
    else:
        assert paged_own in msg and msg[len("lsq_attn_paged_w8_plan: "):] != said[0]


def test_the_legal_geometry_is_planned_by_all_four():
    from torchlsq import extension as E
    a = _geom(E)
    out = (ctypes.c_int32 * 8)()
    dense = _dense(E, a)
    assert E.attn_decode_w8_library().lsq_attn_decode_w8_plan(ctypes.byref(dense), 1, 1, ctypes.byref(out)) == 0 and out[0] != 0
    assert E.attn_prefill_w8_library().lsq_attn_prefill_w8_plan(ctypes.byref(dense), 1, 1, ctypes.byref(out)) == 0 and out[0] != 0
    assert E.attn_decode_split_w8_library().lsq_attn_decode_split_w8_plan(ctypes.byref(dense), 1, 1, 0, ctypes.byref(out)) == 0 and out[0] == 1
    split = list(out)
    pages = E.LsqAttnPagedW8Pages(NP, PS, MP, MP)
    assert E.attn_paged_w8_library().lsq_attn_paged_w8_plan(ctypes.byref(_paged(E, a)), ctypes.byref(pages), 1, 1, 0, ctypes.byref(out)) == 0
    assert list(out)[1:] == split[1:] and out[0] != 0                # one plan rule: grid, threads, rows, chunk, splits, LDS, store
