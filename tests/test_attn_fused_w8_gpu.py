"""The fused attention core on 8-bit levels on the GPU (liblsq_hip_attn_fused_w8.so): bit for bit against the DEFINITION -- the three
functional calls on the CPU (tests/attn_fused_w8_cases.py; tests/test_attn_w8_cpu.py holds those to plain integers, numpy and float64)
-- and against the three GPU launches, at the smallest shapes at which each mechanism of the kernel can fail.  The plan's family is
asserted before every comparison, and beside the op the library's C entry is called directly on the same operands -- no Python host,
no fallback --, so what is compared is the fused kernel's own output; every comparison is torch.equal; the softmax tables are built
once on the CPU and moved.
"""
import copy
import ctypes
import itertools

import pytest
import torch

import attn_fused_w8_cases as C
import attn_w8_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
GUARD = 0x5A
LSQ_EINVAL = -1


def _fused_equals_cpu(c, note="", family="fused", shift=(0, 0, 0)):
    pl = C.plan_of(c, qkv_aligned=not any(shift))
    assert pl["family"] == family, (note, pl)
    C.check_not_degenerate(c)
    got = C.run(c, DEV, shift)
    assert got.shape == c.want.shape and got.dtype == c.want.dtype, note
    assert torch.equal(got.cpu(), c.want), note
    # the library's entry called directly: there is no fallback behind it, so status 0 and these bytes are the fused kernel's own
    rc, y = C.c_entry(c, DEV, shift)
    if family == "fused":
        assert rc == 0 and torch.equal(y.cpu(), c.want), (note, rc)
    else:
        assert rc == LSQ_EINVAL and bool((y.view(U8) == GUARD).all()), (note, rc)
    return pl


# both sides of the row tile and of the K step (63, 64, 65); ViT's 197: a partial packet, a partial row tile; D = 80: a partial K
# step in phase 1 and five column sub-tiles in phase 3; 1024: LDS above 64 KB; 2048 x 128: the largest LDS
SHAPES = [(1, 1, 1, 16), (1, 2, 16, 16), (2, 3, 19, 32), (1, 2, 63, 64), (1, 2, 64, 64), (1, 2, 65, 64), (2, 3, 197, 64), (1, 1, 130, 80),
          (1, 1, 257, 128), (1, 1, 1024, 64), (1, 1, 2048, 128)]


@pytest.mark.parametrize("combo", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_fused_equals_the_cpu_definition(shape, combo):
    B, H, T, D = shape
    dtypes, unsigned = C.COMBOS[combo]
    pl = _fused_equals_cpu(C.case(B, H, T, T, D, 0, dtypes, unsigned), (shape, combo))
    assert pl["grid"] == B * H * ((T + 63) // 64) and pl["lds_bytes"] <= 163840 and pl["lds_dynamic"] == (pl["lds_bytes"] > 65536)
    assert (T < 1024) == (not pl["lds_dynamic"])


@pytest.mark.parametrize("mid", A.MIDS, ids=str)
def test_every_dtype_combination_at_65(mid):
    every = list(itertools.product((U8, I8), repeat=3))
    for dtypes in every:
        for unsigned in itertools.product((True, False), repeat=3):
            _fused_equals_cpu(C.case(1, 2, 65, 65, 64, 1, dtypes, unsigned, mid), (dtypes, unsigned, mid))


@pytest.mark.parametrize("shape", [(1, 2, 5, 197, 64), (1, 1, 130, 33, 32)], ids=str)
def test_tq_differs_from_tk(shape):
    for dtypes, unsigned in C.COMBOS:
        _fused_equals_cpu(C.case(*shape, 2, dtypes, unsigned), shape)


def test_fused_equals_the_three_gpu_launches_and_the_cpu_module():
    core, qkv, want = A.core_case(2, 3, 197, 64)
    three = copy.deepcopy(core).to(DEV)
    fused = copy.deepcopy(three)
    fused.fused = True
    assert list(fused.state_dict()) == list(core.state_dict()) and "fused=True" in repr(fused) and "fused=False" in repr(three)
    heads = A.qkv_heads(qkv.to(DEV), DEV)
    a, b = three(*heads), fused(*heads)
    assert len(want.levels.unique()) > 16
    assert torch.equal(a.levels, b.levels) and torch.equal(b.levels.cpu(), want.levels)
    assert torch.equal(b.scale.cpu(), want.scale) and torch.equal(b.zero_point.cpu(), want.zero_point)
    assert (b.quant_min, b.quant_max, b.type_min, b.type_max) == (want.quant_min, want.quant_max, want.type_min, want.type_max)


def test_row_sums_beyond_32_bits_and_zero_entries():
    # every entry 2^24: S = 2^35 at Tk = 2048, every probability 2^-11 (one level by definition; the fitted int8 sides keep the
    # context's levels apart)
    c = C.case(1, 1, 64, 2048, 64, 3, C.ALL_U8, (True, False, False), BF16, (A.QKV_Z,) * 3, "full")
    assert len(c.p.unique()) == 1 and len(c.want.unique()) > 16
    assert C.plan_of(c)["family"] == "fused"
    assert torch.equal(C.run(c, DEV).cpu(), c.want)
    # rows of equal scores (q at its zero point: every product is 0) among ordinary ones, with the ordinary table
    c = C.Case()
    c.shape, c.mid = (1, 1, 64, 2048, 64), BF16
    c.q, c.k, c.v = C.inputs(*c.shape, 4)
    c.q.levels[:, :, 1::3] = A.QKV_Z
    c.table, c.sides = C.fitted_sides(c.q, c.k, c.v, C.ALL_UNSIGNED, BF16)
    C.finish(c)
    assert len(c.s[0, 0, 1].unique()) == 1 and len(c.s[0, 0, 0].unique()) > 8
    _fused_equals_cpu(c, "equal scores")
    # a table whose tail is 0: entries that add nothing to S
    _fused_equals_cpu(C.case(1, 2, 197, 197, 64, 5, C.ALL_U8, C.ALL_UNSIGNED, BF16, (A.QKV_Z,) * 3, "zeros"), "zeros in the table")


def test_zero_points_far_from_the_middle():
    for dtypes in (C.ALL_U8, (I8, I8, I8), (U8, I8, U8)):
        _fused_equals_cpu(C.case(1, 2, 65, 65, 64, 6, dtypes, C.ALL_UNSIGNED, BF16, (3, 140, 250)), dtypes)


def test_stale_lds_between_launches():
    """LDS is not zeroed between workgroups: a long row's bytes lie behind a shorter row's of the next launch"""
    for T in (256, 197, 1):
        _fused_equals_cpu(C.case(1, 2, T, T, 64, 7), T)


def _host_call(c, out, shift=(0, 0, 0)):
    from torchlsq import extension as E
    return E.attn_fused_w8_q(*C.flat_args(c, DEV, shift), out=out)


def test_output_placement():
    c = C.case(2, 3, 19, 19, 32, 8)
    B, H, T, _, D = c.shape
    # y through the [B, H, T, D] view of a [B, T, H D] region inside a larger buffer of guard bytes, rows 16 bytes longer than H D
    big = torch.full((B, T + 2, H * D + 16), GUARD, dtype=U8, device=DEV)
    yv = big[:, 1:T + 1, :H * D].view(B, T, H, D).permute(0, 2, 1, 3)
    assert C.plan_of(c, y_strides=C.strides(yv))["store"] == "packets"
    _host_call(c, yv)
    assert torch.equal(big[:, 1:T + 1, :H * D].cpu(), c.want)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, 1:T + 1, :H * D] = False
    assert bool((big[mask] == GUARD).all()), "bytes outside the logical y were written"
    # a y one byte off: still the fused kernel, with the byte store
    raw = torch.full((B * T * H * D + 2,), GUARD, dtype=U8, device=DEV)
    yv = raw[1:-1].view(B, T, H, D).permute(0, 2, 1, 3)
    pl = C.plan_of(c, y_aligned=False)
    assert pl["family"] == "fused" and pl["store"] == "elements" and yv.data_ptr() % 16 == 1
    _host_call(c, yv)
    assert torch.equal(raw[1:-1].view(B, T, H * D).cpu(), c.want) and int(raw[0]) == GUARD and int(raw[-1]) == GUARD
    # a q one byte off: the three launches, the same bytes
    _fused_equals_cpu(c, "q one byte off", "three_launches", (1, 0, 0))
    # a k whose rows lie 197 bytes apart: the three launches, the same bytes
    d = C.Case()
    d.shape, d.mid, d.table, d.sides = c.shape, c.mid, c.table, c.sides
    d.q, d.v = c.q, c.v
    d.k = C.level_tensor(A.padded(c.k.levels.contiguous(), 197), A.QKV_Z)
    assert d.k.levels.stride(-2) == 197
    C.finish(d)
    assert torch.equal(d.want, c.want)
    _fused_equals_cpu(d, "rows 197 apart", "three_launches")


def test_launches_repeat_and_rows_depend_on_their_own_inputs_alone():
    c = C.case(2, 3, 197, 197, 64, 9)
    first, second = C.run(c, DEV), C.run(c, DEV)
    assert torch.equal(first, second) and torch.equal(first.cpu(), c.want)
    # the (b, h) slice of the batched call is the call on that slice alone
    from torchlsq.functional import LevelsTensor, lsq_attention_w8_q

    def cut(x, f):
        x = C.moved(x, DEV)
        return LevelsTensor(f(x.levels), x.scale, x.zero_point, x.quant_min, x.quant_max, x.type_min, x.type_max)

    sides, tab = C.sides_on(c.sides, DEV), c.table.to(DEV)
    b, h, D = 1, 2, 64
    one = lsq_attention_w8_q(*(cut(x, lambda t: t[b:b + 1, h:h + 1]) for x in (c.q, c.k, c.v)), tab, *sides, c.mid).levels
    assert torch.equal(one[0], first[b, :, h * D:(h + 1) * D])
    # the first 5 rows of the Tq = 197 call are the Tq = 5 call
    q5 = cut(c.q, lambda t: t[:, :, :5])
    five = lsq_attention_w8_q(q5, C.moved(c.k, DEV), C.moved(c.v, DEV), tab, *sides, c.mid).levels
    assert five.shape == (2, 5, 192) and torch.equal(five, first[:, :5])


def test_c_entry_refuses_an_unserved_geometry_and_writes_nothing():
    from torchlsq import extension as E
    lib = E.attn_fused_w8_library()
    B, H, T, D = 1, 2, 19, 24                          # D is not a multiple of 16: legal, three launches
    assert E.attn_fused_w8_plan(B, H, T, T, D)["family"] == "three_launches"
    qkv = A.levels((B, T, 3, H, D), 0, U8).to(DEV)
    y = torch.full((B, T, H * D), GUARD, dtype=U8, device=DEV)
    st = E.LsqAttnW8Strides(T * 3 * H * D, D, 3 * H * D)
    geom = E.LsqAttnFusedW8Geom(B, H, T, T, D, 0, 0, 0, st, st, st, E.LsqAttnW8Strides(T * H * D, D, H * D))
    s, z = A.one(0.03).to(DEV), A.one(125, torch.int32).to(DEV)
    consts = E.LsqAttnFusedW8Consts(*([s.data_ptr(), z.data_ptr()] * 4))
    sc, sh = A.one(1.0 / 255).to(DEV), A.one(0.0).to(DEV)
    side = E.LsqAttnW8Out(sc.data_ptr(), sh.data_ptr(), 0, 255, 0, 255, 0)
    tab = A.table().to(DEV)
    p = [qkv[:, :, i].data_ptr() for i in range(3)]
    rc = lib.lsq_attn_fused_w8(ctypes.byref(geom), ctypes.byref(consts), ctypes.byref(side), ctypes.byref(side), ctypes.byref(side),
                               tab.data_ptr(), p[0], p[1], p[2], y.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == LSQ_EINVAL and b"not served by the fused kernel" in lib.lsq_attn_fused_w8_last_error()
    assert bool((y == GUARD).all())


def test_fused_core_replays_in_a_graph():
    core, qkv, want = A.core_case(2, 3, 197, 64)
    qkv2 = A.levels(qkv.shape, 99, U8)
    want2 = core(*A.qkv_heads(qkv2)).levels
    assert not torch.equal(want.levels, want2)
    gpu = copy.deepcopy(core).to(DEV)
    gpu.fused = True
    static = qkv.to(DEV)
    heads = A.qkv_heads(static, DEV)
    assert torch.equal(gpu(*heads).levels.cpu(), want.levels)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gpu(*heads)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gpu(*heads).levels
    graph.replay()
    assert torch.equal(out.cpu(), want.levels)
    static.copy_(qkv2)
    graph.replay()
    assert torch.equal(out.cpu(), want2)


def test_smoke_runs_the_fused_step(capsys):
    import __graft_entry__ as G
    G.smoke()
    assert "fused attention core" in capsys.readouterr().out
