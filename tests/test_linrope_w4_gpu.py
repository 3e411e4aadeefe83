"""liblsq_hip_linrope_w4.so on the GPU: every byte against the plain reference of tests/test_linrope_w4_cpu.py, against the existing
GPU ops composed on the same operands and against a second launch.  No tolerance anywhere."""
import copy

import pytest
import torch

import test_linrope_w4_cpu as C
from test_linrope_w4_cpu import FILL, P, TMAX
from torchlsq import extension as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS = torch.ops.torchlsq


def plan_of(c, K, Gs, bits, **kw):
    B, T, H, Hkv, D = c["dims"]
    where = dict(pages=(c["shape"][0], c["ps"], TMAX // c["ps"])) if c["ps"] else dict(Tmax=TMAX)
    return E.linrope_w4_plan(B, T, H, Hkv, D, K, Gs, bits, R=2 * c["cos"].shape[1], P=P, **where, **kw)


def composed(*a, out):
    """the existing GPU ops, one after the other: the packed levels-out linear, the rotation of q, and the dense or paged append"""
    qkv = OPS.lsq_linear_packed_q8_q(*a[:15], False, a[25], True)
    B, T, H, Hkv = a[0].shape[0], a[0].shape[1], a[26], a[27]
    qkv = qkv.view(B, T, H + 2 * Hkv, -1)
    q, k, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
    rot = (*a[15:25], a[25], a[30], False)          # s_q, z_q, cos, sin, the rotation's quantizer, mid_dtype, positions, half style
    rq = E.rope_w8_q(q, *rot, out=out)
    if a[31] is None:
        E.rope_w8_q(k, *rot, out=a[28].permute(0, 2, 1, 3), scatter=True)
        E.rope_w8_kv_copy(v, a[29].permute(0, 2, 1, 3), a[30], True)
    else:
        E.kv_append_paged_w8(E.rope_w8_q(k, *rot), v, a[28], a[29], a[31], a[30])
    return rq


@pytest.mark.parametrize("spec", C.CASES, ids=C.ident)
def test_bytes_equal_the_plain_reference(spec):
    c = C.case(*spec)
    assert plan_of(c, *spec[6:9])["served"]
    got, again = C.call(c, DEV), C.call(c, DEV)
    torch.cuda.synchronize()
    for g, a, w in zip(got[:3], again[:3], c["want"]):
        assert torch.equal(g.cpu(), w) and torch.equal(g, a)        # skipped rows and untouched pages keep FILL
    assert all(bool((t == FILL).all()) for t in got[3])


@pytest.mark.parametrize("seed", [2, 7], ids=["near zero points", "far zero points"])
@pytest.mark.parametrize("spec", [C.CASES[1], C.CASES[2], C.CASES[5]], ids=C.ident)
def test_random_inputs_equal_the_existing_ops_composed(spec, seed):
    c = C.case(*spec, exact=False, seed=seed)
    assert plan_of(c, *spec[6:9])["served"]
    got, old, again = C.call(c, DEV), C.call(c, DEV, fn=composed), C.call(c, DEV)
    off = C.call(c, DEV, fn=lambda *a, out: (OPS.lsq_linear_packed_q8_rope_q(*a), out)[0])      # the op: the caches
    torch.cuda.synchronize()
    assert len(got[0].unique()) > 16
    for g, o, a in zip(got[:3], old[:3], again[:3]):
        assert torch.equal(g, o) and torch.equal(g, a)
    assert torch.equal(off[1], got[1]) and torch.equal(off[2], got[2])
    assert all(bool((t == FILL).all()) for run in (got, old) for t in run[3])
    # the functional with rope_epilogue=False: the same caches and the same rq
    from torchlsq import functional as F
    B, T, H, Hkv, D = c["dims"]
    a, (_, kc, vc), _ = C.call(c, DEV)[4]
    x = F.LevelsTensor(a[0], a[1], a[2], 0, 255)
    pk = F.PackedGroupTensor(*(t.to(DEV) for t in (c["packed"].codes, c["packed"].scale, c["packed"].zero_point)), c["packed"].bits,
                             c["packed"].group_size, c["packed"].quant_min, c["packed"].shape)
    outs = []
    for flag in (True, False):
        kc.fill_(FILL), vc.fill_(FILL)
        rq, kl, vl = F.lsq_qkv_rope_append_packed_a8_q(x, pk, a[17], a[18], (a[9], a[10], *a[11:15]), (a[19], a[20], *a[21:25]), H, Hkv, kc, vc,
                                                       a[30], a[31], bias=a[6], mid_dtype=a[25], rope_epilogue=flag)
        written = torch.tensor([[0 <= int(c["pos"][b]) + t < P for t in range(T)] for b in range(B)], device=DEV)
        outs.append((rq.levels[written].clone(), kl.levels.clone(), vl.levels.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*outs)) and torch.equal(outs[0][1], got[1])


@pytest.mark.parametrize("spec", [C.CASES[4], C.CASES[1]], ids=["dense", "paged"])
def test_one_row_alone_writes_that_row(spec):
    c = C.case(*spec)
    for b, t in ((0, 0), (1, 1)):             # a row that is skipped everywhere, and one that is written
        C.assert_row(c, DEV, b, t)


@pytest.mark.parametrize("layout", ["rq_in_qkv", "token_major"])
def test_strided_destinations_keep_their_surroundings(layout):
    c = C.case(*C.CASES[4])
    got = C.call(c, DEV, layout=layout)
    torch.cuda.synchronize()
    rq, kc, vc = got[4][1]
    assert (layout == "rq_in_qkv" and rq.stride(1) == 6 * 64) or (layout == "token_major" and kc.stride(2) == 2 * 64)
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got[:3], c["want"])) and all(bool((t == FILL).all()) for t in got[3])


def test_seventeen_rows_are_composed_with_the_bits_of_two_calls():
    spec = (17, 1, 2, 1, 32, 32, 512, 128, 4)
    c = C.case(*spec, exact=False, seed=2)
    assert not plan_of(c, *spec[6:9])["served"]
    a, (rq, kc, vc), _ = C.call(c, DEV)[4]
    parts = []
    for lo, hi in ((0, 16), (16, 17)):
        k2, v2 = torch.full_like(kc[lo:hi], FILL), torch.full_like(vc[lo:hi], FILL)
        parts.append((E.linrope_w4_q(a[0][lo:hi], *a[1:28], k2, v2, a[30][lo:hi], None), k2, v2))
    torch.cuda.synchronize()
    written = ((c["pos"] >= 0) & (c["pos"] < P)).to(DEV)
    for i, whole in enumerate((rq, kc, vc)):
        both = torch.cat([p[i] for p in parts])
        assert torch.equal(whole[written], both[written]) if i == 0 else torch.equal(whole, both)


@pytest.mark.parametrize("route", ["dense", "paged"])
def test_the_module_in_a_captured_graph(route):
    from torchlsq import functional as F
    c = C.case(*C.CASES[4])
    m, cache = C.module(c, route, True, DEV)
    s_x, zx = (t.to(DEV) for t in c["lin"][:2])
    x = F.LevelsTensor(c["x"][:, 1:2].contiguous().to(DEV), s_x, zx, 0, 255)
    with torch.no_grad():
        m(F.LevelsTensor(c["x"][:, :1].contiguous().to(DEV), s_x, zx, 0, 255), cache)      # the prompt; the LDS opt-in is not captured
        start = copy.deepcopy(cache)
        want = [t.levels.clone() if hasattr(t, "levels") else t.clone() for t in m(x, copy.deepcopy(start))]
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                got = m(x, cache)
            for _ in range(3):
                for mine, saved in zip(cache.buffers(), start.buffers()):
                    mine.copy_(saved)
                graph.replay()
                torch.cuda.synchronize()
                assert all(torch.equal(g.levels if hasattr(g, "levels") else g, w) for g, w in zip(got, want))
    assert want[3].tolist() == [2, 2] and len(want[0].unique()) > 16
