"""liblsq_hip_linmid_w4.so on the GPU: every byte against the plain reference of tests/test_lindec_w4_cpu.py on exact inputs, and
against the existing GPU ops composed on random ones -- the order-of-sum contract of include/lsq_hip_linmid_w4.h."""
import pytest
import torch

import test_lindec_w4_cpu as C
import test_linglu_w4_cpu as G
import test_linrope_w4_cpu as R
from test_lindec_w4_cpu import BF16, NONE, PRE, U8
from test_lindec_w4_gpu import composed
from test_linmid_w4_cpu import CASES
from torchlsq import _lindec_w4_host, _linmid_w4_host, extension as E, functional as F
from w8_routes import entered

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("spec", CASES, ids=C.ident)
def test_kernel_equals_the_plain_reference_on_exact_inputs(spec):
    c = C.case(*spec)
    assert E.linmid_w4_plan(*spec[:5])["served"]
    with entered(_linmid_w4_host) as calls:
        got = C.run(c, DEV, decode=True)
    assert calls == ["lsq_linmid_w4_linear_levels"]
    assert got.dtype == c["want"].dtype and torch.equal(got.cpu(), c["want"])


@pytest.mark.parametrize("spec", CASES, ids=C.ident)
@pytest.mark.parametrize("seed", [2, 7], ids=["near_zero_points", "far_zero_points"])      # odd: wide_packed's 70000, the 64-bit I
def test_kernel_equals_the_composition_on_random_inputs(spec, seed):
    c = C.case(*spec[:11], exact=False, seed=seed)
    M = spec[0]
    want = composed(c)
    assert len(want.unique()) > min(8, want.numel() // 4), "a vacuous case"
    got = C.run(c, DEV, decode=True)
    assert torch.equal(got, want) and torch.equal(C.run(c, DEV, decode=True), got)         # ... and launches repeat
    lx, s_x, zx, p, bias, out, relu, mid, res = c["args"]
    for m0 in range(0, M, 16):                          # every 16-row block is the <= 16-row call: row m does not depend on M
        part = dict(args=(lx[m0:m0 + 16], s_x, zx, p, bias, out, relu, mid, None if res is None else (res[0][m0:m0 + 16],) + res[1:]))
        assert torch.equal(C.run(part, DEV, decode=True), got[m0:m0 + 16])
    assert torch.equal(C.run(c, DEV, decode=True, M=1), got[:1])


@pytest.mark.parametrize("rows, decode, codes_offset, mid, dec", [(17, True, 0, 1, 0), (64, True, 0, 1, 0), (100, True, 0, 1, 0),
                                                                  (100, False, 0, 0, 0), (64, True, 1, 0, 0), (16, True, 0, 0, 1)])
def test_route(rows, decode, codes_offset, mid, dec):
    """which library a call enters: one launch at 17 to 64 rows, ceil(M / 64) block launches beyond, none without `decode`, with
    misaligned codes or at 16 rows -- and the same bytes on every route"""
    c = C.case(rows, 40, 2176, 128, 4, U8, True, BF16, False, PRE, U8, exact=False, seed=5)
    lx, s_x, zx, p, bias, out, relu, md, res = c["args"]
    shifted = torch.zeros(p.codes.numel() + 16, dtype=U8, device=DEV)[codes_offset:codes_offset + p.codes.numel()].view(p.codes.shape)
    shifted.copy_(p.codes)
    q = F.PackedGroupTensor(shifted, p.scale.to(DEV), p.zero_point.to(DEV), p.bits, p.group_size, p.quant_min, p.shape)
    with entered(_linmid_w4_host) as m_calls, entered(_lindec_w4_host) as d_calls:
        got = C.run(dict(args=(lx, s_x, zx, q, bias, out, relu, md, res)), DEV, decode=decode)
    assert m_calls == ["lsq_linmid_w4_linear_levels"] * (mid * -(-rows // 64)) and d_calls == ["lsq_lindec_w4_linear_levels"] * dec
    assert torch.equal(got, composed(c))


@pytest.mark.parametrize("shape, mid, dec", [((17, 40, 2176, 128, 4), 1, 0), ((32, 40, 2176, 128, 4), 0, 2), ((64, 40, 2176, 128, 4), 1, 0),
                                             ((100, 40, 2176, 128, 4), 2, 0), ((33, 32, 4224, 32, 4), 0, 3), ((64, 4128, 128, 128, 4), 0, 4)])
def test_decode_none_takes_the_measured_route(monkeypatch, shape, mid, dec):
    """with the default on, `decode=None` takes the new kernel where a workgroup stages x once (one chunk; one tile per workgroup, or
    resident x and a second block at most half full) and the 16-row launches elsewhere: 32 rows, two chunks, more tiles than CUs"""
    monkeypatch.setattr(F, "W4A8_MID_DEFAULT", True)
    c = C.case(*shape, U8, True, BF16, False, PRE, U8, exact=False, seed=5)
    with entered(_linmid_w4_host) as m_calls, entered(_lindec_w4_host) as d_calls:
        got = C.run(c, DEV, decode=None)
    assert (len(m_calls), len(d_calls)) == (mid, dec) and torch.equal(got, composed(c))


@pytest.mark.parametrize("mid_default, launches", [(False, 0), (True, 1)])
def test_the_glu_and_rotary_fallbacks_follow_the_default(monkeypatch, mid_default, launches):
    """the ops with an epilogue compose these linears beyond 16 rows: nobody passed `decode`, so `W4A8_MID_DEFAULT` decides"""
    monkeypatch.setattr(F, "W4A8_MID_DEFAULT", mid_default)
    to = lambda t: t.to(DEV) if isinstance(t, torch.Tensor) else t
    c = G.case(20, 16, 128, 128, 4, exact=False, seed=2)
    w = [(p.codes, p.scale.reshape(-1), p.zero_point.reshape(-1), b, o[0], o[1], *o[2]) for p, b, o in zip(c["packed"], c["biases"], c["outs"])]
    g = c["glu"]
    args = (c["lx"], c["s_x"], c["zx"], *w[0], *w[1], c["packed"][0].group_size, c["packed"][0].bits, g["s_u"], g["z_u"], c["table"],
            g["osc"], g["osh"], *g["rng"], c["mid"])
    with entered(_linmid_w4_host) as calls:
        got = torch.ops.torchlsq.lsq_linear_packed_q8_glu_q(*map(to, args))         # (two code buffers: a gate and an up linear)
    assert len(calls) == 2 * launches and torch.equal(got, G.run(c, DEV, glu_epilogue=False, decode=False))
    r = R.case(20, 1, 1, 1, 32, 32, 128, 128, 4, exact=False, seed=2)
    with entered(_linmid_w4_host) as calls:
        rq, kc, vc, _, _ = R.call(r, DEV)
    assert len(calls) == launches
    monkeypatch.setattr(F, "W4A8_MID_DEFAULT", not mid_default)         # the other route: the same bytes
    rq2, kc2, vc2, _, _ = R.call(r, DEV)
    assert torch.equal(rq, rq2) and torch.equal(kc, kc2) and torch.equal(vc, vc2)


@pytest.mark.parametrize("spec", [CASES[8 + 1], CASES[16 + 2], CASES[40 + 4], CASES[48 + 7]], ids=C.ident)
def test_byte_offsets_and_untouched_surroundings(spec):
    """y and the residual at byte offset 1 (the byte paths); a poisoned y keeps every byte outside its M * N"""
    c = C.case(*spec)
    M, N = c["want"].shape
    lx, s_x, zx, p, bias, (osc, osh, rng), relu, mid, res = c["args"]
    g = lambda t: None if t is None else t.to(DEV)
    buf = torch.full((M * N + 64,), 0x5A, dtype=c["want"].dtype, device=DEV)
    y = buf[1:1 + M * N].view(M, N)
    w = (g(p.codes), g(p.scale.reshape(-1)), g(p.zero_point.reshape(-1)), g(bias), p.group_size, p.bits)
    args = (g(lx), g(s_x), g(zx), *w, g(osc), g(osh), *rng, relu, mid)
    with entered(_linmid_w4_host) as calls:
        if res is None:
            E.lindec_w4_linear_levels(*args, out=y)
        else:
            rbuf = torch.zeros(M * N + 16, dtype=res[0].dtype, device=DEV)
            rbuf[1:1 + M * N] = g(res[0]).flatten()
            E.lindec_w4_linear_levels_add(*args, rbuf[1:1 + M * N].view(M, N), g(res[1]), g(res[2]), g(res[3]), g(res[4]), *res[5], out=y)
    assert calls == ["lsq_linmid_w4_linear_levels"] and torch.equal(y.cpu(), c["want"])
    assert bool((buf[:1] == 0x5A).all()) and bool((buf[1 + M * N:] == 0x5A).all())


def test_two_modules_in_a_captured_graph():
    """PackedLinearA8Q -> PackedLinearA8AddQ at 33 rows, decode=True: several replays against the eager composition"""
    from torchlsq.quantized import PackedLinearA8AddQ, PackedLinearA8Q
    a, b = C.case(33, 64, 256, 128, 4, U8, True, BF16, True, NONE, U8, exact=False, seed=2), \
        C.case(33, 32, 64, 32, 4, U8, True, BF16, False, PRE, U8, exact=False, seed=4)
    mods = []
    for cls, c in ((PackedLinearA8Q, a), (PackedLinearA8AddQ, b)):
        _, _, _, p, bias, (osc, osh, rng), relu, mid, res = c["args"]
        m = cls(p.shape[1], p.shape[0], p.bits, p.group_size, p.quant_min, bias=True, output_range=rng, relu=relu, mid_dtype=mid)
        m.codes, m.scale, m.zero_point, m.output_scale, m.output_shift = p.codes.reshape(p.shape[0], -1), p.scale, p.zero_point, osc, osh
        with torch.no_grad():
            m.bias.copy_(bias)
        if res is not None:
            m.pre_scale, m.pre_shift, m.pre_range = res[3], res[4], res[5]
        m.decode = True
        mods.append(m.to(DEV))
    lx, s_x, zx = a["args"][:3]
    res = b["args"][8]
    x = F.LevelsTensor(lx.to(DEV), s_x.to(DEV), zx.to(DEV), 0, 255)
    r = F.LevelsTensor(res[0].to(DEV), res[1].to(DEV), res[2].to(DEV), 0, 255)
    chain = lambda: mods[1](mods[0](x), r).levels
    h = mods[0](x)
    assert torch.equal(h.levels, C.run(a, DEV, decode=False))
    want = C.run(dict(args=(h.levels.cpu(), h.scale.cpu(), h.zero_point.cpu()) + b["args"][3:]), DEV, decode=False)
    with entered(_linmid_w4_host) as calls:
        assert torch.equal(chain(), want) and len(want.unique()) > 8
    assert calls == ["lsq_linmid_w4_linear_levels"] * 2
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = chain()
    for _ in range(3):
        got.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
