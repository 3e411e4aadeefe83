"""liblsq_hip_linglu_w4.so on the GPU: every byte against the plain reference of tests/test_linglu_w4_cpu.py on exact inputs, and
against the existing GPU ops composed on random ones -- the contract of include/lsq_hip_linglu_w4.h."""
import pytest
import torch

import test_linglu_w4_cpu as C
from torchlsq import extension as E, functional as F

pytestmark = pytest.mark.gpu
OPS = torch.ops.torchlsq
DEV = "cuda"


def composed(c, M=None):
    """the definition written out from the existing GPU ops: the packed levels-out linear per projection (never the decode library),
    then the gated product"""
    g = lambda t: None if t is None else t.to(DEV)
    lv = []
    for p, b, (osc, osh, rng) in zip(c["packed"], c["biases"], c["outs"]):
        lv.append(OPS.lsq_linear_packed_q8_q(g(c["lx"][:M]), g(c["s_x"]), g(c["zx"]), g(p.codes), g(p.scale.reshape(-1)),
                                             g(p.zero_point.reshape(-1)), g(b), p.group_size, p.bits, g(osc), g(osh), *rng, False, c["mid"], False))
    osc, osh, rng = c["out"]
    return OPS.lsq_glu_w8_q8_q(lv[0], lv[1], g(c["glu"]["s_u"]), g(c["glu"]["z_u"]), g(c["table"]), g(osc), g(osh), *rng, c["mid"])


@pytest.mark.parametrize("spec", C.CASES, ids=C.L.ident)
def test_kernel_equals_the_plain_reference_on_exact_inputs(spec):
    c = C.case(*spec)
    assert E.linglu_w4_plan(*spec[:5])["served"]
    got = C.run(c, DEV, glu_epilogue=True)
    assert torch.equal(got.cpu().to(torch.int64), c["want"])


@pytest.mark.parametrize("spec", C.CASES, ids=C.L.ident)
@pytest.mark.parametrize("seed", [2, 7], ids=["near_zero_points", "far_zero_points"])      # odd: wide_packed's 70000, the 64-bit I
def test_kernel_equals_the_composition_on_random_inputs(spec, seed):
    c = C.case(*spec, exact=False, seed=seed)
    want = composed(c)
    assert len(want.unique()) > min(8, want.numel() // 4), "a vacuous case"
    got = C.run(c, DEV, glu_epilogue=True)
    assert torch.equal(got, want) and torch.equal(C.run(c, DEV, glu_epilogue=True), got)   # ... and launches repeat
    assert torch.equal(C.run(c, DEV, glu_epilogue=False), want)


@pytest.mark.parametrize("spec", [C.CASES[4], C.CASES[1], C.CASES[7]], ids=C.L.ident)     # packets, bytes, many tiles
def test_y_at_a_byte_offset_keeps_its_surroundings(spec):
    c = C.case(*spec)
    M, N = c["want"].shape
    g = lambda t: None if t is None else t.to(DEV)
    ydt = torch.uint8 if c["out"][2][1] > 127 else torch.int8
    buf = torch.full((M * N + 64,), 0x5A, dtype=ydt, device=DEV)
    w = [(g(p.codes), g(p.scale.reshape(-1)), g(p.zero_point.reshape(-1)), g(b), g(o[0]), g(o[1]), *o[2])
         for p, b, o in zip(c["packed"], c["biases"], c["outs"])]
    osc, osh, rng = c["out"]
    E.linglu_w4_q(g(c["lx"]), g(c["s_x"]), g(c["zx"]), *w[0], *w[1], spec[3], spec[4], g(c["glu"]["s_u"]), g(c["glu"]["z_u"]), g(c["table"]),
                  g(osc), g(osh), *rng, c["mid"], out=buf[1:1 + M * N].view(M, N))
    assert torch.equal(buf[1:1 + M * N].view(M, N).cpu().to(torch.int64), c["want"])
    assert bool((buf[:1] == 0x5A).all()) and bool((buf[1 + M * N:] == 0x5A).all())


def test_more_rows_compose_with_the_same_bits_row_by_row():
    spec = (17,) + C.CASES[1][1:]
    c = C.case(*spec, exact=False, seed=5)
    assert not E.linglu_w4_plan(*spec[:5])["served"]
    whole = C.run(c, DEV, glu_epilogue=True)
    assert len(whole.unique()) > 8
    for m0 in (0, 16):
        assert torch.equal(C.run(dict(c, lx=c["lx"][m0:m0 + 16]), DEV, glu_epilogue=True), whole[m0:m0 + 16])


def test_the_module_with_a_residual_down_projection_in_a_captured_graph():
    from torchlsq.quantized import convert_packed_a8_glu
    block, q, xl, rl = C.qat_block(False)
    conv = convert_packed_a8_glu(block, {"mlp": q}, mid_dtype=torch.bfloat16, glu_epilogue=True, decode=True).mlp.to(DEV)
    dev = lambda t: F.LevelsTensor(t.levels.to(DEV), t.scale.to(DEV), t.zero_point.to(DEV), t.quant_min, t.quant_max, t.type_min, t.type_max)
    x, r = dev(xl), dev(rl)
    with torch.no_grad():
        want = conv(x, r).levels.clone()
        conv.glu_epilogue = False
        assert torch.equal(conv(x, r).levels, want) and len(want.unique()) > 8
        conv.glu_epilogue = True
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = conv(x, r).levels
        for _ in range(3):
            got.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(got, want)
