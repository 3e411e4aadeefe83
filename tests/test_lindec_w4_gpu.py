"""liblsq_hip_lindec_w4.so on the GPU: every byte against the plain reference of tests/test_lindec_w4_cpu.py on exact inputs, and
against the existing GPU ops composed on random ones -- the order-of-sum contract of include/lsq_hip_lindec_w4.h."""
import pytest
import torch

import test_lindec_w4_cpu as C
from test_lindec_w4_cpu import BF16, F32, I8, NONE, PRE, RES, U8
from torchlsq import extension as E, functional as F

pytestmark = pytest.mark.gpu
OPS = torch.ops.torchlsq
DEV = "cuda"


def composed(c, M=None):
    """the definition written out from the existing GPU ops"""
    lx, s_x, zx, p, bias, (osc, osh, rng), relu, mid, res = c["args"]
    g = lambda t: None if t is None else t.to(DEV)
    y = OPS.lsq_linear_packed_q8(g(lx[:M]), g(s_x), g(zx), g(p.codes), g(p.scale.reshape(-1)), g(p.zero_point.reshape(-1)), g(bias),
                                 p.group_size, p.bits, mid)
    if res is not None:
        rl, rs, rz, psc, psh, prng = res
        if psc is not None:
            y = F.lsq(y, g(psc), g(psh), *prng)
        y = y + F.LevelsTensor(g(rl[:M]), g(rs), g(rz), 0, 255).dequantize(mid)
    if relu:
        y = torch.where(y < 0, torch.zeros_like(y), y)
    lv = OPS.lsq_levels_per_tensor(y, g(osc), g(osh), *rng, 0)
    return lv.view(U8) if rng[1] > 127 else lv


@pytest.mark.parametrize("spec", C.CASES, ids=C.ident)
def test_kernel_equals_the_plain_reference_on_exact_inputs(spec):
    c = C.case(*spec)
    M, N, K, G, bits = spec[:5]
    assert E.lindec_w4_plan(M, N, K, G, bits)["served"]
    got = C.run(c, DEV, decode=True)
    assert got.dtype == c["want"].dtype and torch.equal(got.cpu(), c["want"])


@pytest.mark.parametrize("spec", C.CASES, ids=C.ident)
@pytest.mark.parametrize("seed", [2, 7], ids=["near_zero_points", "far_zero_points"])      # odd: wide_packed's 70000, the 64-bit I
def test_kernel_equals_the_composition_on_random_inputs(spec, seed):
    c = C.case(*spec[:11], exact=False, seed=seed)
    want = composed(c)
    assert len(want.unique()) > min(8, want.numel() // 4), "a vacuous case"
    got = C.run(c, DEV, decode=True)
    assert torch.equal(got, want) and torch.equal(C.run(c, DEV, decode=True), got)         # ... and launches repeat
    assert torch.equal(C.run(c, DEV, decode=False), want)


@pytest.mark.parametrize("rows", [17, 40])
@pytest.mark.parametrize("kind", [NONE, PRE])
def test_more_rows_compose_with_the_same_bits_row_by_row(rows, kind):
    c = C.case(rows, 40, 2176, 128, 4, U8, True, BF16, False, kind, I8, exact=False, seed=5)
    assert not E.lindec_w4_plan(rows, 40, 2176, 128, 4)["served"]
    whole = C.run(c, DEV, decode=True)
    for m0 in range(0, rows, 16):
        lx, s_x, zx, p, bias, out, relu, mid, res = c["args"]
        part = dict(args=(lx[m0:m0 + 16], s_x, zx, p, bias, out, relu, mid, None if res is None else (res[0][m0:m0 + 16],) + res[1:]))
        assert torch.equal(C.run(part, DEV, decode=True), whole[m0:m0 + 16])
    assert torch.equal(C.run(c, DEV, decode=True, M=1), whole[:1])


@pytest.mark.parametrize("spec", [C.CASES[1], C.CASES[4], C.CASES[7]], ids=C.ident)
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
    if res is None:
        E.lindec_w4_linear_levels(*args, out=y)
    else:
        rbuf = torch.zeros(M * N + 16, dtype=res[0].dtype, device=DEV)
        rbuf[1:1 + M * N] = g(res[0]).flatten()
        E.lindec_w4_linear_levels_add(*args, rbuf[1:1 + M * N].view(M, N), g(res[1]), g(res[2]), g(res[3]), g(res[4]), *res[5], out=y)
    assert torch.equal(y.cpu(), c["want"])
    assert bool((buf[:1] == 0x5A).all()) and bool((buf[1 + M * N:] == 0x5A).all())


def test_misaligned_codes_take_the_composed_route():
    c = C.case(*C.CASES[3], exact=False, seed=2)
    lx, s_x, zx, p, bias, out, relu, mid, res = c["args"]
    shifted = torch.zeros(p.codes.numel() + 16, dtype=U8, device=DEV)[1:1 + p.codes.numel()].view(p.codes.shape)
    shifted.copy_(p.codes)
    assert shifted.data_ptr() % 16 == 1
    q = F.PackedGroupTensor(shifted, p.scale.to(DEV), p.zero_point.to(DEV), p.bits, p.group_size, p.quant_min, p.shape)
    assert torch.equal(C.run(dict(args=(lx, s_x, zx, q, bias, out, relu, mid, res)), DEV, decode=True), C.run(c, DEV, decode=True))


def test_two_modules_in_a_captured_graph():
    """PackedLinearA8Q -> PackedLinearA8AddQ, decode=True: several replays against the eager result"""
    from torchlsq.quantized import PackedLinearA8AddQ, PackedLinearA8Q
    a, b = C.case(4, 64, 256, 128, 4, U8, True, BF16, True, NONE, U8, exact=False, seed=2), \
        C.case(4, 32, 64, 32, 4, U8, True, BF16, False, PRE, U8, exact=False, seed=4)
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
    h = mods[0](x)                                      # the functional calls, composed: layer 2 on layer 1's levels and constants
    assert torch.equal(h.levels, C.run(a, DEV, decode=False))
    want = C.run(dict(args=(h.levels.cpu(), h.scale.cpu(), h.zero_point.cpu()) + b["args"][3:]), DEV, decode=False)
    assert torch.equal(chain(), want) and len(want.unique()) > 8
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = chain()
    for _ in range(3):
        got.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
