"""The levels-out linears on packed 4- / 2-bit codes (include/lsq_hip_lindec_w4.h) on CPU tensors, and what the GPU tests share.
`lsq_linear_packed_q8_q` / `lsq_linear_packed_q8_add_q` define nothing new, so the reference is PLAIN: the codes unpacked, the int64
/ float64 linear, then each step of the contract in float64 rounded to `mid_dtype`, then the project's CPU `lsq_levels_per_tensor`.
The inputs are exact -- qlinear_a8_cases.wide_exact_packed, S_X_EXACT, a bias of sixteenths, power-of-two quantizer scales with
integer zero points -- so every fp32 step of every order of the sum is exact and the comparison is on the bytes."""
import functools

import pytest
import torch

import qlinear_a8_cases as A
from torchlsq import extension, functional as F

OPS = torch.ops.torchlsq
U8, I8 = torch.uint8, torch.int8
F32, BF16 = torch.float32, torch.bfloat16
NONE, RES, PRE = 0, 1, 2            # no residual / a residual / a residual and the layer's own pre-quantizer
# (M, N, K, G, bits): one span | 17 spans, N % 16 != 0 | two chunks, four groups per span | span = lcm(3, 4) packets | a group
# across load steps | 2 bits (twice) | more tiles than compute units, x resident
SHAPES = [(1, 16, 128, 128, 4), (16, 40, 2176, 128, 4), (5, 32, 4224, 32, 4), (16, 16, 768, 96, 4), (9, 16, 512, 256, 4),
          (16, 48, 1024, 64, 2), (3, 16, 256, 128, 2), (2, 4128, 128, 128, 4)]
# (x levels, output levels unsigned, mid_dtype, relu, kind, residual levels) per shape: the cross product pruned to distinct code
VARIANTS = [(U8, True, BF16, False, NONE, U8), (U8, True, F32, True, PRE, I8), (I8, False, BF16, False, RES, U8), (U8, False, F32, False, PRE, U8),
            (I8, True, BF16, True, RES, I8), (U8, True, F32, False, NONE, U8), (I8, False, F32, True, NONE, U8), (U8, True, BF16, False, RES, U8)]
# ... and the byte-path shape with a plain residual on weights WITHOUT far zero points (exact_packed): the 32-bit forming of I
CASES = [s + v for s, v in zip(SHAPES, VARIANTS)] + [SHAPES[1] + VARIANTS[0], SHAPES[5] + VARIANTS[3], SHAPES[1] + VARIANTS[2] + (True, 0, False)]


def ident(spec):
    return "-".join(str(v).replace("torch.", "") for v in spec)


def quantizer(scale, zero, unsigned):
    lo, hi = (0, 255) if unsigned else (-128, 127)
    return torch.tensor([scale], dtype=F32), torch.tensor([-zero * scale], dtype=F32), (lo, hi, lo, hi)


def reference(c):
    """the bytes of one exact case: float64 steps, each rounded to `mid` (float64 -> float32 is exact or the fp32 step's one rounding)"""
    lx, s_x, zx, p, bias, (osc, osh, rng), relu, mid, res = c["args"]
    r, _ = A.reference(lx, float(s_x), int(zx), p, bias)
    u = r.float().to(mid)
    if res is not None:
        rl, rs, rz, psc, psh, prng = res
        if psc is not None:
            zp = -float(psh) / float(psc)
            u = ((torch.clamp(torch.round(u.double() / float(psc) + zp), prng[0], prng[1]) - zp) * float(psc)).float().to(mid)
        d = ((rl.double() - int(rz)) * float(rs)).float().to(mid)
        u = (u.double() + d.double()).float().to(mid)
    if relu:
        u = torch.where(u < 0, torch.zeros_like(u), u)
    lv = OPS.lsq_levels_per_tensor(u, osc, osh, *rng, 0)
    return lv.view(U8) if rng[1] > 127 else lv


@functools.lru_cache(maxsize=None)
def case(M, N, K, G, bits, x_dt=U8, unsigned=True, mid=BF16, relu=False, kind=NONE, r_dt=U8, exact=True, seed=0, wide=True):
    """CPU operands of one case, built once and left unchanged; `want` (exact cases): the plain reference's bytes"""
    lx = A.levels((M, K), *((0, 255) if x_dt == U8 else (-128, 127)), seed)
    zx = 117 if x_dt == U8 else -11
    if exact:
        p, s_x = (A.wide_exact_packed if wide else A.C.exact_packed)(N, K, G, bits, seed), A.S_X_EXACT
        bias = torch.randint(-64, 65, (N,), generator=A._gen(seed + 9)).float() / 16
    else:
        p, s_x = (A.wide_packed if seed % 2 else A.C.random_packed)(N, K, G, bits, seed), 0.0173
        bias = A.C.random_bias(N, F32, seed)
    s_x, zx = A.act(s_x, zx)
    r, _ = A.reference(lx, float(s_x), int(zx), p, bias)
    sd = 1.4826 * float((r - r.median()).abs().median()) + 1e-3         # of the bulk: a far zero point's column does not set the step
    step = 2.0 ** round(torch.log2(torch.tensor(sd / 24)).item()) * (1.0 if exact else 1.1)
    out = quantizer(step, 0 if relu or not unsigned else 128, unsigned)
    res = None
    if kind != NONE:
        rl = A.levels((M, N), *((0, 255) if r_dt == U8 else (-128, 127)), seed + 7)
        pre = quantizer(2 * step, 128, True) if kind == PRE else (None, None, (0, 255, 0, 255))
        res = (rl, torch.tensor([step / 2], dtype=F32), torch.tensor([100 if r_dt == U8 else -3], dtype=torch.int32)) + pre
    c = dict(args=(lx, s_x, zx, p, bias, out, relu, mid, res))
    if exact:
        c["want"] = reference(c)
        assert len(c["want"].unique()) > min(8, M * N // 4), "a vacuous case"
    return c


def run(c, device="cpu", decode=True, out=None, M=None):
    """the functional call on the case's operands (the first M rows) moved to `device`: the levels"""
    lx, s_x, zx, p, bias, (osc, osh, rng), relu, mid, res = c["args"]
    to = lambda t: None if t is None else t.to(device)
    x = F.LevelsTensor(to(lx[:M]), to(s_x), to(zx), *((0, 255) if lx.dtype == U8 else (-128, 127)))
    pk = F.PackedGroupTensor(to(p.codes), to(p.scale), to(p.zero_point), p.bits, p.group_size, p.quant_min, p.shape)
    kw = dict(out_scale=to(osc), out_shift=to(osh), out_quant_min=rng[0], out_quant_max=rng[1], relu=relu, mid_dtype=mid, decode=decode)
    if res is None:
        return F.lsq_linear_packed_a8_q(x, pk, to(bias), **kw).levels
    rl, rs, rz, psc, psh, prng = res
    r = F.LevelsTensor(to(rl[:M]), to(rs), to(rz), *((0, 255) if rl.dtype == U8 else (-128, 127)))
    return F.lsq_linear_packed_a8_add_q(x, pk, to(bias), r, pre_scale=to(psc), pre_shift=to(psh), pre_quant_min=prng[0],
                                        pre_quant_max=prng[1], **kw).levels


@pytest.mark.parametrize("spec", CASES, ids=ident)
def test_cpu_ops_equal_the_plain_reference(spec):
    c = case(*spec)
    for decode in (True, False, None):
        got = run(c, decode=decode)
        assert got.dtype == c["want"].dtype and torch.equal(got, c["want"])


@pytest.mark.parametrize("args, want", [
    ((16, 4096, 4096, 128, 4), dict(served=True, block=1024, chunks=1, x_resident=True, store="packets", res_load="packets",
                                    lds_bytes=16384 + 256 + 16 * 4112 + 16 * 32 * 4)),
    ((5, 32, 4224, 32, 4), dict(served=True, grid=2, chunks=2, x_resident=False)),
    ((16, 16, 4608, 96, 4), dict(served=True, chunks=2, lds_bytes=16384 + 256 + 16 * 3856 + 16 * 40 * 4)),
    ((16, 40, 2176, 128, 4), dict(served=True, grid=3, store="bytes", res_load="bytes")),
    ((3, 16, 256, 128, 2, True, False, True), dict(served=True, store="bytes", res_load="packets")),
    ((17, 4096, 4096, 128, 4), dict(served=False, grid=0, block=0, lds_bytes=0)),
    ((1, 64, 128, 8, 4), dict(served=False)),
    ((1, 64, 128, 32, 2), dict(served=False)),
    ((1, 64, 8192, 8192, 4), dict(served=False)),
    ((1, 64, 128, 128, 4, False), dict(served=False)),
])
def test_plan(args, want):
    pl = extension.lindec_w4_plan(*args)
    assert {k: pl[k] for k in want} == want, pl


def test_fake_kernels_give_the_shape_and_level_dtype():
    c = case(*CASES[2])
    lx, s_x, zx, p, bias, (osc, osh, rng), relu, mid, res = c["args"]
    w = (p.codes, p.scale.reshape(-1), p.zero_point.reshape(-1), bias, p.group_size, p.bits)
    with torch._subclasses.FakeTensorMode() as mode:
        f = lambda t: None if t is None else mode.from_tensor(t)
        y = OPS.lsq_linear_packed_q8_add_q(f(lx), f(s_x), f(zx), *[f(t) if isinstance(t, torch.Tensor) else t for t in w], f(osc), f(osh),
                                           *rng, relu, mid, f(res[0]), f(res[1]), f(res[2]), f(res[3]), f(res[4]), *res[5], True)
    assert y.shape == c["want"].shape and y.dtype == c["want"].dtype


def test_convert_packed_a8_q_equals_the_functional_calls_and_the_state_dict_round_trip():
    import test_qlinear_a8_cpu as Q
    from torchlsq.quantized import PackedLinearA8AddQ, PackedLinearA8Q, convert_packed_a8_q
    model, in_q, mid_q = Q._qat_model()                 # Linear(64, 32) -> ReLU -> Linear(32, 8), group-wise 4-bit weights
    conv = convert_packed_a8_q(model, {"0": in_q, "2": mid_q}, {"0": mid_q, "2": in_q}, relu=("0",), mid_dtype=BF16, decode=True)
    assert [type(m).__name__ for m in conv] == ["PackedLinearA8Q", "Identity", "PackedLinearA8Q"] and isinstance(model[0], torch.nn.Linear)
    assert conv[0].decode is True and conv[2].decode is True and conv[0].relu and not conv[2].relu
    x, r = in_q.quantize(torch.randn(5, 64)), in_q.quantize(torch.randn(5, 8))
    packed = [model[i].weight_fake_quant.export_packed(model[i].weight.detach()) for i in (0, 2)]
    out = lambda q: dict(out_scale=q.scale, out_shift=q.shift, out_quant_min=0, out_quant_max=127, out_type_min=0, out_type_max=255)
    with torch.no_grad():
        h = F.lsq_linear_packed_a8_q(x, packed[0], model[0].bias, relu=True, mid_dtype=BF16, **out(mid_q))
        want = F.lsq_linear_packed_a8_q(h, packed[1], None, mid_dtype=BF16, **out(in_q))
        got = conv(x)
        assert len(want.levels.unique()) > 8 and torch.equal(got.levels, want.levels) and torch.equal(got.scale, want.scale)
        add = PackedLinearA8AddQ.from_float(model[2], mid_q, in_q, pre_quantizer=mid_q, mid_dtype=BF16)
        want = F.lsq_linear_packed_a8_add_q(h, packed[1], None, F.LevelsTensor.from_quantized(r), mid_dtype=BF16, pre_scale=mid_q.scale,
                                            pre_shift=mid_q.shift, pre_quant_min=0, pre_quant_max=127, pre_type_min=0, pre_type_max=255,
                                            **out(in_q))
        assert torch.equal(add(h, r).levels, want.levels) and not torch.equal(want.levels, got.levels)
        for m, fresh in ((conv[2], PackedLinearA8Q(32, 8, bias=False)), (add, PackedLinearA8AddQ(32, 8, bias=False))):
            for decode in (None, False, True):          # `decode` is written only when it is not None
                m.decode = decode
                state = m.state_dict()
                assert ("decode" in state["_extra_state"]) == (decode is not None)
                fresh.load_state_dict(state)
                assert fresh.decode is decode and fresh.mid_dtype == BF16
                args = (h,) if m is conv[2] else (h, r)
                assert torch.equal(fresh(*args).levels, m(*args).levels)
