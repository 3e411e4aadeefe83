"""The gate and up linears on packed 4- / 2-bit codes with the gated product behind them (include/lsq_hip_linglu_w4.h) on CPU
tensors, and what the GPU tests share.  `lsq_linear_packed_q8_glu_q` defines nothing new, so the reference is PLAIN: the gate and
up bytes from test_lindec_w4_cpu.reference (float64 steps on exact inputs: every order of the fp32 sum is exact), the product by
glu_w8_cases' numpy restatement on those bytes."""
import functools

import pytest
import torch

import glu_w8_cases as GC
import qlinear_a8_cases as A
import test_lindec_w4_cpu as L
from torchlsq import extension, functional as F

OPS = torch.ops.torchlsq
U8, I8, F32, BF16 = L.U8, L.I8, L.F32, L.BF16
GATE, UP = 0, 1
# (x levels, gate levels unsigned, up levels unsigned, mid, fused halves under one quantizer, the strip with far zero points) per shape
VARIANTS = [(U8, True, True, BF16, True, GATE), (I8, False, True, F32, False, UP), (U8, True, False, BF16, False, GATE),
            (I8, True, True, F32, True, UP), (U8, False, False, BF16, True, GATE), (U8, True, False, F32, False, UP),
            (I8, False, True, BF16, False, GATE), (U8, True, True, F32, True, UP)]
CASES = [s + v for s, v in zip(L.SHAPES, VARIANTS)]


@functools.lru_cache(maxsize=None)
def case(M, C, K, G, bits, x_dt=U8, g_uns=True, u_uns=True, mid=BF16, fused=True, far=GATE, exact=True, seed=0):
    """CPU operands of one case, built once and left unchanged; `want` (exact cases): the plain reference's int64 levels"""
    lx = A.levels((M, K), *((0, 255) if x_dt == U8 else (-128, 127)), seed)
    if fused:
        u_uns = g_uns                                   # one quantizer
    packed, biases = [], []
    for side in (GATE, UP):
        if exact:
            p = (A.wide_exact_packed if side == far else A.C.exact_packed)(C, K, G, bits, seed + 31 * side)
            b = torch.randint(-64, 65, (C,), generator=A._gen(seed + 9 + side)).float() / 16
        else:
            p = (A.wide_packed if seed % 2 and side == far else A.C.random_packed)(C, K, G, bits, seed + 31 * side)
            b = A.C.random_bias(C, F32, seed + side)
        packed.append(p)
        biases.append(b if (C + side) % 2 else None)     # with and without a bias
    if fused:
        biases[UP] = None if biases[GATE] is None else torch.randint(-64, 65, (C,), generator=A._gen(seed + 10)).float() / 16
    s_x, zx = A.act(A.S_X_EXACT if exact else 0.0173, 117 if x_dt == U8 else -11)
    r = [A.reference(lx, float(s_x), int(zx), p, b)[0] for p, b in zip(packed, biases)]
    if not exact and seed % 2:      # random far zero points move a whole strip: a bias brings it back onto the SiLU's bend
        biases = [torch.zeros(C) if b is None else b for b in biases]
        biases[far] = biases[far] - r[far].median().float()
        r[far] = r[far] - r[far].median()
    outs = []
    for side, uns in ((GATE, g_uns), (UP, u_uns)):
        rr = torch.cat(r) if fused else r[side]
        sd = 1.4826 * float((rr - rr.median()).abs().median()) + 1e-3
        step = 2.0 ** round(torch.log2(torch.tensor(sd / 24)).item()) * (1.0 if exact else 1.1)
        outs.append(L.quantizer(step, 128 if uns else 0, uns))
    c = dict(M=M, C=C, lx=lx, s_x=s_x, zx=zx, packed=packed, biases=biases, outs=outs, mid=mid, fused=fused)
    # the two byte tensors, then the product's table and quantizer from the reference's own distribution
    gu = [L.reference(dict(args=(lx, s_x, zx, p, b, o, False, mid, None))) for p, b, o in zip(packed, biases, outs)]
    s_g, z_g = F._act_constants(*outs[GATE][:2], *outs[GATE][2][2:])
    s_u, z_u = F._act_constants(*outs[UP][:2], *outs[UP][2][2:])
    g = dict(rows=M, C=C, bufs=[t.contiguous().view(U8).flatten() for t in gu], gate=(0, 0, C), up=(1, 0, C), gd=gu[0].dtype, ud=gu[1].dtype,
             s_g=s_g, z_g=z_g, s_u=s_u, z_u=z_u, mid=mid, table=F.lsq_glu_table("silu", s_g, z_g, gu[0].dtype, None, mid))
    g["osc"], g["osh"], g["rng"] = GC.out_quantizer(torch.from_numpy(GC.numpy_value(g)), (M + C) % 3 != 0)
    c.update(table=g["table"], out=(g["osc"], g["osh"], g["rng"]), glu=g)
    if exact:
        c["want"] = torch.from_numpy(GC.numpy_result(g))
        ends = ((c["want"] == g["rng"][0]).sum() + (c["want"] == g["rng"][1]).sum()).item()
        assert len(c["want"].unique()) > min(8, M * C // 4) and 2 * ends <= M * C, "a vacuous case"
    return c


def run(c, device="cpu", glu_epilogue=True, decode=None, M=None):
    """the functional call on the case's operands (the first M rows) moved to `device`: the levels"""
    to = lambda t: None if t is None else t.to(device)
    x = F.LevelsTensor(to(c["lx"][:M]), to(c["s_x"]), to(c["zx"]), *((0, 255) if c["lx"].dtype == U8 else (-128, 127)))
    pk = [F.PackedGroupTensor(to(p.codes), to(p.scale), to(p.zero_point), p.bits, p.group_size, p.quant_min, p.shape) for p in c["packed"]]
    b, C = [to(t) for t in c["biases"]], c["C"]
    if c["fused"]:          # ONE [2 C, K] weight, passed as its two row halves under one quantizer
        cat = lambda ts: torch.cat(ts, 0)
        whole = F.PackedGroupTensor(cat([p.codes for p in pk]), cat([p.scale for p in pk]), cat([p.zero_point for p in pk]), pk[0].bits,
                                    pk[0].group_size, pk[0].quant_min, (2 * C, pk[0].shape[1]))
        half = lambda lo: F.PackedGroupTensor(whole.codes[lo:lo + C], whole.scale[lo:lo + C], whole.zero_point[lo:lo + C], whole.bits,
                                              whole.group_size, whole.quant_min, pk[0].shape)
        pk = [half(0), half(C)]
        if b[0] is not None:
            bb = cat(b)
            b = [bb[:C], bb[C:]]
    q = [(to(o[0]), to(o[1]), *o[2]) for o in c["outs"]]
    osc, osh, rng = c["out"]
    return F.lsq_gated_linear_packed_a8_q(x, pk[0], pk[1], to(c["table"]), q[0], None if c["fused"] else q[1], b[0], b[1], to(osc), to(osh),
                                          *rng, mid_dtype=c["mid"], glu_epilogue=glu_epilogue, decode=decode).levels


@pytest.mark.parametrize("spec", CASES, ids=L.ident)
def test_cpu_op_equals_the_plain_reference(spec):
    c = case(*spec)
    for glu_epilogue in (True, False, None):
        got = run(c, glu_epilogue=glu_epilogue)
        assert got.dtype == (U8 if c["out"][2][1] > 127 else I8) and torch.equal(got.to(torch.int64), c["want"])


@pytest.mark.parametrize("args, want", [
    ((16, 11008, 4096, 128, 4), dict(served=True, block=1024, chunks=1, x_resident=True, store="packets",
                                     lds_bytes=2 * 16384 + 3 * 256 + 1024 + 16 * 4112 + 16 * 32 * 4)),
    ((5, 32, 4224, 32, 4), dict(served=True, grid=2, chunks=2, x_resident=False)),
    ((16, 40, 2176, 128, 4), dict(served=True, grid=3, store="bytes")),
    ((3, 16, 256, 128, 2, True, False), dict(served=True, store="bytes")),
    ((17, 4096, 4096, 128, 4), dict(served=False, grid=0, block=0, lds_bytes=0)),
    ((1, 64, 128, 8, 4), dict(served=False)),
    ((1, 64, 128, 32, 2), dict(served=False)),
    ((1, 64, 128, 128, 4, False), dict(served=False)),
])
def test_plan(args, want):
    pl = extension.linglu_w4_plan(*args)
    assert {k: pl[k] for k in want} == want, pl


def test_fake_kernel_gives_the_shape_and_level_dtype():
    c = case(*CASES[1])
    w = [(p.codes, p.scale.reshape(-1), p.zero_point.reshape(-1), b, o[0], o[1], *o[2]) for p, b, o in zip(c["packed"], c["biases"], c["outs"])]
    g = c["glu"]
    args = (c["lx"], c["s_x"], c["zx"], *w[0], *w[1], c["packed"][0].group_size, c["packed"][0].bits, g["s_u"], g["z_u"], c["table"],
            g["osc"], g["osh"], *g["rng"], c["mid"])
    with torch._subclasses.FakeTensorMode() as mode:
        y = OPS.lsq_linear_packed_q8_glu_q(*[mode.from_tensor(t) if isinstance(t, torch.Tensor) else t for t in args])
    assert y.shape == c["want"].shape and y.dtype == (U8 if g["rng"][1] > 127 else I8)


def qat_block(shared):
    """glu_w8_cases' gated MLP block with group-wise 4-bit weight quantizers, fitted once: (block, the quantizer dict of its "mlp",
    the levels of a [5, 64] sample under the input quantizer and under the add's)"""
    from torch.ao.quantization.observer import MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    block, qs, x = GC.mlp_block(shared=shared, d=64, hidden=32, rows=5)
    for lin in (block.mlp.gate_proj, block.mlp.up_proj, block.mlp.down_proj):
        wq = LSQFakeQuantizer(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                              qscheme=torch.per_channel_symmetric, quant_min=-8, quant_max=7, group_size=32).train()
        wq(lin.weight.detach())
        wq.disable_observer()
        lin.weight_fake_quant = wq.eval()
    q = GC.mlp_quantizers(qs)
    return block, q, F.LevelsTensor.from_quantized(q["input_quantizer"].quantize(x)), F.LevelsTensor.from_quantized(q["add_quantizer"].quantize(x))


@pytest.mark.parametrize("shared", [True, False], ids=["fused", "pair"])
def test_convert_packed_a8_glu_equals_the_functional_calls_and_the_state_dict_round_trip(shared):
    from torchlsq.quantized import GatedMLPPackedA8Q, convert_packed_a8_glu
    block, q, xl, rl = qat_block(shared)
    conv = convert_packed_a8_glu(block, {"mlp": q}, mid_dtype=BF16).mlp
    assert isinstance(conv, GatedMLPPackedA8Q) and conv.fused == shared and "_extra_state" not in conv.state_dict()
    pk = [m.weight_fake_quant.export_packed(m.weight.detach()) for m in (block.mlp.gate_proj, block.mlp.up_proj)]
    out = lambda side: (lambda m: (m.output_scale, m.output_shift, *m.output_range))(conv.gate_up if shared else (conv.gate_proj, conv.up_proj)[side])
    with torch.no_grad():
        h = F.lsq_gated_linear_packed_a8_q(xl, pk[0], pk[1], conv.glu.table, out(GATE), out(UP), block.mlp.gate_proj.bias,
                                           block.mlp.up_proj.bias, conv.glu.output_scale, conv.glu.output_shift, *conv.glu.output_range,
                                           mid_dtype=BF16, glu_epilogue=False)
        want = conv.down(h, rl).levels
        assert len(want.unique()) > 8
        for glu_epilogue in (None, False, True):
            conv.glu_epilogue = glu_epilogue
            state = conv.state_dict()
            assert ("_extra_state" in state) == (glu_epilogue is not None)
            fresh = convert_packed_a8_glu(block, {"mlp": q}, mid_dtype=BF16, glu_epilogue=not glu_epilogue).mlp
            fresh.load_state_dict(state)
            assert fresh.glu_epilogue is glu_epilogue and torch.equal(fresh(xl, rl).levels, want) and torch.equal(conv(xl, rl).levels, want)
