"""What tests/test_glu_w8_cpu.py and tests/test_glu_w8_gpu.py share: the gated product act(gate) * up on 8-bit levels
(include/lsq_hip_glu_w8.h).  The op is DEFINED as existing ops composed -- with an activation quantizer
`lsq_mul_gate_w8_q(lsq_lut_w8(gate, act table), up, out)` on dense copies, without one `lsq_levels_per_tensor(fn(gate.dequantize(mid))
* up.dequantize(mid), out)` -- so every comparison is on the bits, and there is no tolerance anywhere in the three files.

A CASE is a dict: the byte buffers the operands live in (`bufs`, 1-D uint8), where gate and up lie in them (`gate`, `up`: buffer
index, byte offset, row stride), their level dtypes and constants, the float table (built ONCE on the CPU -- for the transcendental
functions ATen's CPU and GPU kernels may round differently -- and moved), the output quantizer (or None: floats out) and mid_dtype.
`operands(case, device)` moves each buffer once and cuts the views there, so the layout under test -- dense, the two halves of one
fused [rows, 2 C] buffer, the halves of a padded [rows, 2 C + 16] buffer, a base one byte off, a row stride that is no multiple of 16
-- is the layout the device sees.

Gate levels are uniform over all 256 bytes with scale 0.05 and zero point 128 (as uint8): the gate spans -6.4 .. 6.35, both bends of
SiLU / GELU / sigmoid.  Up levels are uniform with scale 0.0371 and zero point 128 or 3.  The output quantizer comes from the float32
products by `out_quantizer`: their 2nd to 98th percentile on the level range.  `assert_conditions` holds a random
levels-out case of at least 1000 outputs to `assert_not_vacuous` and to at least 40 % of the levels changing when gate, and when up,
is rolled by one column.
"""
import numpy as np
import torch

import eltwise_w8_cases as E
import requant_w8_cases as R

OPS = torch.ops.torchlsq
MIDS = R.MIDS
LEVEL_DTYPES = (torch.uint8, torch.int8)
DTYPE_PAIRS = [(g, u) for g in LEVEL_DTYPES for u in LEVEL_DTYPES]
S_G, Z_G, S_U = 0.05, 128, 0.0371
CLAMP_TYPE = ("relu", "identity")
TRANSCENDENTAL = ("silu", "gelu", "gelu_tanh", "sigmoid")
LAYOUTS = ("dense", "halves", "padded")
name, bits, one = E.name, E.bits, E.one


def pair_id(p):
    return "%s_%s" % (name(p[0]), name(p[1]))


def spec(layout, rows, C):
    """(bytes of each buffer, gate (buffer, offset, row stride), up (...)) of a layout"""
    if layout == "dense":
        return [rows * C, rows * C], (0, 0, C), (1, 0, C)
    if layout == "halves":
        return [rows * 2 * C], (0, 0, 2 * C), (0, C, 2 * C)
    if layout == "padded":
        return [rows * (2 * C + 16)], (0, 0, 2 * C + 16), (0, C, 2 * C + 16)
    if layout == "off_by_one":                      # both bases one byte off a 16-byte boundary
        return [rows * C + 16, rows * C + 16], (0, 1, C), (1, 1, C)
    if layout == "odd_stride":                      # row strides that are no multiple of 16
        return [rows * (C + 8), rows * (C + 24)], (0, 0, C + 8), (1, 0, C + 24)
    raise ValueError(layout)


def view(buf, where, rows, C, dtype):
    _, off, ld = where
    return buf.as_strided((rows, C), (ld, 1), off).view(dtype)


def glu_case(rows, C, pair=(torch.uint8, torch.uint8), out_variant=(True, torch.float32), fn="silu", act_q=False, layout="dense",
             zu=128, seed=0, exhaustive=False):
    """one case on the CPU, see the module's docstring; `out_variant`: (unsigned output levels -- None: floats out --, mid_dtype);
    `act_q`: a quantizer between the activation and the product (uint8, fitted to the activation's values on the 256 gate levels);
    `exhaustive`: gate byte = row index, up byte = column index (rows = C = 256)"""
    from torchlsq.functional import LevelsTensor, lsq_glu_table
    gd, ud = pair
    unsigned, mid = out_variant
    g = torch.Generator().manual_seed(7000 + seed + 13 * rows + C)
    sizes, gw, uw = spec(layout, rows, C)
    bufs = [torch.randint(0, 256, (n,), generator=g).to(torch.uint8) for n in sizes]      # the padding holds random bytes too
    if exhaustive:
        assert rows == 256 and C == 256
        view(bufs[gw[0]], gw, rows, C, torch.uint8).copy_(torch.arange(256, dtype=torch.uint8).reshape(256, 1).expand(256, 256))
        view(bufs[uw[0]], uw, rows, C, torch.uint8).copy_(torch.arange(256, dtype=torch.uint8).reshape(1, 256).expand(256, 256))
    # the random bytes ARE the stored bytes: as int8 they are levels of the same distribution less 128, with the zero point moved along
    z_g = one(Z_G if gd == torch.uint8 else Z_G - 128, torch.int32)
    z_u = one(zu if ud == torch.uint8 else zu - 128, torch.int32)
    s_g, s_u = one(S_G), one(S_U)
    case = dict(rows=rows, C=C, bufs=bufs, gate=gw, up=uw, gd=gd, ud=ud, s_g=s_g, z_g=z_g, s_u=s_u, z_u=z_u, mid=mid, fn=fn, layout=layout,
                act=None, osc=None, osh=None, rng=None)
    if act_q:
        from torchlsq.functional import act_function
        b = torch.arange(256, dtype=torch.uint8).view(gd)
        call, _ = act_function(fn)
        v = LevelsTensor(b, s_g, z_g, 0, 255).dequantize(torch.float32)
        v = v if call is None else call(v)
        a_s = float(v.max() - v.min()) / 255.0                      # the activation's range on 0..255
        case["act"] = (one(a_s), one(float(v.min())), 0, 255, 0, 255)
    case["table"] = lsq_glu_table(fn, s_g, z_g, gd, case["act"], mid)
    if unsigned is not None:
        gt, ut = operands(case)
        v = case["table"][gt.levels.contiguous().view(torch.uint8).long()] * ut.dequantize(torch.float32)
        case["osc"], case["osh"], case["rng"] = out_quantizer(v, unsigned)
    return case


def out_quantizer(v, unsigned):
    """(out_scale [1], out_shift [1], (quant_min, quant_max, type_min, type_max)) for float32 products v: the range runs from their
    2nd to their 98th percentile (widened to hold 0, so the zero point is a level), so about 4 % of the levels sit on the borders, both
    are hit, and the rest lie strictly inside.  (`requant_w8_cases.out_quantizer` takes its scale from the median absolute deviation,
    which is 0 where half the products are: a ReLU gate.)"""
    v = v.detach().double().flatten()
    lo, hi = min(float(v.quantile(0.02)), 0.0), max(float(v.quantile(0.98)), 0.0)
    qlo, qhi = (0, 255) if unsigned else (-128, 127)
    s = (hi - lo) / (qhi - qlo)
    zp = round(qlo - lo / s)
    return one(s), one(-zp * s), (qlo, qhi, qlo, qhi)


def operands(case, device=None):
    """(gate, up) as LevelsTensors whose levels are VIEWS of the case's buffers moved to `device` (None: the CPU's as they are)"""
    from torchlsq.functional import LevelsTensor
    bufs = case["bufs"] if device is None else [b.to(device) for b in case["bufs"]]
    mv = (lambda t: t) if device is None else (lambda t: t.to(device))
    lo = {torch.uint8: (0, 255), torch.int8: (-128, 127)}
    gate = LevelsTensor(view(bufs[case["gate"][0]], case["gate"], case["rows"], case["C"], case["gd"]), mv(case["s_g"]), mv(case["z_g"]),
                        *lo[case["gd"]])
    up = LevelsTensor(view(bufs[case["up"][0]], case["up"], case["rows"], case["C"], case["ud"]), mv(case["s_u"]), mv(case["z_u"]),
                      *lo[case["ud"]])
    return gate, up


def run(case, device=None, ops=None):
    """the op under test on `device`; `ops`: operands already there (to look at the buffers afterwards)"""
    gate, up = operands(case, device) if ops is None else ops
    mv = (lambda t: t) if device is None else (lambda t: t.to(device))
    args = (gate.levels, up.levels, up.scale, up.zero_point, mv(case["table"]))
    if case["rng"] is None:
        return OPS.lsq_glu_w8_q8(*args, case["mid"])
    return OPS.lsq_glu_w8_q8_q(*args, mv(case["osc"]), mv(case["osh"]), *case["rng"], case["mid"])


def dense(t):
    from torchlsq.functional import LevelsTensor
    return LevelsTensor(t.levels.contiguous(), t.scale, t.zero_point, t.quant_min, t.quant_max, t.type_min, t.type_max)


def composed_with_act_quantizer(case, device=None):
    """the first composition: `lsq_mul_gate_w8_q(lsq_lut_w8(gate, act table), up, out)` on dense copies (floats out: `lsq_mul_gate_w8`)"""
    from torchlsq.functional import lsq_act_table, lsq_lut_w8, lsq_mul_gate_w8, lsq_mul_gate_w8_q
    assert case["act"] is not None
    gate, up = (dense(t) for t in operands(case, device))
    mv = (lambda t: t) if device is None else (lambda t: t.to(device))
    act = tuple(mv(t) if isinstance(t, torch.Tensor) else t for t in case["act"])
    # the byte table is built on the CPU, as the float table was, and moved
    table = mv(lsq_act_table(case["fn"], case["s_g"], case["z_g"], case["gd"], *case["act"], mid_dtype=case["mid"]))
    a = lsq_lut_w8(gate, table, *act)
    if case["rng"] is None:
        return lsq_mul_gate_w8(a, up, case["mid"])
    return lsq_mul_gate_w8_q(a, up, mv(case["osc"]), mv(case["osh"]), *case["rng"], mid_dtype=case["mid"]).levels


def composed_without(case):
    """the second composition, on the CPU: `lsq_levels_per_tensor(fn(gate.dequantize(mid)) * up.dequantize(mid), out)`"""
    from torchlsq.functional import act_function
    assert case["act"] is None
    gate, up = operands(case)
    call, _ = act_function(case["fn"])
    a = gate.dequantize(case["mid"])
    t = (a if call is None else call(a)) * up.dequantize(case["mid"])
    return t if case["rng"] is None else R.levels_of(t, case["osc"], case["osh"], case["rng"], False)


def numpy_value(case):
    """t of the contract in np.float32 steps with the roundings to `mid` explicit: float32 values [rows, C]"""
    f = np.float32
    gate, up = operands(case)
    a = E.round_to(case["table"].numpy(), case["mid"])[gate.levels.contiguous().view(torch.uint8).numpy().astype(np.int64)]
    d = E.round_to(((up.levels.numpy().astype(f) - f(int(case["z_u"]))) * f(float(case["s_u"]))).astype(f), case["mid"])
    return E.round_to((a * d).astype(f), case["mid"])


def numpy_result(case):
    """the result by the numpy restatement: int64 levels, or float32 values of `mid`"""
    t = numpy_value(case)
    return t if case["rng"] is None else E.numpy_levels(t, case["osc"], case["osh"], case["rng"])


def same(got, want):
    """bit equality of two results (levels, or floats of mid) of one shape"""
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(bits(got.cpu()), bits(want.cpu()))


def matches_numpy(got, case):
    want = numpy_result(case)
    if case["rng"] is None:
        return same(got.float(), torch.from_numpy(want))
    return bool((got.to(torch.int64).numpy() == want).all())


def expected_plan(rows, C, gs=None, us=None, aligned=True, cus=256, max_per=2):
    """the plan's fields by the rule of include/lsq_hip_glu_w8.h"""
    gs, us = C if gs is None else gs, C if us is None else us
    if not aligned or C % 16 or gs % 16 or us % 16:
        return dict(family="generic", grid=-(-rows * C // 256), block=256, packets_per_lane=1, lds_bytes=0, packets=0)
    packets, per = rows * C // 16, max_per
    while per > 1 and -(-packets // (256 * per)) < 2 * cus:
        per //= 2
    return dict(family="packets", grid=-(-packets // (256 * per)), block=256, packets_per_lane=per, lds_bytes=1024, packets=packets)


def plan_of(case, aligned=True):
    from torchlsq import extension as X
    return X.glu_w8_plan(case["rows"], case["C"], case["gate"][2], case["up"][2], aligned)


def differ(a, b):
    return (a != b).double().mean().item()


def assert_conditions(got, case, note=""):
    """the non-vacuity conditions of a random levels-out case of at least 1000 outputs, on the CPU path's result `got`"""
    assert got.numel() >= 1000 and case["rng"] is not None
    R.assert_not_vacuous(got, case["rng"], note)
    for side in ("gate", "up"):
        rolled = dict(case, bufs=[b.clone() for b in case["bufs"]])
        v = view(rolled["bufs"][case[side][0]], case[side], case["rows"], case["C"], torch.uint8)
        v.copy_(v.roll(1, 1))
        share = differ(got, run(rolled))
        assert share >= 0.40, (note, "only %.1f %% of the levels change when %s is rolled by one column" % (100 * share, side))


# ---------------------------------------------------------------------------------------------------
# a Llama-style MLP for the modules and the converter
# ---------------------------------------------------------------------------------------------------
class GatedMLP(torch.nn.Module):
    """HF's LlamaMLP: down_proj(act_fn(gate_proj(x)) * up_proj(x))"""

    def __init__(self, d=32, hidden=48, act=None):
        super().__init__()
        self.gate_proj = torch.nn.Linear(d, hidden)
        self.up_proj = torch.nn.Linear(d, hidden)
        self.down_proj = torch.nn.Linear(hidden, d)
        self.act_fn = torch.nn.SiLU() if act is None else act

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class Block(torch.nn.Module):
    def __init__(self, d=32, hidden=48):
        super().__init__()
        self.mlp = GatedMLP(d, hidden)

    def forward(self, x):
        return self.mlp(x) + x


def mlp_block(shared=True, act_q=False, d=32, hidden=48, rows=24, seed=0):
    """(the QAT block in eval mode, its per-tensor quint8 quantizers by site, a float32 sample [rows, d]): per-channel symmetric qint8
    weights.  Sites: "in", "gate", "up" (`shared`: the SAME object as "gate", fitted on both), optionally "act", "hidden" (the
    product), "down" (the down projection's own output), "add"."""
    import norm_w8_cases as N
    torch.manual_seed(7100 + seed)
    net = Block(d, hidden)
    with torch.no_grad():
        net.mlp.gate_proj.weight.mul_(4.0)          # gate values of a few units: both bends of the SiLU
    x = torch.randn(rows, d, generator=torch.Generator().manual_seed(7200 + seed)) * 2
    net = N._prepared(net, x)
    T = R.trained_quantizer
    qs = {}
    with torch.no_grad():
        qs["in"] = T(x)
        xq = qs["in"](x)
        g, u = net.mlp.gate_proj(xq), net.mlp.up_proj(xq)
        if shared:
            qs["gate"] = qs["up"] = T(torch.cat((g.flatten(), u.flatten())))
        else:
            qs["gate"], qs["up"] = T(g), T(u)
        a = net.mlp.act_fn(qs["gate"](g))
        if act_q:
            qs["act"] = T(a)
            a = qs["act"](a)
        h = a * qs["up"](u)
        qs["hidden"] = T(h)
        o = net.mlp.down_proj(qs["hidden"](h))
        qs["down"] = T(o)
        qs["add"] = T(qs["down"](o) + xq)
    return net, qs, x


def mlp_quantizers(qs, add=True):
    """the dict `convert_w8a8_glu` takes for the block's "mlp" """
    d = dict(input_quantizer=qs["in"], gate_quantizer=qs["gate"], up_quantizer=qs["up"], hidden_quantizer=qs["hidden"],
             down_output_quantizer=qs["down"])
    if "act" in qs:
        d["act_quantizer"] = qs["act"]
    if add:
        d["add_quantizer"] = qs["add"]
    return d
