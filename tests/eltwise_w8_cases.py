"""What tests/test_eltwise_w8_cpu.py and tests/test_eltwise_w8_gpu.py share: the elementwise ops on 8-bit levels
(include/lsq_hip_eltwise_w8.h).  Both ops are DEFINED as existing ops composed -- the table op is `table[x.long()]`, the gate
multiply is `lsq_levels_per_tensor(x.dequantize(mid) * gate.dequantize(mid)[:, :, None, None], ...)` -- so every comparison is on
the bits, and there is no tolerance anywhere in the three files.

Gate cases are built so that no comparison is vacuous: x levels uniform in 0..255 with s_x = 0.0371, gate levels uniform in
0..255 with s_g = 1 / 255, the output quantizer from the float32 products by `requant_w8_cases.out_quantizer` -- its form without
ReLU (zero point in the middle of the range, scale sd / 64) where the products have both signs; where they have one (x zero
point 0 or 3 with gate zero point 0: no product is below -0.12, and no level below a mid-range zero point can be reached) its
other form (zero point on quant_min, scale sd / 96), see `one_sided`.
`assert_conditions` holds every random levels-out case of at least 1000 outputs to `assert_not_vacuous` (at least 25 % of the
levels strictly inside the range, both borders hit) and to at least 40 % of the levels changing when the gate is rolled by one
channel, and by one image.  The table op's tests use a random PERMUTATION of 0..255 as the table, so that every wrong index
shows, and plant a shuffled arange(256) in x, so that every entry is read.
"""
import numpy as np
import torch

import requant_w8_cases as R

OPS = torch.ops.torchlsq
CL = torch.channels_last
MIDS = R.MIDS
LEVEL_DTYPES = (torch.uint8, torch.int8)
S_X, S_G = 0.0371, 1.0 / 255.0
# (B, C, H, W): H = W = 1 is the same-shape product; 480 to 50176 outputs
GEOMETRIES = [(1, 16, 1, 1), (3, 32, 1, 1), (2, 16, 3, 5), (2, 48, 7, 7), (4, 64, 14, 14)]
# (x dtype, gate dtype, x zero point, gate zero point) as for uint8 levels; an int8 operand holds the same levels less 128
VARIANTS = [(xd, gd, zx, zg) for xd in LEVEL_DTYPES for gd in LEVEL_DTYPES for zx in (0, 3, 128) for zg in (0, 128)]
# (unsigned output levels -- None: floats out --, mid_dtype)
OUT_VARIANTS = [(u, mid) for u in (True, False, None) for mid in MIDS]
NAMED = ("identity", "relu", "relu6", "hardtanh", "leaky_relu", "hardswish", "hardsigmoid", "silu", "gelu", "gelu_tanh", "sigmoid", "tanh")
CLAMP_TYPE = ("identity", "relu", "relu6", "hardtanh")
LUT_SIZES = (1, 15, 16, 17, 255, 256, 4096)


def name(dtype):
    return str(dtype).replace("torch.", "")


def geom_id(g):
    return "%dx%dx%dx%d" % g


def variant_id(v):
    return "%s_%s_z%d_%d" % (name(v[0]), name(v[1]), v[2], v[3])


def bits(t):
    """a floating tensor as integers, for torch.equal on the bits (NaNs and signed zeros included)"""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16) if t.is_floating_point() else t


def one(v, dtype=torch.float32):
    return torch.tensor([v], dtype=dtype)


# -------------------------------------------------------------------------------------------------
# the table op
# -------------------------------------------------------------------------------------------------
def perm_table(seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randperm(256, generator=g).to(torch.uint8)


def lut_x(n, seed=0):
    """n random bytes; from 256 bytes on a shuffled arange(256) is planted at a random offset, so every table entry is read"""
    g = torch.Generator().manual_seed(2000 + seed + n)
    x = torch.randint(0, 256, (n,), generator=g).to(torch.uint8)
    if n >= 256:
        at = int(torch.randint(0, n - 255, (1,), generator=g))
        x[at:at + 256] = torch.randperm(256, generator=g).to(torch.uint8)
        assert len(x.unique()) == 256
    return x


def hardswish_table(device="cpu", mid=torch.bfloat16):
    """a real table: hardswish between a uint8 quantizer of scale 0.05, zero point 128 and one of scale 0.03, zero point 13"""
    from torchlsq.functional import lsq_act_table
    return lsq_act_table("hardswish", one(0.05).to(device), one(128, torch.int32).to(device), torch.uint8, one(0.03).to(device),
                         one(-13 * 0.03).to(device), 0, 255, mid_dtype=mid)


def expected_plan_lut(n, aligned=True, cus=256, max_per=2):
    """the plan's fields by the rule of include/lsq_hip_eltwise_w8.h"""
    if not aligned or n < 16:
        return dict(family="generic", grid=-(-n // 256), block=256, packets_per_lane=1, lds_bytes=0, packets=0, tail_bytes=0)
    packets, per = n // 16, max_per
    while per > 1 and -(-packets // (256 * per)) < 2 * cus:
        per //= 2
    return dict(family="packets", grid=-(-packets // (256 * per)), block=256, packets_per_lane=per, lds_bytes=256, packets=packets,
                tail_bytes=n % 16)


def expected_plan_mul(B, C, H, W, aligned=True, cus=256, max_pix=4):
    if not aligned or C % 16:
        return dict(family="generic", grid=-(-B * C * H * W // 256), block=256, pixels_per_lane=1, lds_bytes=0, lanes_per_image=0)
    pix = max_pix
    while pix > 1 and pix > H * W:
        pix //= 2
    while pix > 1 and -(-(B * (C // 16) * -(-H * W // pix)) // 256) < 2 * cus:
        pix //= 2
    lanes = (C // 16) * -(-H * W // pix)
    return dict(family="packets", grid=-(-B * lanes // 256), block=256, pixels_per_lane=pix, lds_bytes=0, lanes_per_image=lanes)


# -------------------------------------------------------------------------------------------------
# the gate multiply
# -------------------------------------------------------------------------------------------------
def as_dtype(levels_u8, zero_u8, dtype):
    """uint8 levels and their zero point as `dtype` levels of the same real values: int8 holds the levels less 128"""
    if dtype == torch.uint8:
        return levels_u8, one(zero_u8, torch.int32)
    return (levels_u8.to(torch.int16) - 128).to(torch.int8), one(zero_u8 - 128, torch.int32)


def mul_case(geometry, variant, out_variant, seed=0):
    """(lx, s_x, zx, lg, s_g, zg, out_scale, out_shift, range or None, mid): x [B, C, H, W] channels-last (H = W = 1: [B, C]), the
    gate [B, C, 1, 1] ([B, C])"""
    B, C, H, W = geometry
    xd, gd, zx8, zg8 = variant
    unsigned, mid = out_variant
    g = torch.Generator().manual_seed(3000 + seed + 7 * B + C + 31 * H)
    lx8 = torch.randint(0, 256, (B, C, H, W), generator=g).to(torch.uint8)
    lg8 = torch.randint(0, 256, (B, C, 1, 1), generator=g).to(torch.uint8)
    if H == 1 and W == 1:
        lx8, lg8 = lx8.reshape(B, C), lg8.reshape(B, C)
    else:
        lx8 = lx8.contiguous(memory_format=CL)
    lx, zx = as_dtype(lx8, zx8, xd)
    lg, zg = as_dtype(lg8, zg8, gd)
    s_x, s_g = one(S_X), one(S_G)
    if unsigned is None:
        return (lx, s_x, zx, lg, s_g, zg, None, None, None, mid)
    v = value(lx, s_x, zx, lg, s_g, zg, torch.float32)
    osc, osh, rng = R.out_quantizer(v, unsigned, one_sided(v))
    return (lx, s_x, zx, lg, s_g, zg, osc, osh, rng, mid)


def one_sided(v):
    """whether (nearly) no product is negative: x zero point 0 or 3 with gate zero point 0, an SE gate after a hardswish.  A level
    below a mid-range zero point is then out of reach, so `out_quantizer` is asked for its other form, the zero point on
    quant_min and the scale sd / 96: the conditions of `assert_conditions` are the same in both forms"""
    return float((v < 0).double().mean()) < 0.05


def value(lx, s_x, zx, lg, s_g, zg, mid):
    """t of the definition through `LevelsTensor.dequantize` and torch's multiply, as they are"""
    from torchlsq.functional import LevelsTensor
    a = LevelsTensor(lx, s_x, zx, 0, 255).dequantize(mid)
    g = LevelsTensor(lg, s_g, zg, 0, 255).dequantize(mid)
    return a * g.reshape(g.shape[0], g.shape[1], *([1] * (lx.dim() - 2)))


def run(case, device=None):
    """the op under test, on `device` (None: where the case lies)"""
    lx, s_x, zx, lg, s_g, zg, osc, osh, rng, mid = case if device is None else \
        tuple(t.to(device) if isinstance(t, torch.Tensor) else t for t in case)
    if rng is None:
        return OPS.lsq_mul_gate_w8_q8(lx, s_x, zx, lg, s_g, zg, mid)
    return OPS.lsq_mul_gate_w8_q8_q(lx, s_x, zx, lg, s_g, zg, osc, osh, *rng, mid)


def composed(case, device=None):
    """the definition: the existing ops composed -- `dequantize`, `torch.mul`, `lsq_levels_per_tensor`"""
    lx, s_x, zx, lg, s_g, zg, osc, osh, rng, mid = case if device is None else \
        tuple(t.to(device) if isinstance(t, torch.Tensor) else t for t in case)
    t = value(lx, s_x, zx, lg, s_g, zg, mid)
    if rng is None:
        return t
    return R.levels_of(t, osc, osh, rng, False)


def round_to(v, mid):
    """np.float32 values rounded to `mid` and back, through torch's conversion"""
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(mid).to(torch.float32).numpy()


def numpy_value(lx, s_x, zx, lg, s_g, zg, mid):
    """t of the contract in np.float32 steps with the roundings to `mid` explicit: float32 values of x's shape"""
    f = np.float32
    shape = tuple(lg.shape[:2]) + (1,) * (lx.dim() - 2)
    a = (lx.cpu().numpy().astype(f) - f(int(zx))) * f(float(s_x))
    g = (lg.cpu().numpy().astype(f).reshape(shape) - f(int(zg))) * f(float(s_g))
    a, g = round_to(a.astype(f), mid), round_to(g.astype(f), mid)
    return round_to((a * g).astype(f), mid)


def numpy_levels(u, osc, osh, rng):
    """lsq_math.hpp's level() in np.float32 steps on float32 values u: int64 levels"""
    qmin, qmax, tmin, tmax = (np.float32(v) for v in rng)
    s = np.maximum(np.abs(np.float32(float(osc))), np.float32(np.finfo(np.float32).eps))
    inv = np.float32(1.0) / s
    zp = np.rint(np.minimum(tmax, np.maximum(tmin, -np.float32(float(osh)) * inv)))
    t = u.astype(np.float32) * inv + zp
    q = np.rint(np.minimum(qmax, np.maximum(qmin, t)))
    return np.where(np.isnan(t), qmin, q).astype(np.int64)


def differ(a, b):
    return (a != b).double().mean().item()


def assert_conditions(got, case, note=""):
    """the non-vacuity conditions of a levels-out case of at least 1000 outputs, on the CPU path's result `got`; returns (share
    strictly inside the range, share changed by a channel roll of the gate, by an image roll -- None for one image)"""
    lx, s_x, zx, lg, s_g, zg, osc, osh, rng, mid = case
    assert got.numel() >= 1000 and rng is not None
    R.assert_not_vacuous(got, rng, note)
    ch = differ(got, run((lx, s_x, zx, lg.roll(1, 1), s_g, zg, osc, osh, rng, mid)))
    assert ch >= 0.40, (note, "only %.1f %% of the levels change when the gate is rolled by one channel" % (100 * ch))
    im = None
    if lx.shape[0] > 1:
        im = differ(got, run((lx, s_x, zx, lg.roll(1, 0), s_g, zg, osc, osh, rng, mid)))
        assert im >= 0.40, (note, "only %.1f %% of the levels change when the gate is rolled by one image" % (100 * im))
    lv = got.to(torch.int64)
    return ((lv > rng[0]) & (lv < rng[1])).double().mean().item(), ch, im


# -------------------------------------------------------------------------------------------------
# a MobileNetV3-style block
# -------------------------------------------------------------------------------------------------
class SqueezeExcitation(torch.nn.Module):
    """torchvision's quantizable SE block: global average pool -> 1 x 1 + ReLU -> 1 x 1 -> hardsigmoid, and the multiply through
    a FloatFunctional, operands in torchvision's order"""

    def __init__(self, channels, squeeze):
        super().__init__()
        self.avgpool = torch.nn.AdaptiveAvgPool2d(1)
        self.fc1 = torch.nn.Sequential(torch.nn.Conv2d(channels, squeeze, 1), torch.nn.ReLU())
        self.fc2 = torch.nn.Conv2d(squeeze, channels, 1)
        self.scale_activation = torch.nn.Hardsigmoid()
        self.skip_mul = torch.ao.nn.quantized.FloatFunctional()

    def _scale(self, x):
        return self.scale_activation(self.fc2(self.fc1(self.avgpool(x))))

    def forward(self, x):
        return self.skip_mul.mul(self._scale(x), x)


class V3Block(torch.nn.Module):
    """MobileNetV3's block at stride 1: 1 x 1 expand + hardswish -> depthwise 3 x 3 + hardswish -> SE -> 1 x 1 project -> + x"""

    def __init__(self, channels=16, hidden=48, squeeze=16):
        super().__init__()
        self.expand = torch.nn.Sequential(torch.nn.Conv2d(channels, hidden, 1), torch.nn.Hardswish())
        self.depthwise = torch.nn.Sequential(torch.nn.Conv2d(hidden, hidden, 3, padding=1, groups=hidden), torch.nn.Hardswish())
        self.se = SqueezeExcitation(hidden, squeeze)
        self.project = torch.nn.Conv2d(hidden, channels, 1)
        self.add = torch.ao.nn.quantized.FloatFunctional()

    def forward(self, x):
        return self.add.add(self.project(self.se(self.depthwise(self.expand(x)))), x)


def v3_block():
    """(the QAT block in eval mode, the per-tensor quint8 activation quantizers beside it, a float32 sample): per-channel symmetric
    qint8 weights (the README's qconfig).  Quantizers: "in" (x), "e" (the expand conv's output), "h" (after its hardswish), "d" (the
    depthwise conv's output), "da" (after its hardswish), "gap", "f1" (fc1 + ReLU), "f2" (fc2), "gate" (after the hardsigmoid),
    "mul" (the product); the project layer carries its own output fake-quantizer and the FloatFunctional the add's"""
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    torch.manual_seed(41)
    net = V3Block()
    with torch.no_grad():
        net.se.fc2.weight.mul_(8.0)                                        # the hardsigmoid's input then spans both of its bends
    weight = LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                        qscheme=torch.per_channel_symmetric)
    net.qconfig = QConfig(activation=torch.nn.Identity, weight=weight)
    net.train()
    prepare_qat(net, inplace=True)
    x = torch.randn(2, 16, 9, 7) * 2
    net(x)                                                                 # one batch: initialises the weight quantizers
    net.eval()
    T = R.trained_quantizer
    qs = {}
    with torch.no_grad():
        qs["in"] = T(x)
        e = net.expand[0](qs["in"](x))
        qs["e"] = T(e)
        h = net.expand[1](qs["e"](e))
        qs["h"] = T(h)
        d = net.depthwise[0](qs["h"](h))
        qs["d"] = T(d)
        da = net.depthwise[1](qs["d"](d))
        qs["da"] = T(da)
        p = net.se.avgpool(qs["da"](da))
        qs["gap"] = T(p)
        f1 = net.se.fc1(qs["gap"](p))
        qs["f1"] = T(f1)
        f2 = net.se.fc2(qs["f1"](f1))
        qs["f2"] = T(f2)
        gate = net.se.scale_activation(qs["f2"](f2))
        qs["gate"] = T(torch.cat([gate.flatten(), torch.zeros(1)]))         # a gate is positive: its quantizer's range starts at 0
        m = qs["gate"](gate) * qs["da"](da)
        qs["mul"] = T(m)
        out = net.project(qs["mul"](m))
        q_pre = T(out)
        q_add = T(q_pre(out) + qs["in"](x))
    net.se.skip_mul.activation_post_process = qs["mul"]
    net.project.activation_post_process = q_pre
    net.add.activation_post_process = q_add
    return net, qs, x


def convert_v3_block(net, qs, mid):
    """the dense layers by convert_w8a8_q, the depthwise layer by convert_w8a8_depthwise, the global pool by convert_w8a8_pool, the
    three activations and the SE multiply by convert_w8a8_eltwise, the project layer and the add by convert_w8a8_add_q, all on
    disjoint names; the block's and the SE block's forward as they are"""
    from torchlsq.quantized import (convert_w8a8_add_q, convert_w8a8_depthwise, convert_w8a8_eltwise, convert_w8a8_pool, convert_w8a8_q)
    new = convert_w8a8_q(net, {"expand.0": qs["in"], "se.fc1.0": qs["gap"], "se.fc2": qs["f1"]},
                         {"expand.0": qs["e"], "se.fc1.0": qs["f1"], "se.fc2": qs["f2"]}, relu=("se.fc1.0",), mid_dtype=mid)
    new = convert_w8a8_depthwise(new, {"depthwise.0": qs["h"]}, {"depthwise.0": qs["d"]}, mid_dtype=mid, inplace=True)
    new = convert_w8a8_pool(new, {"se.avgpool": qs["gap"]}, mid_dtype=mid, inplace=True)
    new = convert_w8a8_eltwise(new, {"expand.1": (qs["e"], qs["h"]), "depthwise.1": (qs["d"], qs["da"]),
                                     "se.scale_activation": (qs["f2"], qs["gate"])}, {"se.skip_mul": None}, mid_dtype=mid, inplace=True)
    return convert_w8a8_add_q(new, {"add": "project"}, {"project": qs["mul"]}, mid_dtype=mid, inplace=True)


def v3_block_written_out(net, qs, x, mid):
    """the same block as the modules written out on the levels tensor x: (the add's levels, and the intermediate LevelsTensors)"""
    from torchlsq.quantized import (ActivationW8Q, AdaptiveAvgPool2dW8Q, AddW8A8Q, Conv2dW8A8AddQ, Conv2dW8A8Q, DepthwiseConv2dW8A8Q,
                                    MulGateW8Q)
    dev = x.device
    e = Conv2dW8A8Q.from_float(net.expand[0], qs["in"], qs["e"], mid_dtype=mid).to(dev)(x)
    h = ActivationW8Q.from_float(net.expand[1], qs["e"], qs["h"], mid_dtype=mid, device=dev)(e)
    d = DepthwiseConv2dW8A8Q.from_float(net.depthwise[0], qs["h"], qs["d"], mid_dtype=mid).to(dev)(h)
    da = ActivationW8Q.from_float("hardswish", qs["d"], qs["da"], mid_dtype=mid, device=dev)(d)
    p = AdaptiveAvgPool2dW8Q.from_float(net.se.avgpool, qs["gap"], mid_dtype=mid).to(dev)(da)
    f1 = Conv2dW8A8Q.from_float(net.se.fc1[0], qs["gap"], qs["f1"], relu=True, mid_dtype=mid).to(dev)(p)
    f2 = Conv2dW8A8Q.from_float(net.se.fc2, qs["f1"], qs["f2"], mid_dtype=mid).to(dev)(f1)
    gate = ActivationW8Q.from_float(torch.nn.Hardsigmoid(), qs["f2"], qs["gate"], mid_dtype=mid, device=dev)(f2)
    m = MulGateW8Q.from_float(None, qs["mul"], mid_dtype=mid).to(dev)(da, gate)
    project = Conv2dW8A8AddQ.from_float(net.project, qs["mul"], net.add.activation_post_process, mid_dtype=mid).to(dev)
    return AddW8A8Q().add(project(m), x), dict(e=e, h=h, d=d, da=da, gap=p, f1=f1, f2=f2, gate=gate, mul=m)
