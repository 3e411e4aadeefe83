"""What tests/test_norm_w8_cpu.py and tests/test_norm_w8_gpu.py share: LayerNorm and RMSNorm on 8-bit levels
(include/lsq_hip_norm_w8.h).  The CPU path of the ops is the definition; `np_norm` restates it in numpy (np.int64 sums, np.float32
steps one at a time, explicit roundings to mid_dtype) and `f64_norm` is the norm of the dequantized values in float64.  GPU against
CPU is `torch.equal`: there is no tolerance between the two anywhere in the three files.

Inputs are built so that no comparison is vacuous: each row has a mean uniform in 0..255 and a spread uniform in 1..80 levels,
rounded and clamped (an int8 row holds the same levels less 128); w = 1 + 0.2 N(0, 1), bias = 0.3 N(0, 1); the output quantizer comes
from the CPU path's float32 result by `requant_w8_cases.out_quantizer`: its form without ReLU (zero point in the middle of the range,
scale sd / 64) wherever the normalised values have both signs -- every LayerNorm case, and RMSNorm with a mid-range zero point.
RMSNorm with the zero point at the low end (0 or 3 of 0..255) has no negative t, so no level below a mid-range zero point can
be reached: those cases take the quantizer's other form (zero point on quant_min, scale sd / 96), see `one_sided`; the conditions
are the same.  `assert_conditions` holds every
levels-out case of at least 1000 outputs to `assert_not_vacuous` (at least 25 % of the levels strictly inside the range, both
borders hit) and to at least 40 % of the levels changing when w is rolled by one channel.
"""
import numpy as np
import torch

import requant_w8_cases as R

OPS = torch.ops.torchlsq
MIDS = R.MIDS
LEVEL_DTYPES = (torch.uint8, torch.int8)
KINDS = ("layer", "rms")
S_X = 0.02
EPS = {"layer": 1e-5, "rms": 1e-6}


def name(dtype):
    return str(dtype).replace("torch.", "")


def one(v, dtype=torch.float32):
    return torch.tensor([v], dtype=dtype)


def bits(t):
    """a floating tensor as integers, for torch.equal on the bits"""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16) if t.is_floating_point() else t


# -------------------------------------------------------------------------------------------------
# inputs
# -------------------------------------------------------------------------------------------------
def rows(R_, C, seed=0, dtype=torch.uint8):
    """[R_, C] levels: a row mean uniform in 0..255, a row spread uniform in 1..80, rounded and clamped"""
    g = torch.Generator().manual_seed(7000 + 131 * seed + 17 * R_ + C)
    mean = torch.rand(R_, 1, generator=g) * 255
    spread = 1 + torch.rand(R_, 1, generator=g) * 79
    lv = (mean + spread * torch.randn(R_, C, generator=g)).round().clamp(0, 255)
    return as_dtype(lv.to(torch.uint8), dtype)


def rows_for(C):
    """the rows of a levels-out case: at least 4000 outputs and at least 64 rows.  An RMSNorm row whose mean lies far from the
    zero point has all its values near +1 or -1; the borders of the output range are reached by the rows whose mean lies near it,
    about one in ten, so a case needs a few of them (measured on the CPU path over 144 RMSNorm cases: with 64 rows every one meets
    the conditions, with 24 rows one does not)"""
    return max(64, 4000 // C + 1)


def as_dtype(u8, dtype):
    """uint8 levels as they are, or the same levels less 128 as int8"""
    return u8 if dtype == torch.uint8 else (u8.to(torch.int16) - 128).to(torch.int8)


def params(C, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(9000 + seed + C)
    return (1 + 0.2 * torch.randn(C, generator=g)).to(dtype), (0.3 * torch.randn(C, generator=g)).to(dtype)


def zero_for(dtype, z_u8):
    """the zero point of an int8 tensor that holds the uint8 levels less 128"""
    return one(z_u8 if dtype == torch.uint8 else z_u8 - 128, torch.int32)


PLANTED = ("one_zero_in_255s", "one_8_in_7s", "alternating_0_255", "constant", "int8_extremes")


def planted(C, dtype=torch.uint8, seed=0):
    """([5 + 3, C] levels: the five integer-statistics rows between random ones, the planted rows' indices by name).  A float32
    E[x^2] - E[x]^2 or a 32-bit V gets these wrong; `int8_extremes` alternates -128 / 127 for int8 levels (0 / 255 read as uint8,
    in the other phase than `alternating_0_255`)."""
    x = rows(8, C, 40 + seed)
    g = torch.Generator().manual_seed(40 + seed + C)
    at = {}
    x[1] = 255
    x[1, int(torch.randint(0, C, (1,), generator=g))] = 0
    at["one_zero_in_255s"] = 1
    x[2] = 7
    x[2, int(torch.randint(0, C, (1,), generator=g))] = 8
    at["one_8_in_7s"] = 2
    x[4] = torch.tensor([0, 255], dtype=torch.uint8).repeat((C + 1) // 2)[:C]
    at["alternating_0_255"] = 4
    x[5] = 93
    at["constant"] = 5
    x[6] = torch.tensor([255, 0], dtype=torch.uint8).repeat((C + 1) // 2)[:C]
    at["int8_extremes"] = 6
    return as_dtype(x, dtype), at


# -------------------------------------------------------------------------------------------------
# the ops
# -------------------------------------------------------------------------------------------------
def run(kind, x, s_x, zx, w, b, eps, out_q, mid):
    """the op on x's device; out_q = (out_scale, out_shift, range) or None for floats"""
    base = "lsq_layer_norm_w8_q8" if kind == "layer" else "lsq_rms_norm_w8_q8"
    if out_q is None:
        return getattr(OPS, base)(x, s_x, zx, w, b, eps, mid)
    return getattr(OPS, base + "_q")(x, s_x, zx, w, b, eps, out_q[0], out_q[1], *out_q[2], mid)


def to(device, *tensors):
    return [None if t is None else t.to(device) for t in tensors]


def run_on(device, kind, x, s_x, zx, w, b, eps, out_q, mid):
    q = None if out_q is None else (out_q[0].to(device), out_q[1].to(device), out_q[2])
    return run(kind, *to(device, x, s_x, zx, w, b), eps, q, mid)


def one_sided(kind, z_u8):
    """whether no normalised value of the case is negative (before w and bias): RMSNorm of levels that lie above their zero point"""
    return kind == "rms" and z_u8 < 64


def quantizer_for(kind, x, s_x, zx, w, b, eps, unsigned, low_zero=False):
    """the output quantizer from the CPU path's float32 result; `low_zero`: its form with the zero point on quant_min"""
    return R.out_quantizer(run(kind, x, s_x, zx, w, b, eps, None, torch.float32), unsigned, relu=low_zero)


def assert_conditions(kind, x, s_x, zx, w, b, eps, out_q, mid, levels, note=""):
    """on the CPU path's levels of a case of at least 1000 outputs"""
    if levels.numel() < 1000:
        return
    R.assert_not_vacuous(levels, out_q[2], note)
    if w is not None and w.numel() > 1:
        rolled = run(kind, x, s_x, zx, torch.roll(w, 1), b, eps, out_q, mid)
        changed = (rolled != levels).double().mean().item()
        assert changed >= 0.40, (note, "only %.1f %% of the levels change when w is rolled by one channel" % (100 * changed))


# -------------------------------------------------------------------------------------------------
# restatements
# -------------------------------------------------------------------------------------------------
def np_round_mid(a, mid):
    """float32 numpy values rounded to `mid` (round to nearest even) and widened again"""
    a = np.asarray(a, dtype=np.float32)
    if mid == torch.float32:
        return a
    if mid == torch.float16:
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(a), a, r)


def np_levels(u, out_scale, out_shift, rng):
    """lsq_math.hpp's level() in np.float32 steps; a NaN goes to quant_min"""
    f = np.float32
    qmin, qmax, tmin, tmax = (f(v) for v in rng)
    s = max(abs(f(out_scale)), f(np.finfo(np.float32).eps))
    inv_s = f(1) / s
    zp = np.rint(np.fmin(tmax, np.fmax(tmin, -f(out_shift) * inv_s)))
    c = u.astype(f) * inv_s
    c = c + zp
    lv = np.rint(np.fmin(qmax, np.fmax(qmin, c))).astype(np.int64)
    return lv.astype(np.uint8) if rng[1] > 127 or rng[3] > 127 else lv.astype(np.int8)


def np_norm(kind, x, s_x, zx, w, b, eps, mid, stats=None):
    """the definition in numpy: u (float32 values of `mid`) of [R, C] levels x.  `stats="float32"` (LayerNorm): what the definition
    is NOT, the float32 shortcut on the dequantized values v = (b - zx) s_x: mean = sum v / C, var = sum v^2 / C - mean^2,
    t = (v - mean) / sqrt(var + eps)"""
    f = np.float32
    lv = x.numpy().astype(np.int64)
    C = lv.shape[-1]
    fC = f(C)
    s = f(float(s_x))
    e = f(eps) / (s * s)
    if kind == "layer":
        S1 = lv.sum(-1, keepdims=True)
        S2 = (lv * lv).sum(-1, keepdims=True)
        V = C * S2 - S1 * S1
        num = C * lv - S1
        var = V.astype(f) / (fC * fC)
    else:
        num = lv - int(zx)
        var = (num * num).sum(-1, keepdims=True).astype(f) / fC
    with np.errstate(divide="ignore", invalid="ignore"):
        r = f(1) / np.sqrt(var + e)
        rc = r / fC if kind == "layer" else r
        t = num.astype(f) * rc.astype(f)
        if stats == "float32":
            v = (lv - int(zx)).astype(f) * s
            mean = v.sum(-1, keepdims=True, dtype=f) / fC
            short = (v * v).sum(-1, keepdims=True, dtype=f) / fC - mean * mean
            t = (v - mean) / np.sqrt(short + f(eps))
        if w is not None:
            t = t * w.float().numpy()
        if b is not None:
            t = t + b.float().numpy()
    return np_round_mid(t, mid)


def f64_norm(kind, x, s_x, zx, w, b, eps):
    """(a, t w, bias) in float64: the norm in (near) real arithmetic of the dequantized values (b - zx) s_x, with s_x, eps, w and
    bias taken as the float32 numbers given"""
    d = np.float64
    s = d(np.float32(float(s_x)))
    v = (x.numpy().astype(d) - d(int(zx))) * s
    e = d(np.float32(eps))
    if kind == "layer":
        c = v - v.mean(-1, keepdims=True)
        t = c / np.sqrt((c * c).mean(-1, keepdims=True) + e)
    else:
        t = v / np.sqrt((v * v).mean(-1, keepdims=True) + e)
    tw = t * (w.float().numpy().astype(d) if w is not None else 1.0)
    bias = b.float().numpy().astype(d) if b is not None else np.zeros(1)
    return tw + bias, tw, bias


# -------------------------------------------------------------------------------------------------
# the plan by the rule of include/lsq_hip_norm_w8.h
# -------------------------------------------------------------------------------------------------
def choose_lp(C):
    best = None
    for P in range(1, 9):
        lanes = -(-(C // 16) // P)
        L = 4
        while L < lanes:
            L *= 2
        if L <= 64 and (best is None or L - lanes < best[0]):
            best = (L - lanes, L, P)
    return best[1], best[2]


def expected_plan(R_, C, aligned=True, has_w=True, has_b=True, cus=256):
    if not (aligned and C % 16 == 0 and C <= 8192):
        return dict(family="generic", grid=-(-R_ // 4), block=256, lanes_per_row=64, packets_per_lane=0, rows_per_workgroup=4,
                    params="none", lds_bytes=0)
    L, P = choose_lp(C)
    G, K = 256 // L, 8
    while K > 1 and -(-R_ // (G * K)) < 2 * cus:
        K //= 2
    params = "none" if not (has_w or has_b) else ("registers" if P == 1 else "lds")
    return dict(family="packets", grid=-(-R_ // (G * K)), block=256, lanes_per_row=L, packets_per_lane=P, rows_per_workgroup=G * K,
                params=params, lds_bytes=4 * C * (int(has_w) + int(has_b)) if params == "lds" else 0)


def every_lp():
    """{(L, P): the smallest C that the plan serves with it} over every C the packets family takes"""
    seen = {}
    for C in range(16, 8192 + 1, 16):
        seen.setdefault(choose_lp(C), C)
    return seen


# -------------------------------------------------------------------------------------------------
# the product and the add are rounded apart: inputs where contracting t w + bias into one fma changes a level
# -------------------------------------------------------------------------------------------------
NO_FMA_SEEDS = (1, 2, 3, 4, 5, 6)
NO_FMA_SCALE = 2.0 ** -10          # the output quantizer: scale 2^-10, shift 0, so level = rne(a 2^10) exactly


def no_fma_case(seed, kind="layer"):
    """(x [1, 16] uint8, w, bias, the channels that are witnesses, the levels a contracted t w + bias would give there).  For each
    channel, with t the definition's float32 t and p = t w exact (48 bits, held in float64): bias = T - fl(p) with T = 0.5 * 2^-10
    where p > fl(p) and T = 1.5 * 2^-10 where p < fl(p).  Where that bias is a float32 number, fl(p) + bias is T exactly, a tie,
    which goes to the even level (0 resp. 2); one fma rounds p + bias, which lies beyond the tie, to level 1."""
    g = torch.Generator().manual_seed(5000 + seed)
    x = rows(1, 16, 300 + seed)
    w = (1 + 0.2 * torch.randn(16, generator=g)).to(torch.float32)
    t = run(kind, x, one(S_X), one(128, torch.int32), None, None, EPS[kind], None, torch.float32).numpy().astype(np.float64)[0]
    p = t * w.numpy().astype(np.float64)
    flp = p.astype(np.float32).astype(np.float64)
    T = np.where(p > flp, 0.5, 1.5) * NO_FMA_SCALE
    bias64 = T - flp
    bias = bias64.astype(np.float32)
    witness = (bias.astype(np.float64) == bias64) & (p != flp)
    witness &= (flp.astype(np.float32) + bias).astype(np.float64) == T            # the separate add lands on the tie exactly
    fused = np.rint((p + bias.astype(np.float64)).astype(np.float32).astype(np.float64) / NO_FMA_SCALE).astype(np.int64)
    bias = np.where(witness, bias, np.float32(0))
    return x, w, torch.from_numpy(bias.astype(np.float32)), np.nonzero(witness)[0], fused[witness]


# -------------------------------------------------------------------------------------------------
# a ConvNeXt-style block and a token block
# -------------------------------------------------------------------------------------------------
class LayerNorm2d(torch.nn.LayerNorm):
    """torchvision's: LayerNorm over C of a [B, C, H, W] tensor"""

    def forward(self, x):
        return torch.nn.functional.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps).permute(0, 3, 1, 2)


class CNBlock(torch.nn.Module):
    """ConvNeXt's block: depthwise 7 x 7 -> LayerNorm over C -> 1 x 1 -> GELU -> 1 x 1 -> + x"""

    def __init__(self, channels=16, hidden=64):
        super().__init__()
        self.dw = torch.nn.Conv2d(channels, channels, 7, padding=3, groups=channels)
        self.norm = LayerNorm2d(channels, eps=1e-6)
        self.pw1 = torch.nn.Conv2d(channels, hidden, 1)
        self.act = torch.nn.GELU()
        self.pw2 = torch.nn.Conv2d(hidden, channels, 1)
        self.add = torch.ao.nn.quantized.FloatFunctional()

    def forward(self, x):
        return self.add.add(self.pw2(self.act(self.pw1(self.norm(self.dw(x))))), x)


class TokenBlock(torch.nn.Module):
    """the seam of a ViT block: projection + residual -> LayerNorm -> fc1"""

    def __init__(self, dim=48, hidden=96):
        super().__init__()
        self.proj = torch.nn.Linear(dim, dim)
        self.add = torch.ao.nn.quantized.FloatFunctional()
        self.norm = torch.nn.LayerNorm(dim)
        self.fc1 = torch.nn.Linear(dim, hidden)

    def forward(self, x):
        return self.fc1(self.norm(self.add.add(self.proj(x), x)))


def _prepared(net, x):
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    weight = LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                        qscheme=torch.per_channel_symmetric)
    net.qconfig = QConfig(activation=torch.nn.Identity, weight=weight)
    net.train()
    prepare_qat(net, inplace=True)
    net(x)                                                                 # one batch: initialises the weight quantizers
    return net.eval()


def _norm_params(norm, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(norm.weight.shape, generator=g))
        norm.bias.copy_(0.3 * torch.randn(norm.bias.shape, generator=g))


def cn_block():
    """(the QAT block in eval mode, the per-tensor quint8 activation quantizers beside it, a float32 sample).  Quantizers: "in" (x),
    "d" (the depthwise conv's output), "n" (the norm's), "p1" (the first 1 x 1's), "g" (after the GELU); the second 1 x 1 carries its
    own output fake-quantizer and the FloatFunctional the add's"""
    torch.manual_seed(43)
    net = CNBlock()
    _norm_params(net.norm, 44)
    x = torch.randn(2, 16, 9, 7) * 2
    net = _prepared(net, x)
    T, qs = R.trained_quantizer, {}
    with torch.no_grad():
        qs["in"] = T(x)
        d = net.dw(qs["in"](x))
        qs["d"] = T(d)
        n = net.norm(qs["d"](d))
        qs["n"] = T(n)
        p1 = net.pw1(qs["n"](n))
        qs["p1"] = T(p1)
        gl = net.act(qs["p1"](p1))
        qs["g"] = T(gl)
        out = net.pw2(qs["g"](gl))
        q_pre = T(out)
        q_add = T(q_pre(out) + qs["in"](x))
    net.pw2.activation_post_process = q_pre
    net.add.activation_post_process = q_add
    return net, qs, x


def convert_cn_block(net, qs, mid):
    from torchlsq.quantized import convert_w8a8_add_q, convert_w8a8_depthwise, convert_w8a8_eltwise, convert_w8a8_norm, convert_w8a8_q
    new = convert_w8a8_depthwise(net, {"dw": qs["in"]}, {"dw": qs["d"]}, mid_dtype=mid)
    new = convert_w8a8_norm(new, {"norm": qs["n"]}, channels_first=("norm",), mid_dtype=mid, inplace=True)
    new = convert_w8a8_q(new, {"pw1": qs["n"]}, {"pw1": qs["p1"]}, mid_dtype=mid, inplace=True)
    new = convert_w8a8_eltwise(new, {"act": (qs["p1"], qs["g"])}, mid_dtype=mid, inplace=True)
    return convert_w8a8_add_q(new, {"add": "pw2"}, {"pw2": qs["g"]}, mid_dtype=mid, inplace=True)


def cn_block_written_out(net, qs, x, mid):
    """the same block as the modules written out on the levels tensor x: (the add's levels, the intermediate LevelsTensors)"""
    from torchlsq.quantized import ActivationW8Q, AddW8A8Q, Conv2dW8A8AddQ, Conv2dW8A8Q, DepthwiseConv2dW8A8Q, LayerNormW8Q
    dev = x.device
    d = DepthwiseConv2dW8A8Q.from_float(net.dw, qs["in"], qs["d"], mid_dtype=mid).to(dev)(x)
    n = LayerNormW8Q.from_float(net.norm, qs["n"], mid_dtype=mid, channels_first=True).to(dev)(d)
    p1 = Conv2dW8A8Q.from_float(net.pw1, qs["n"], qs["p1"], mid_dtype=mid).to(dev)(n)
    gl = ActivationW8Q.from_float(net.act, qs["p1"], qs["g"], mid_dtype=mid, device=dev)(p1)
    pw2 = Conv2dW8A8AddQ.from_float(net.pw2, qs["g"], net.add.activation_post_process, mid_dtype=mid).to(dev)
    return AddW8A8Q().add(pw2(gl), x), dict(d=d, n=n, p1=p1, g=gl)


def token_block():
    """(the QAT block in eval mode, quantizers "in" (x), "a" (the add's), "n" (the norm's output), a float32 sample [2, 10, 48]); fc1
    gives floats"""
    torch.manual_seed(47)
    net = TokenBlock()
    _norm_params(net.norm, 48)
    x = torch.randn(2, 10, 48) * 2
    net = _prepared(net, x)
    T, qs = R.trained_quantizer, {}
    with torch.no_grad():
        qs["in"] = T(x)
        out = net.proj(qs["in"](x))
        q_pre = T(out)
        a = q_pre(out) + qs["in"](x)
        qs["a"] = T(a)
        n = net.norm(qs["a"](a))
        qs["n"] = T(n)
        qs["f"] = T(net.fc1(qs["n"](n)))
    net.proj.activation_post_process = q_pre
    net.add.activation_post_process = qs["a"]
    return net, qs, x


def convert_token_block(net, qs, mid):
    from torchlsq.quantized import convert_w8a8_add_q, convert_w8a8_norm, convert_w8a8_q
    new = convert_w8a8_add_q(net, {"add": "proj"}, {"proj": qs["in"]}, mid_dtype=mid)
    new = convert_w8a8_norm(new, {"norm": qs["n"]}, mid_dtype=mid, inplace=True)
    return convert_w8a8_q(new, {"fc1": qs["n"]}, {"fc1": qs["f"]}, mid_dtype=mid, inplace=True)


def token_block_written_out(net, qs, x, mid):
    from torchlsq.quantized import AddW8A8Q, LayerNormW8Q, LinearW8A8AddQ, LinearW8A8Q
    dev = x.device
    proj = LinearW8A8AddQ.from_float(net.proj, qs["in"], net.add.activation_post_process, mid_dtype=mid).to(dev)
    a = AddW8A8Q().add(proj(x), x)
    n = LayerNormW8Q.from_float(net.norm, qs["n"], mid_dtype=mid).to(dev)(a)
    return LinearW8A8Q.from_float(net.fc1, qs["n"], qs["f"], mid_dtype=mid).to(dev)(n), dict(a=a, n=n)
