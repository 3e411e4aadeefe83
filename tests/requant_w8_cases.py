"""What tests/test_requant_w8_cpu.py and tests/test_requant_w8_gpu.py share: the W8A8 ops with an 8-bit output
(include/lsq_hip_requant_w8.h) are DEFINED as three existing ops composed -- the float-output op writing a `mid_dtype` y, a
select, `lsq_levels_per_tensor` -- so the reference here is that composition, and every comparison is on the bits.

Output quantizers are chosen from the data so that no comparison is vacuous: with sd the standard deviation of the float32
result -- taken from the median absolute deviation, sd = 1.4826 MAD as for a normal distribution, because the variants put weight
zero points on the borders of their range and those few columns would dominate a plain standard deviation -- scale sd / 64 and the zero point in the middle of the range without ReLU (about 95 % of the levels strictly inside, both
borders hit), scale sd / 96 and the zero point on quant_min with ReLU (the negative half on quant_min, about 50 % inside).
`assert_not_vacuous` holds every random case to it, on the CPU path's result.
"""
import itertools

import torch

import qlinear_w8_cases as W

MIDS = (torch.float32, torch.bfloat16, torch.float16)
# (unsigned output levels, relu, mid_dtype): every combination
OUT_VARIANTS = list(itertools.product((True, False), (False, True), MIDS))
OPS = torch.ops.torchlsq


def out_id(v):
    return "%s_%s_%s" % ("u8" if v[0] else "i8", "relu" if v[1] else "lin", str(v[2]).replace("torch.", ""))


def out_quantizer(v, unsigned, relu):
    """(out_scale [1], out_shift [1], (quant_min, quant_max, type_min, type_max)) for float32 results v, see above"""
    v = v.detach().float().cpu().flatten()
    sd = 1.4826 * float((v - v.median()).abs().median())      # the standard deviation of the bulk, see the module's docstring
    lo, hi = (0, 255) if unsigned else (-128, 127)
    s = sd / 96 if relu else sd / 64
    zp = lo if relu else (lo + hi + 1) // 2
    return torch.tensor([s], dtype=torch.float32), torch.tensor([-zp * s], dtype=torch.float32), (lo, hi, lo, hi)


def assert_not_vacuous(levels, rng, note=""):
    lv = levels.detach().cpu().to(torch.int64)
    inside = ((lv > rng[0]) & (lv < rng[1])).double().mean().item()
    assert inside >= 0.25, (note, "only %.1f %% of the levels inside the range" % (100 * inside))
    assert bool((lv == rng[0]).any()) and bool((lv == rng[1]).any()), (note, "a border of the range is never hit")


def select(u):
    return torch.where(u < 0, torch.zeros_like(u), u)


def levels_of(u, osc, osh, rng, relu):
    """steps 2 and 3 of the definition on a `mid_dtype` y, through the existing op"""
    lv = OPS.lsq_levels_per_tensor(select(u) if relu else u, osc, osh, *rng, 0)
    return lv.view(torch.uint8) if rng[1] > 127 else lv


def to(device, *tensors):
    return [None if t is None else t.to(device) for t in tensors]


def linear_q(lx, s, z, lw, s_w, zw, bias, osc, osh, rng, relu, mid):
    return OPS.lsq_linear_w8_q8_q(lx, s, z, lw, s_w, zw, bias, osc, osh, *rng, relu, mid)


def linear_composed(lx, s, z, lw, s_w, zw, bias, osc, osh, rng, relu, mid):
    return levels_of(OPS.lsq_linear_w8_q8(lx, s, z, lw, s_w, zw, bias, mid), osc, osh, rng, relu)


def conv_q(lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, relu, mid):
    return OPS.lsq_conv2d_w8_q8_q(lx, s, z, lw, s_w, zw, bias, *geo, osc, osh, *rng, relu, mid)


def conv_composed(lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, relu, mid):
    return levels_of(OPS.lsq_conv2d_w8_q8(lx, s, z, lw, s_w, zw, bias, *geo, mid), osc, osh, rng, relu)


def f32_bias(bias):
    return None if bias is None else bias.float()


def linear_case(M, N, K, variant, out_variant, seed):
    """the CPU operands of one random linear case: (lx, s, z, lw, s_w, zw, bias, osc, osh, rng, relu, mid)"""
    x_dt, zx, w_dt, zeros, _, bias_kind = variant
    unsigned, relu, mid = out_variant
    lw, s_w, zw = W.weight(N, K, w_dt, seed, zeros)
    bias = None if bias_kind is None else W.random_bias(N, torch.float32 if bias_kind == "f32" else mid, seed)
    lx = W.levels((M, K), *W.LEVEL_RANGE[x_dt], seed + 1)
    s, z = W.act(0.0371, zx)
    # the quantizer from 64 rows of the same distribution: a row's quantizer must not depend on M
    ref = OPS.lsq_linear_w8_q8(W.levels((64, K), *W.LEVEL_RANGE[x_dt], seed + 2), s, z, lw, s_w, zw, f32_bias(bias), torch.float32)
    osc, osh, rng = out_quantizer(ref, unsigned, relu)
    return (lx, s, z, lw, s_w, zw, bias, osc, osh, rng, relu, mid)


def conv_case(geometry, variant, out_variant, seed):
    """the CPU operands of one random convolution case: (lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, relu, mid)"""
    import qconv_w8_cases as V
    B, Cin, H, Wd, N, k, st, p, d = geometry
    x_dt, zx, w_dt, zeros, _, bias_kind = variant
    unsigned, relu, mid = out_variant
    lw, s_w, zw = V.conv_weight(N, Cin, k, w_dt, seed, zeros)
    bias = None if bias_kind is None else W.random_bias(N, torch.float32 if bias_kind == "f32" else mid, seed)
    lx = V.x_levels(B, Cin, H, Wd, x_dt, seed + 1)
    s, z = W.act(0.0371, zx)
    geo = (list(st), list(p), list(d))
    ref = OPS.lsq_conv2d_w8_q8(lx, s, z, lw, s_w, zw, f32_bias(bias), *geo, torch.float32)
    osc, osh, rng = out_quantizer(ref, unsigned, relu)
    return (lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, relu, mid)


def trained_quantizer(sample):
    """a per-tensor quint8 LSQFakeQuantizer that has seen `sample` and whose scale and shift are then set to cover the sample's
    range (the scale and shift of a quantizer are learned in the backward pass, which no test here runs), observer off, eval"""
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    q = LSQFakeQuantizer(observer=MovingAverageMinMaxObserver, otype="activation")
    q.train()
    q(sample)
    lo, hi = float(sample.min()), float(sample.max())
    with torch.no_grad():
        q.scale.fill_((hi - lo) / (q.quant_max - q.quant_min))
        q.shift.fill_(lo)
    q.disable_observer()
    return q.eval()
