"""What tests/test_resadd_w8_cpu.py and tests/test_resadd_w8_gpu.py share: the W8A8 ops that close a residual block
(include/lsq_hip_resadd_w8.h) are DEFINED as existing ops composed -- the float-output op writing a `mid` y, with `pre` the
per-tensor fake-quantize forward on it, `+ residual.dequantize(mid)`, a select, `lsq_levels_per_tensor` -- so the reference here
is that composition, and every comparison is on the bits.

The cases stand on requant_w8_cases.linear_case / conv_case.  With sd the MAD-based deviation of the layer's float32 output (as
in requant_w8_cases.out_quantizer):
  * residual levels clip(rint(z_r + 32 N(0, 1))) of either level type, z_r the middle of the type's range, scale sd / 32: the
    residual weighs as much as the layer, and the sum stays near normal;
  * `pre`, when on, a quantizer of scale sd / 16 with a mid-range zero point: coarser than the output's on purpose;
  * the output quantizer by out_quantizer from the float32 SUM.
`assert_conditions` holds every random case of at least 336 outputs to: assert_not_vacuous as it stands; at least 40 % of the
levels differ from the op without the residual; with `pre` on at least 25 % differ from `pre` off.  (A numpy model of these
recipes: 0.97 / 0.50 of the levels strictly inside without / with ReLU, 0.98 / 0.62 differ from the no-residual op, 0.61 / 0.34
from `pre` off.)
"""
import itertools

import torch

import qlinear_w8_cases as W
import requant_w8_cases as R
from torchlsq.functional import lsq

OPS = torch.ops.torchlsq
NO_PRE = (None, None, (0, 255, 0, 255))
# (pre on, residual level type)
RES_VARIANTS = list(itertools.product((False, True), (torch.uint8, torch.int8)))


def res_id(v):
    return "%s_res%s" % ("pre" if v[0] else "nopre", "u8" if v[1] == torch.uint8 else "i8")


def bulk_sd(v):
    v = v.detach().float().cpu().flatten()
    return 1.4826 * float((v - v.median()).abs().median())


def residual(shape, sd, dtype, seed):
    """(levels of `shape`, scale [1] float32, zero point [1] int32)"""
    lo, hi = W.LEVEL_RANGE[dtype]
    z = (lo + hi + 1) // 2
    g = torch.Generator(device="cpu").manual_seed(seed + 700)
    lv = torch.clamp(torch.round(z + 32 * torch.randn(shape, generator=g)), lo, hi).to(torch.int32).to(dtype)
    return lv, torch.tensor([sd / 32], dtype=torch.float32), torch.tensor([z], dtype=torch.int32)


def pre_quantizer(sd, unsigned):
    lo, hi = (0, 255) if unsigned else (-128, 127)
    s, zp = sd / 16, (lo + hi + 1) // 2
    return torch.tensor([s], dtype=torch.float32), torch.tensor([-zp * s], dtype=torch.float32), (lo, hi, lo, hi)


def dequantize(rl, rs, rz, mid):
    """LevelsTensor.dequantize(mid)"""
    return ((rl.to(torch.float32) - rz.to(torch.float32)) * rs).to(mid)


def fake_quantize(y, psc, psh, prng):
    """step 2 of the definition: `torchlsq.functional.lsq` on a `mid` y.  The CPU kernels have no float16 storage type: there
    the float32 forward on the (exactly converted) values, rounded to float16 once, as the 16-bit kernels compute"""
    if y.dtype == torch.float16 and not y.is_cuda:
        return lsq(y.float(), psc, psh, *prng).to(torch.float16)
    return lsq(y, psc, psh, *prng)


def close(y, c, k):
    """steps 2 to 5 of the definition on a `mid` y; c[k:] = (osc, osh, rng, relu, mid, rl, rs, rz, psc, psh, prng)"""
    osc, osh, rng, relu, mid, rl, rs, rz, psc, psh, prng = c[k:]
    if psc is not None:
        y = fake_quantize(y, psc, psh, prng)
    return R.levels_of(y + dequantize(rl, rs, rz, mid), osc, osh, rng, relu)


def linear_add(lx, s, z, lw, s_w, zw, bias, osc, osh, rng, relu, mid, rl, rs, rz, psc, psh, prng):
    return OPS.lsq_linear_w8_q8_add_q(lx, s, z, lw, s_w, zw, bias, osc, osh, *rng, relu, mid, rl, rs, rz, psc, psh, *prng)


def linear_composed(*c):
    return close(OPS.lsq_linear_w8_q8(*c[:7], c[11]), c, 7)


def conv_add(lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, relu, mid, rl, rs, rz, psc, psh, prng):
    return OPS.lsq_conv2d_w8_q8_add_q(lx, s, z, lw, s_w, zw, bias, *geo, osc, osh, *rng, relu, mid, rl, rs, rz, psc, psh, *prng)


def conv_composed(*c):
    return close(OPS.lsq_conv2d_w8_q8(*c[:7], *c[7], c[12]), c, 8)


def _sum_quantizer(ref, sd, res_variant, out_variant, seed):
    """(pre, the output quantizer from the float32 sum of `ref` (through `pre`) and a residual of the recipe)"""
    pre_on, res_dt = res_variant
    pre = pre_quantizer(sd, res_dt == torch.int8) if pre_on else NO_PRE       # the pre-quantizer's level type: not the residual's
    if pre_on:
        ref = lsq(ref, pre[0], pre[1], *pre[2])
    total = ref + dequantize(*residual(ref.shape, sd, res_dt, seed + 50), torch.float32)
    return pre, R.out_quantizer(total, out_variant[0], out_variant[1])


def linear_case(M, N, K, variant, out_variant, res_variant, seed):
    """the CPU operands of one random case: requant_w8_cases.linear_case's twelve (the output quantizer from the sum) and
    (residual levels [M, N], their scale, their zero point, pre_scale, pre_shift, the pre range)"""
    c = list(R.linear_case(M, N, K, variant, out_variant, seed))
    lx, s, z, lw, s_w, zw, bias = c[:7]
    # everything from 64 rows of the same distribution: a row's constants must not depend on M
    ref = OPS.lsq_linear_w8_q8(W.levels((64, K), *W.LEVEL_RANGE[variant[0]], seed + 2), s, z, lw, s_w, zw, R.f32_bias(bias), torch.float32)
    sd = bulk_sd(ref)
    pre, (c[7], c[8], c[9]) = _sum_quantizer(ref, sd, res_variant, out_variant, seed)
    return tuple(c) + residual((M, N), sd, res_variant[1], seed) + (pre[0], pre[1], pre[2])


def conv_case(geometry, variant, out_variant, res_variant, seed):
    """the same for a convolution: requant_w8_cases.conv_case's thirteen and the six; the residual is a logical
    [B, Cout, OH, OW] tensor in channels-last memory"""
    c = list(R.conv_case(geometry, variant, out_variant, seed))
    lx, s, z, lw, s_w, zw, bias, geo = c[:8]
    ref = OPS.lsq_conv2d_w8_q8(lx, s, z, lw, s_w, zw, R.f32_bias(bias), *geo, torch.float32)
    sd = bulk_sd(ref)
    pre, (c[8], c[9], c[10]) = _sum_quantizer(ref, sd, res_variant, out_variant, seed)
    B, N, OH, OW = ref.shape
    rl, rs, rz = residual((B, OH, OW, N), sd, res_variant[1], seed)
    return tuple(c) + (rl.permute(0, 3, 1, 2), rs, rz, pre[0], pre[1], pre[2])


def differ(a, b):
    return (a != b).double().mean().item()


def assert_conditions(got, case, conv, note=""):
    """the three conditions of the module's docstring, on the CPU result `got` of the CPU case `case`"""
    k = 8 if conv else 7
    rng = case[k + 2]
    R.assert_not_vacuous(got, rng, note)
    plain = (R.conv_q if conv else R.linear_q)(*case[:k + 5])
    assert differ(got, plain) >= 0.40, (note, "only %.1f %% of the levels differ from the op without the residual" % (100 * differ(got, plain)))
    if case[k + 8] is not None:
        off = (conv_add if conv else linear_add)(*case[:k + 8], *NO_PRE)
        assert differ(got, off) >= 0.25, (note, "only %.1f %% of the levels differ from pre off" % (100 * differ(got, off)))


# -------------------------------------------------------------------------------------------------
# a BasicBlock-like module: conv1 (3 x 3, stride 2) + ReLU, conv2 (3 x 3), a 1 x 1 stride-2 downsample, add_relu
# -------------------------------------------------------------------------------------------------
class BasicBlock(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from torch.ao.nn.quantized import FloatFunctional
        self.conv1 = torch.nn.Conv2d(16, 32, 3, stride=2, padding=1)
        self.relu = torch.nn.ReLU()
        self.conv2 = torch.nn.Conv2d(32, 32, 3, padding=1)
        self.downsample = torch.nn.Conv2d(16, 32, 1, stride=2, bias=False)
        self.add_relu = FloatFunctional()

    def forward(self, x):
        identity = self.downsample(x)
        out = self.conv2(self.relu(self.conv1(x)))
        return self.add_relu.add_relu(out, identity)


def basic_block():
    """(the QAT block in eval mode, the quantizers {"in", "mid", "identity"}, a float32 sample x): weights per-channel symmetric
    qint8 (the README's qconfig), conv2 with an output fake-quantizer of its own (`activation_post_process`, the `pre` of the fused
    op) and the FloatFunctional with the add's; the three activation quantizers of the block's input, conv2's input and the
    downsample's output are kept beside the model, as in qconv_w8_cases.qat_conv_model"""
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    torch.manual_seed(12)
    block = BasicBlock()
    weight = LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                        qscheme=torch.per_channel_symmetric)
    block.qconfig = QConfig(activation=torch.nn.Identity, weight=weight)
    block.train()
    prepare_qat(block, inplace=True)
    x = torch.randn(4, 16, 10, 10)
    block(x)                                                               # one batch: initialises the weight quantizers
    block.eval()
    with torch.no_grad():
        q_in = R.trained_quantizer(x)
        xq = q_in(x)
        q_id = R.trained_quantizer(block.downsample(xq))
        q_mid = R.trained_quantizer(block.relu(block.conv1(xq)))
        out = block.conv2(q_mid(block.relu(block.conv1(xq))))
        q_pre = R.trained_quantizer(out)
        q_add = R.trained_quantizer(torch.relu(q_pre(out) + q_id(block.downsample(xq))))
    block.conv2.activation_post_process = q_pre
    block.add_relu.activation_post_process = q_add
    return block, dict({"in": q_in, "mid": q_mid, "identity": q_id}), x


def convert_block(block, qs, mid):
    """conv1 + ReLU and the downsample by convert_w8a8_q, conv2 + add_relu by convert_w8a8_add_q; the block's forward as it is"""
    from torchlsq.quantized import convert_w8a8_add_q, convert_w8a8_q
    new = convert_w8a8_q(block, {"conv1": qs["in"], "downsample": qs["in"]}, {"conv1": qs["mid"], "downsample": qs["identity"]},
                         relu=("conv1",), mid_dtype=mid)
    new.relu = torch.nn.Identity()                                          # conv1's ReLU moved into its kernel
    return convert_w8a8_add_q(new, {"add_relu": "conv2"}, {"conv2": qs["mid"]}, mid_dtype=mid, inplace=True)


def block_written_out(block, qs, x, mid):
    """the same block as the EXISTING modules and ops written out, on the levels tensor x: final levels"""
    from torchlsq.quantized import Conv2dW8A8, Conv2dW8A8Q
    from torchlsq.quantized.modules.packed_linear_a8 import _per_tensor_constants
    dev = x.device
    h = Conv2dW8A8Q.from_float(block.conv1, qs["in"], qs["mid"], relu=True, mid_dtype=mid).to(dev)(x)
    identity = Conv2dW8A8Q.from_float(block.downsample, qs["in"], qs["identity"], mid_dtype=mid).to(dev)(x)
    m = Conv2dW8A8.from_float(block.conv2, qs["mid"]).to(dev)
    y = OPS.lsq_conv2d_w8_q8(h.levels, h.scale, h.zero_point, m.weight_levels, m.weight_scale, m.weight_zero_point, m.bias, [1, 1], [1, 1],
                             [1, 1], mid)
    psc, psh, *prng = _per_tensor_constants(block.conv2.activation_post_process, "pre")
    osc, osh, *orng = _per_tensor_constants(block.add_relu.activation_post_process, "add")
    t = fake_quantize(y, psc.to(dev), psh.to(dev), prng) + identity.dequantize(mid)
    return R.levels_of(t, osc.to(dev), osh.to(dev), orng, True)


def contraction_case():
    """(case, k, the levels with d and p + d rounded one after the other, the levels with the two contracted into one fma):
    float32, no pre, s_w = s_x = 1, so p = I = a_m b_n exactly; residual levels l_r - z_r = k = -I and s_r = 1 + 2^-23, so that
    p + d cancels to what the rounding of d left; output scale 2^-23, zero point 128.  Both models in numpy."""
    import numpy as np
    a, b = torch.arange(1, 12), torch.arange(-11, 12)
    lx, lw = torch.zeros(11, 16, dtype=torch.int8), torch.zeros(23, 16, dtype=torch.int8)
    lx[:, 0], lw[:, 0] = a.to(torch.int8), b.to(torch.int8)
    I = a.reshape(-1, 1) * b.reshape(1, -1)
    k = -I
    s, z = W.act(1.0, 0)
    s_r = np.float32(1.0) + np.float32(2.0 ** -23)
    case = (lx, s, z, lw, torch.ones(23), torch.zeros(23, dtype=torch.int32), None, torch.tensor([2.0 ** -23]),
            torch.tensor([-128 * 2.0 ** -23]), (0, 255, 0, 255), False, torch.float32, k.to(torch.int8), torch.tensor([float(s_r)]),
            torch.zeros(1, dtype=torch.int32)) + NO_PRE
    kf, If = k.numpy().astype(np.float32), I.numpy().astype(np.float32)

    def level(t):
        q = t.astype(np.float32) * np.float32(2.0 ** 23) + np.float32(128)
        return torch.from_numpy(np.rint(np.clip(q, 0, 255)).astype(np.int64))

    two_step = level(If + kf * s_r)                                                      # float32: each step rounded once
    fused = level((kf.astype(np.float64) * np.float64(s_r) + If.astype(np.float64)).astype(np.float32))   # exact, rounded once
    return case, k, two_step, fused
