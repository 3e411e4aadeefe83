"""What tests/test_dwconv_w8_cpu.py and tests/test_dwconv_w8_gpu.py share: the W8A8 depthwise conv2d on 8-bit levels
(include/lsq_hip_dwconv_w8.h).  The CPU path of the ops is the definition; it is pinned by existing ops -- with the depthwise
weight embedded in a dense [C, C, kh, kw] weight whose off-diagonal entries hold the level zw[n] (they contribute (lw - zw) = 0),
`lsq_conv2d_w8_q8` yields the same exact integer and the same rounded fp32 steps -- and by a numpy restatement.  Every comparison
is on the bits.

Inputs stand on the existing helpers: qlinear_w8_cases.weight(C, kh kw) reshaped, qconv_w8_cases.x_levels and VARIANTS,
requant_w8_cases.out_quantizer taken from the float32 result without activation.  ReLU6 has a fixed bound, so for it the input
scale is first set such that the bulk of the results has the standard deviation 4 (about 43 % of a normal distribution inside
(0, 6), 7 % above), and the output scale is capped at 6 / (quant_max - quant_min): the value 6 then lands on quant_max and
both borders of the range are hit.  `assert_conditions` holds every random levels-out case of at least 1000 outputs to
requant_w8_cases.assert_not_vacuous and to two conditions of its own: at least 40 % of the levels change when each channel's taps
are rolled by one, and when the weights are rolled by one channel -- a kernel that reads the wrong tap or the wrong channel's
weights cannot pass.
"""
import itertools

import numpy as np
import torch

import qconv_w8_cases as V
import qlinear_w8_cases as W
import requant_w8_cases as R
import resadd_w8_cases as A

OPS = torch.ops.torchlsq
CL = torch.channels_last
MIDS = R.MIDS
ACTS = (0, 1, 2)
# (B, C, H, W, kernel, stride, padding, dilation): the smallest at which each mechanism can go wrong
GEOMETRIES = [
    (2, 16, 9, 7, (3, 3), (1, 1), (1, 1), (1, 1)),      # unrolled stride 1, every border, OW = 7 is no multiple of P
    (2, 32, 9, 8, (3, 3), (2, 2), (1, 1), (1, 1)),      # unrolled stride 2, asymmetric right border
    (1, 48, 11, 9, (5, 5), (1, 1), (2, 2), (1, 1)),     # 5 x 5
    (2, 16, 7, 9, (3, 3), (1, 1), (2, 2), (2, 2)),      # dilation, the loop
    (1, 16, 6, 10, (1, 3), (2, 1), (0, 1), (1, 1)),     # asymmetric kernel
    (2, 16, 3, 3, (3, 3), (1, 1), (2, 2), (1, 1)),      # outputs that see padding only
]
VARIANTS = V.VARIANTS
# (output: True uint8 levels, False int8 levels, None floats; mid_dtype; act)
OUT_VARIANTS = list(itertools.product((True, False, None), MIDS, ACTS))


def geom_id(g):
    return "B%d_C%d_%dx%d_k%dx%d_s%d%d_p%d%d_d%d%d" % (g[0], g[1], g[2], g[3], *g[4], *g[5], *g[6], *g[7])


def out_hw(g):
    return V.out_hw(g[2], g[3], g[4], g[5], g[6], g[7])


def dw_weight(C, kernel, dtype=torch.int8, seed=0, zeros=None, exact=False):
    """(levels [kh, kw, C] of dtype, tap-major, scale [C] float32, zero point [C] int32)"""
    kh, kw = kernel
    lw, s, z = W.weight(C, kh * kw, dtype, seed, zeros, exact)
    return lw.reshape(C, kh, kw).permute(1, 2, 0).contiguous(), s, z


def dense_embedding(lw, zw):
    """the [C, C, kh, kw] weight (channels-last) of a groups == 1 convolution that computes the depthwise one: the tap-major
    depthwise levels on the diagonal, the level zw[n] everywhere else in row n"""
    kh, kw, C = lw.shape
    dense = zw.to(lw.dtype).reshape(C, 1, 1, 1).expand(C, C, kh, kw).clone()
    idx = torch.arange(C)
    dense[idx, idx] = lw.permute(2, 0, 1)
    return dense.contiguous(memory_format=CL)


def act_of(u, act):
    """the selects of the contract on a mid tensor"""
    if act >= 1:
        u = torch.where(u < 0, torch.zeros_like(u), u)
    if act == 2:
        u = torch.where(u > 6, torch.full_like(u, 6), u)
    return u


def out_quantizer(v, unsigned, act):
    osc, osh, rng = R.out_quantizer(v, unsigned, act >= 1)
    if act == 2:
        s = min(float(osc), 6.0 / (rng[1] - rng[0]))
        osc, osh = torch.tensor([s], dtype=torch.float32), torch.tensor([-rng[0] * s], dtype=torch.float32)
    return osc, osh, rng


def case(geometry, variant, out_variant, seed=0):
    """the CPU operands of one random case: (lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, act, mid); osc, osh, rng are None
    for the floating output"""
    B, C, H, Wd, k, st, p, d = geometry
    x_dt, zx, w_dt, zeros, _, bias_kind = variant
    unsigned, mid, act = out_variant
    lw, s_w, zw = dw_weight(C, k, w_dt, seed, zeros)
    bias = None if bias_kind is None else W.random_bias(C, torch.float32 if bias_kind == "f32" else mid, seed)
    lx = V.x_levels(B, C, H, Wd, x_dt, seed + 1)
    s, z = W.act(0.0371, zx)
    geo = (list(st), list(p), list(d))
    ref = OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_w, zw, R.f32_bias(bias), *geo, 0, torch.float32)
    if act == 2:
        # ReLU6 has a fixed bound: the input scale is set so that the bulk of the results has the standard deviation 4 (about 43 %
        # of a normal distribution inside (0, 6) and 7 % above 6), whatever the variant's zero points make of the sums
        v = ref.flatten()
        s = s * (4.0 / (1.4826 * float((v - v.median()).abs().median())))
        ref = OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_w, zw, R.f32_bias(bias), *geo, 0, torch.float32)
    if unsigned is None:
        return (lx, s, z, lw, s_w, zw, bias, geo, None, None, None, act, mid)
    osc, osh, rng = out_quantizer(ref, unsigned, act)
    return (lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, act, mid)


def run(c, device=None, out=None):
    """the op of a case, on `device` (None: where the case's tensors are)"""
    lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, act, mid = c
    t = (lx, s, z, lw, s_w, zw, bias, osc, osh)
    if device is not None:
        lx, s, z, lw, s_w, zw, bias, osc, osh = R.to(device, *t)
    if rng is None:
        return OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_w, zw, bias, *geo, act, mid)
    return OPS.lsq_dwconv2d_w8_q8_q(lx, s, z, lw, s_w, zw, bias, *geo, osc, osh, *rng, act, mid)


def composed(c, device=None):
    """the same through the EXISTING ops on the dense embedding: lsq_conv2d_w8_q8 writing a mid y, the selects, and
    lsq_levels_per_tensor (or the activated mid tensor itself)"""
    lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, act, mid = c
    dense = dense_embedding(lw, zw)
    t = (lx, s, z, dense, s_w, zw, bias, osc, osh)
    if device is not None:
        lx, s, z, dense, s_w, zw, bias, osc, osh = R.to(device, *t)
    u = act_of(OPS.lsq_conv2d_w8_q8(lx, s, z, dense, s_w, zw, bias, *geo, mid), act)
    if rng is None:
        return u
    return R.levels_of(u, osc, osh, rng, False)


def bits(t):
    """a tensor as integers of its width, for torch.equal on the bits"""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.contiguous().view(torch.int16)
    return t


def assert_conditions(got, c, note=""):
    """the non-vacuity conditions of the module's docstring on the CPU result `got` of the levels-out CPU case `c`; returns
    (inside share, tap-roll share, channel-roll share)"""
    lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, act, mid = c
    R.assert_not_vacuous(got, rng, note)
    kh, kw, C = lw.shape
    taps = run((lx, s, z, lw.reshape(kh * kw, C).roll(1, 0).reshape(kh, kw, C), s_w, zw, bias, geo, osc, osh, rng, act, mid))
    chans = run((lx, s, z, lw.roll(1, 2), s_w.roll(1), zw.roll(1), bias, geo, osc, osh, rng, act, mid))
    t, ch = A.differ(got, taps), A.differ(got, chans)
    if kh * kw > 1:
        assert t >= 0.40, (note, "only %.1f %% of the levels change when each channel's taps are rolled by one" % (100 * t))
    assert ch >= 0.40, (note, "only %.1f %% of the levels change when the weights are rolled by one channel" % (100 * ch))
    lv = got.to(torch.int64)
    return ((lv > rng[0]) & (lv < rng[1])).double().mean().item(), t, ch


def numpy_value(lx, s_x, zx, lw, s_w, zw, bias, geo):
    """v of the contract as np.float32 [B, C, OH, OW], tap by tap: int64 sums over the taps inside x, then np.float32 steps"""
    (sh, sw), (ph, pw), (dh, dw) = geo
    x = lx.cpu().numpy().astype(np.int64) - int(zx)
    w = lw.cpu().numpy().astype(np.int64) - zw.cpu().numpy().astype(np.int64).reshape(1, 1, -1)
    B, C, H, Wd = x.shape
    kh, kw, _ = w.shape
    OH = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    OW = (Wd + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    I = np.zeros((B, C, OH, OW), dtype=np.int64)
    for oh in range(OH):
        for ow in range(OW):
            for i in range(kh):
                for j in range(kw):
                    ih, iw = oh * sh - ph + i * dh, ow * sw - pw + j * dw
                    if 0 <= ih < H and 0 <= iw < Wd:
                        I[:, :, oh, ow] += x[:, :, ih, iw] * w[i, j].reshape(1, C)
    v = (s_w.cpu().numpy().astype(np.float32).reshape(1, C, 1, 1) * I.astype(np.float32)) * np.float32(float(s_x))
    if bias is not None:
        v = v + bias.float().cpu().numpy().reshape(1, C, 1, 1)
    return v.astype(np.float32), I


def numpy_levels(u, osc, osh, rng):
    """lsq_math.hpp's level() in np.float32 steps on float32 values u: int64 levels"""
    qmin, qmax, tmin, tmax = (np.float32(v) for v in rng)
    s = np.maximum(np.abs(np.float32(float(osc))), np.float32(np.finfo(np.float32).eps))
    inv = np.float32(1.0) / s
    zp = np.rint(np.minimum(tmax, np.maximum(tmin, -np.float32(float(osh)) * inv)))
    t = u.astype(np.float32) * inv + zp
    q = np.rint(np.minimum(qmax, np.maximum(qmin, t)))
    return np.where(np.isnan(t), qmin, q).astype(np.int64)


def expected_plan(B, C, OH, OW, kernel, stride, dilation, aligned=True, y_aligned=True, pix=(1, 1), cus=256):
    """(family, pixels per lane, grid, unrolled window, unrolled stride) by the rule of include/lsq_hip_dwconv_w8.h; `pix`: the
    library's pixels per lane of the unrolled kernels at stride 1 and 2"""
    if not (aligned and y_aligned) or C % 16:
        return "generic", 1, -(-B * OH * OW * C // 256), 0, 0
    P, K, S = 1, 0, 0
    if tuple(kernel) == (3, 3) and tuple(dilation) == (1, 1) and tuple(stride) in ((1, 1), (2, 2)):
        K, S = 3, stride[0]
        P = pix[S - 1]
        while P > 1 and -(-(B * OH * -(-OW // P) * (C // 16)) // 256) < 2 * cus:
            P //= 2
    return "packets", P, -(-(B * OH * -(-OW // P) * (C // 16)) // 256), K, S


class InvertedResidual(torch.nn.Module):
    """MobileNetV2's block at stride 1: 1 x 1 expand + ReLU -> depthwise 3 x 3 + ReLU6 -> 1 x 1 project -> + x"""

    def __init__(self, channels=16, expand=3):
        super().__init__()
        hidden = channels * expand
        self.expand = torch.nn.Sequential(torch.nn.Conv2d(channels, hidden, 1), torch.nn.ReLU())
        self.depthwise = torch.nn.Sequential(torch.nn.Conv2d(hidden, hidden, 3, padding=1, groups=hidden), torch.nn.ReLU6())
        self.project = torch.nn.Conv2d(hidden, channels, 1)
        self.add = torch.ao.nn.quantized.FloatFunctional()

    def forward(self, x):
        return self.add.add(self.project(self.depthwise(self.expand(x))), x)


def inverted_residual():
    """(the QAT block in eval mode, the quantizers {"in", "hidden", "dw"} beside it, a float32 sample): per-channel symmetric
    qint8 weights (the README's qconfig); the project layer carries its own output fake-quantizer and the FloatFunctional the
    add's"""
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    torch.manual_seed(31)
    net = InvertedResidual()
    weight = LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                        qscheme=torch.per_channel_symmetric)
    net.qconfig = QConfig(activation=torch.nn.Identity, weight=weight)
    net.train()
    prepare_qat(net, inplace=True)
    x = torch.randn(2, 16, 9, 7)
    net(x)                                                                 # one batch: initialises the weight quantizers
    net.eval()
    with torch.no_grad():
        q_in = R.trained_quantizer(x)
        h = net.expand(q_in(x))
        q_hidden = R.trained_quantizer(h)
        d = net.depthwise(q_hidden(h))
        q_dw = R.trained_quantizer(d)
        out = net.project(q_dw(d))
        q_pre = R.trained_quantizer(out)
        q_add = R.trained_quantizer(q_pre(out) + q_in(x))
    net.project.activation_post_process = q_pre
    net.add.activation_post_process = q_add
    return net, {"in": q_in, "hidden": q_hidden, "dw": q_dw}, x


def convert_inverted_residual(net, qs, mid):
    """the expand layer by convert_w8a8_q, the depthwise layer by convert_w8a8_depthwise, the project layer and the add by
    convert_w8a8_add_q, on disjoint names; the block's forward as it is"""
    from torchlsq.quantized import convert_w8a8_add_q, convert_w8a8_depthwise, convert_w8a8_q
    new = convert_w8a8_q(net, {"expand.0": qs["in"]}, {"expand.0": qs["hidden"]}, relu=("expand.0",), mid_dtype=mid)
    new = convert_w8a8_depthwise(new, {"depthwise.0": qs["hidden"]}, {"depthwise.0": qs["dw"]}, relu6=("depthwise.0",), mid_dtype=mid,
                                 inplace=True)
    return convert_w8a8_add_q(new, {"add": "project"}, {"project": qs["dw"]}, mid_dtype=mid, inplace=True)


def inverted_residual_written_out(net, qs, x, mid):
    """the same block as the modules written out on the levels tensor x: the add's levels"""
    from torchlsq.quantized import AddW8A8Q, Conv2dW8A8AddQ, Conv2dW8A8Q, DepthwiseConv2dW8A8Q
    dev = x.device
    h = Conv2dW8A8Q.from_float(net.expand[0], qs["in"], qs["hidden"], relu=True, mid_dtype=mid).to(dev)(x)
    d = DepthwiseConv2dW8A8Q.from_float(net.depthwise[0], qs["hidden"], qs["dw"], act="relu6", mid_dtype=mid).to(dev)(h)
    project = Conv2dW8A8AddQ.from_float(net.project, qs["dw"], net.add.activation_post_process, mid_dtype=mid).to(dev)
    return AddW8A8Q().add(project(d), x), h, d
