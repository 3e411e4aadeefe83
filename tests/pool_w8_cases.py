"""What tests/test_pool_w8_cpu.py and tests/test_pool_w8_gpu.py share: pooling on 8-bit levels (include/lsq_hip_pool_w8.h).  The
CPU path of the ops is the definition; the GPU must equal it bit for bit, and the CPU tests hold it to an independent numpy
restatement (int64 window sums, np.float32 steps) and to torch's float64 pooling of the dequantized values.

Inputs stand on the existing helpers: levels clip(rint(z + 32 N(0, 1))) of either level type (resadd_w8_cases.residual, z the
middle of the type's range, scale 1 / 32), output quantizers by requant_w8_cases.out_quantizer from the float32 averages (MAD-based
scale sd / 64, mid-range zero point).  `assert_conditions` holds every random average-pool case of at least 336 outputs to:
requant_w8_cases.assert_not_vacuous as it stands, and at least 40 % of the levels change when every window is shifted by one
pixel along W (computed on the CPU path: 0.965 .. 0.992 over the 151 cases that the two test files hold to it, listed in
DESIGN.md 9.11).
"""
import numpy as np
import torch

import requant_w8_cases as R
import resadd_w8_cases as A

OPS = torch.ops.torchlsq
CL = torch.channels_last
LEVEL_DTYPES = (torch.uint8, torch.int8)
MIDS = R.MIDS

# max pool: (H, W, kernel, stride, padding, dilation, ceil_mode)
MAX_GEOMS = [
    (9, 7, (3, 3), (2, 2), (1, 1), (1, 1), False),
    (9, 7, (2, 2), (2, 2), (0, 0), (1, 1), False),
    (9, 7, (3, 3), (1, 1), (1, 1), (1, 1), False),
    (9, 7, (3, 2), (2, 1), (1, 0), (1, 2), False),
    (8, 8, (3, 3), (2, 2), (0, 0), (1, 1), True),           # the last window overhangs the input
]
# average pool, a window per lane: (H, W, kernel, stride, padding, ceil_mode, count_include_pad, divisor_override)
AVG_LANE_CASES = [
    (12, 10, (2, 2), (2, 2), (0, 0), False, True, None),
    (12, 10, (3, 3), (2, 2), (1, 1), False, True, None),
    (12, 10, (3, 3), (2, 2), (1, 1), False, False, None),
    (12, 10, (3, 3), (2, 2), (1, 1), False, True, 7),
    (12, 11, (3, 3), (2, 2), (1, 1), True, True, None),
    (12, 11, (3, 3), (2, 2), (1, 1), True, False, None),
]
# (unsigned output levels or None for floats out, mid_dtype)
AVG_VARIANTS = [(u, mid) for u in (True, False, None) for mid in MIDS]


def geom_id(g):
    return "_".join(str(v).replace(" ", "") for v in g)


def avg_id(v):
    return "%s_%s" % ({True: "u8", False: "i8", None: "float"}[v[0]], str(v[1]).replace("torch.", ""))


def x_levels(B, C, H, W, dtype, seed=0):
    """(levels [B, C, H, W] in channels-last memory, s_x [1] float32, zx [1] int32)"""
    lv, s, z = A.residual((B, H, W, C), 1.0, dtype, seed)
    return lv.permute(0, 3, 1, 2), s, z


def negative_corner(lx):
    """int8 levels whose top-left 2 x 3 pixels are all negative: a padded tap taken for the byte 0 would win the first window"""
    lx = lx.clone(memory_format=torch.preserve_format)
    lx[:, :, :2, :3] = -lx[:, :, :2, :3].to(torch.int32).abs().clamp(1, 127).to(torch.int8)
    return lx


def out_hw(H, W, kernel, stride, padding, dilation, ceil_mode):
    def extent(n, k, s, p, d):
        num = n + 2 * p - d * (k - 1) - 1
        out = (-(-num // s) if ceil_mode else num // s) + 1
        return out - 1 if ceil_mode and (out - 1) * s >= n + p else out
    return extent(H, kernel[0], stride[0], padding[0], dilation[0]), extent(W, kernel[1], stride[1], padding[1], dilation[1])


def avg_args(case):
    """the op's geometry arguments of an AVG_LANE_CASES row"""
    H, W, k, s, p, ceil_mode, cip, div = case
    return (list(k), list(s), list(p), ceil_mode, cip, div)


def avg_float(lx, s_x, zx, args, dtype=torch.float32):
    return OPS.lsq_avg_pool2d_q8(lx, s_x, zx, *args, dtype)


def avg_q(lx, s_x, zx, args, osc, osh, rng, mid):
    return OPS.lsq_avg_pool2d_q8_q(lx, s_x, zx, *args, osc, osh, *rng, mid)


def avg_case(B, C, case, x_dtype, unsigned, seed):
    """the CPU operands of one random case: (lx, s_x, zx, args, osc, osh, rng); the output quantizer from the float32 averages"""
    lx, s_x, zx = x_levels(B, C, case[0], case[1], x_dtype, seed)
    args = avg_args(case)
    osc, osh, rng = R.out_quantizer(avg_float(lx, s_x, zx, args), unsigned, False)
    return lx, s_x, zx, args, osc, osh, rng


def assert_conditions(got, c, mid, note=""):
    """the two conditions of the module's docstring, on the CPU levels `got` of the CPU case `c`"""
    lx, s_x, zx, args, osc, osh, rng = c
    R.assert_not_vacuous(got, rng, note)
    a = avg_q(lx[..., 1:].contiguous(memory_format=CL), s_x, zx, args, osc, osh, rng, mid)
    b = avg_q(lx[..., :-1].contiguous(memory_format=CL), s_x, zx, args, osc, osh, rng, mid)
    changed = A.differ(a, b)
    assert changed >= 0.40, (note, "only %.1f %% of the levels change when the windows are shifted by one pixel" % (100 * changed))
    return changed


def numpy_avg(lx, s_x, zx, kernel, stride, padding, ceil_mode, count_include_pad, divisor_override):
    """v of the contract as np.float32 [B, C, OH, OW], window by window: an int64 sum, then np.float32 steps"""
    l = lx.cpu().numpy().astype(np.int64) - int(zx)
    B, C, H, W = l.shape
    (kh, kw), (sh, sw), (ph, pw) = kernel, stride, padding
    OH, OW = out_hw(H, W, kernel, stride, padding, (1, 1), ceil_mode)
    v = np.zeros((B, C, OH, OW), dtype=np.float32)
    s = np.float32(float(s_x))
    for oh in range(OH):
        for ow in range(OW):
            h0, w0 = oh * sh - ph, ow * sw - pw
            hs, he, ws, we = max(h0, 0), min(h0 + kh, H), max(w0, 0), min(w0 + kw, W)
            if divisor_override is not None:
                D = divisor_override
            elif count_include_pad:
                D = (min(h0 + kh, H + ph) - h0) * (min(w0 + kw, W + pw) - w0)
            else:
                D = (he - hs) * (we - ws)
            S = l[:, :, hs:he, ws:we].sum(axis=(2, 3))
            v[:, :, oh, ow] = (S.astype(np.float32) * s) / np.float32(D)
    return v


def numpy_levels(u, osc, osh, rng):
    """lsq_math.hpp's level() in np.float32 steps on float32 values u: int64 levels"""
    qmin, qmax, tmin, tmax = (np.float32(v) for v in rng)
    s = np.maximum(np.abs(np.float32(float(osc))), np.float32(np.finfo(np.float32).eps))
    inv = np.float32(1.0) / s
    zp = np.rint(np.minimum(tmax, np.maximum(tmin, -np.float32(float(osh)) * inv)))
    t = u.astype(np.float32) * inv + zp
    q = np.rint(np.minimum(qmax, np.maximum(qmin, t)))
    return np.where(np.isnan(t), qmin, q).astype(np.int64)


def exact_mean(lx, s_x, zx, args):
    """F.avg_pool2d of the float64 dequantized values (the products formed in float64): torch's own divisor semantics"""
    k, s, p, ceil_mode, cip, div = args
    d = (lx.cpu().to(torch.float64) - float(zx)) * float(s_x)
    return torch.nn.functional.avg_pool2d(d, k, s, p, ceil_mode, cip, div)


def expected_avg_plan(B, C, OH, OW, taps, aligned=True, cus=256):
    """(family, lanes per window, grid) by the rule of include/lsq_hip_pool_w8.h"""
    if not aligned or C % 16:
        return "generic", 1, -(-B * OH * OW * C // 256)
    items = B * OH * OW * (C // 16)
    lanes = 1
    if taps >= 10:
        cap = 1
        while cap < 256 and cap * 2 <= taps:
            cap *= 2
        while lanes < cap and -(-items // (256 // lanes)) < 2 * cus:
            lanes *= 2
    return ("packets" if lanes == 1 else "packets_shared"), lanes, -(-items // (256 // lanes))


class SmallNet(torch.nn.Module):
    """conv 16 -> 16 3 x 3 + ReLU -> max pool 3/2/1 -> resadd_w8_cases.BasicBlock -> adaptive average pool -> flatten -> linear"""

    def __init__(self, block):
        super().__init__()
        self.stem = torch.nn.Conv2d(16, 16, 3, padding=1)
        self.relu = torch.nn.ReLU()
        self.maxpool = torch.nn.MaxPool2d(3, 2, 1)
        self.block = block
        self.avgpool = torch.nn.AdaptiveAvgPool2d(1)
        self.flatten = torch.nn.Flatten()
        self.fc = torch.nn.Linear(32, 10)

    def forward(self, x):
        return self.fc(self.flatten(self.avgpool(self.block(self.maxpool(self.relu(self.stem(x)))))))


def small_net():
    """(the QAT network in eval mode, its quantizers, a float32 sample): per-channel symmetric qint8 weights (the README's qconfig),
    the block's conv2 and FloatFunctional with their own output fake-quantizers as in resadd_w8_cases.basic_block; the per-tensor
    quint8 activation quantizers {"x", "in" (the stem's output: the max pool hands its levels on to the block), "mid", "identity",
    "gap" (the average pool's output), "out" (the classifier's)} are kept beside the model"""
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    torch.manual_seed(21)
    net = SmallNet(A.BasicBlock())
    weight = LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                        qscheme=torch.per_channel_symmetric)
    net.qconfig = QConfig(activation=torch.nn.Identity, weight=weight)
    net.train()
    prepare_qat(net, inplace=True)
    x = torch.randn(4, 16, 19, 19)
    net(x)                                                                 # one batch: initialises the weight quantizers
    net.eval()
    b = net.block
    with torch.no_grad():
        q_x = R.trained_quantizer(x)
        s = net.relu(net.stem(q_x(x)))
        q_in = R.trained_quantizer(s)
        p = net.maxpool(q_in(s))
        q_id = R.trained_quantizer(b.downsample(p))
        q_mid = R.trained_quantizer(b.relu(b.conv1(p)))
        out = b.conv2(q_mid(b.relu(b.conv1(p))))
        q_pre = R.trained_quantizer(out)
        t = torch.relu(q_pre(out) + q_id(b.downsample(p)))
        q_add = R.trained_quantizer(t)
        g = net.avgpool(q_add(t))
        q_gap = R.trained_quantizer(g)
        q_out = R.trained_quantizer(net.fc(net.flatten(q_gap(g))))
    b.conv2.activation_post_process = q_pre
    b.add_relu.activation_post_process = q_add
    return net, {"x": q_x, "in": q_in, "mid": q_mid, "identity": q_id, "gap": q_gap, "out": q_out}, x


def convert_small_net(net, qs, mid):
    """the stem (+ ReLU) and the classifier by convert_w8a8_q, the block by resadd_w8_cases.convert_block, the two pools by
    convert_w8a8_pool; the network's forward as it is"""
    from torchlsq.quantized import convert_w8a8_pool, convert_w8a8_q
    new = convert_w8a8_q(net, {"stem": qs["x"], "fc": qs["gap"]}, {"stem": qs["in"], "fc": qs["out"]}, relu=("stem",), mid_dtype=mid)
    new.relu = torch.nn.Identity()                                         # the stem's ReLU moved into its kernel
    new.block = A.convert_block(new.block, qs, mid)
    return convert_w8a8_pool(new, {"maxpool": None, "avgpool": qs["gap"]}, mid_dtype=mid, inplace=True)


def small_net_written_out(net, qs, x, mid):
    """the same network as the existing modules and the new ops written out, on the levels tensor x: the classifier's levels"""
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import Conv2dW8A8Q, LinearW8A8Q
    from torchlsq.quantized.modules.packed_linear_a8 import _per_tensor_constants
    dev = x.device
    h = Conv2dW8A8Q.from_float(net.stem, qs["x"], qs["in"], relu=True, mid_dtype=mid).to(dev)(x)
    p = LevelsTensor(OPS.lsq_max_pool2d_q8(h.levels, [3, 3], [2, 2], [1, 1], [1, 1], False), h.scale, h.zero_point, h.quant_min, h.quant_max, h.type_min, h.type_max)
    bl = A.block_written_out(net.block, qs, p, mid)
    asc, ash, *arng = _per_tensor_constants(net.block.add_relu.activation_post_process, "add")
    from torchlsq._qlinear_a8_host import _act_constants
    s_b, z_b = _act_constants(asc.to(dev), ash.to(dev), arng[2], arng[3])
    gsc, gsh, *grng = _per_tensor_constants(qs["gap"], "gap")
    g = OPS.lsq_avg_pool2d_q8_q(bl, s_b, z_b, [bl.shape[2], bl.shape[3]], [bl.shape[2], bl.shape[3]], [0, 0], False, True, None,
                                gsc.to(dev), gsh.to(dev), *grng, mid)
    s_g, z_g = _act_constants(gsc.to(dev), gsh.to(dev), grng[2], grng[3])
    fc = LinearW8A8Q.from_float(net.fc, qs["gap"], qs["out"], mid_dtype=mid).to(dev)
    return fc(LevelsTensor(g.flatten(1), s_g, z_g, *grng)).levels
