"""What tests/test_qconv_w8_cpu.py and tests/test_qconv_w8_gpu.py share: geometries, conv weights as levels, the int64 / float64
reference and the accuracy bound of the W8A8 conv2d op (include/lsq_hip_qconv_w8.h).

    I[b, n, oh, ow] = sum_{i, j, c} (lx[b, c, oh sh - ph + i dh, ow sw - pw + j dw] - zx) * (lw[n, c, i, j] - zw[n])
    r = s_x s_w[n] I (+ bias[n])

The bound is qlinear_w8_cases.reference's, as it is: the same four roundings (float(I), times s_w, times s_x, plus bias) and
then the output rounding; the number of terms of I does not enter, because I is exact.
"""
import torch
import torch.nn.functional as F

import qlinear_w8_cases as W

# (B, Cin, H, W, Cout, kernel, stride, padding, dilation): the smallest shapes at which each mechanism of the matrix-core form
# can go wrong
GEOMETRIES = [
    (2, 16, 5, 7, 17, (3, 3), (1, 1), (1, 1), (1, 1)),      # K = 144: a tail step; padding on every side; M = 70
    (1, 32, 6, 6, 5, (3, 3), (2, 2), (1, 1), (1, 1)),       # K = 288: two steps; M = 9 < 16
    (3, 16, 4, 9, 67, (1, 1), (2, 1), (0, 0), (1, 1)),
    (1, 48, 7, 5, 20, (1, 3), (1, 1), (0, 2), (1, 2)),      # tap borders inside a 64-byte MFMA step and inside a 256-byte step
    (2, 16, 3, 3, 16, (3, 3), (1, 1), (2, 2), (1, 1)),      # outputs that see padding only
    (1, 16, 9, 9, 16, (5, 5), (1, 1), (4, 4), (2, 2)),
]
# the linear test's four variants: (x level type, zx, w level type, zero points written over the first channels, y type, bias kind)
VARIANTS = [(torch.uint8, 3, torch.int8, (-7, 127), torch.float32, "f32"),
            (torch.uint8, 125, torch.uint8, (0, 255, 131), torch.bfloat16, "y"),
            (torch.int8, -128, torch.int8, (-128, 5), torch.float16, None),
            (torch.int8, 127, torch.uint8, (7, 200), torch.float32, None),
            (torch.uint8, 255, torch.int8, (-128, 127), torch.float32, None)]


def geom_id(g):
    return "B%d_C%d_%dx%d_N%d_k%dx%d_s%d%d_p%d%d_d%d%d" % (g[0], g[1], g[2], g[3], g[4], *g[5], *g[6], *g[7], *g[8])


def out_hw(H, Wd, kernel, stride, padding, dilation):
    return tuple((n + 2 * p - d * (k - 1) - 1) // s + 1 for n, k, s, p, d in zip((H, Wd), kernel, stride, padding, dilation))


def conv_weight(Cout, Cin, kernel, dtype=torch.int8, seed=0, zeros=None, exact=False):
    """(levels [Cout, Cin, kh, kw] of dtype in channels-last memory, scale [Cout] float32, zero point [Cout] int32)"""
    kh, kw = kernel
    lw, s, z = W.weight(Cout, kh * kw * Cin, dtype, seed, zeros, exact)
    return lw.reshape(Cout, kh, kw, Cin).permute(0, 3, 1, 2), s, z         # the [N, K] matrix IS the channels-last weight


def x_levels(B, Cin, H, Wd, dtype, seed=0):
    """[B, Cin, H, W] levels over the type's range, channels-last memory"""
    lo, hi = W.LEVEL_RANGE[dtype]
    return W.levels((B, H, Wd, Cin), lo, hi, seed).permute(0, 3, 1, 2)


def exact_I(lx, zx, lw, zw, stride, padding, dilation):
    """[B, Cout, OH, OW] int64: the exact integer of the contract, one int64 convolution of the differences"""
    a = lx.cpu().to(torch.int64) - int(zx)
    wz = lw.cpu().to(torch.int64) - zw.cpu().to(torch.int64).reshape(-1, 1, 1, 1)
    return F.conv2d(a, wz, None, stride, padding, dilation)


def unfold_I(lx, zx, lw, zw, stride, padding, dilation):
    """the same integers by another road: F.unfold of lx - zx (float64, exact for 9-bit integers; its zero padding is the
    padding with zx) and qlinear_w8_cases.exact_I on the [B L, Cin kh kw] matrix"""
    B, Cout = lx.shape[0], lw.shape[0]
    a = (lx.cpu().to(torch.int64) - int(zx)).double()
    cols = F.unfold(a, lw.shape[2:], dilation, padding, stride)            # [B, Cin kh kw, L], k = (c, i, j)
    mat = cols.transpose(1, 2).reshape(-1, cols.shape[1]).to(torch.int64)
    I = W.exact_I(mat, 0, lw.cpu().reshape(Cout, -1), zw)                  # [B L, Cout]
    oh, ow = out_hw(lx.shape[2], lx.shape[3], lw.shape[2:], stride, padding, dilation)
    return I.reshape(B, oh, ow, Cout).permute(0, 3, 1, 2)


def reference(lx, s_x, zx, lw, s_w, zw, bias, stride, padding, dilation):
    """(r, E) in float64, [B, Cout, OH, OW]: float64 F.conv2d on the dequantized tensors with the scales taken out of the sum --
    lx - zx and lw - zw are integers below 2^9 and their sums stay below 2^53, so the float64 convolution is exact, and
    r = s_x s_w I carries two float64 roundings.  (With the scales inside, each term of the float64 sum would carry a rounding
    of its own, measured against sum |terms| and not against |I|: an error of the reference, not of the op.)  E as in
    qlinear_w8_cases.reference."""
    a = (lx.cpu().to(torch.int64) - int(zx)).double()
    wz = (lw.cpu().to(torch.int64) - zw.cpu().to(torch.int64).reshape(-1, 1, 1, 1)).double()
    I = F.conv2d(a, wz, None, stride, padding, dilation)
    sw = s_w.cpu().double().reshape(1, -1, 1, 1)
    r = float(s_x) * sw * I
    S = float(s_x) * sw * I.abs()
    if bias is not None:
        b = bias.detach().cpu().double().reshape(1, -1, 1, 1)
        r, S = r + b, S + b.abs()
    return r, 9 * 2.0 ** -24 * S


def image_of(M):
    """(B, H, W) with B H W == M, for a 1 x 1 or a padded stride-1 convolution that keeps the image's size"""
    h = max(d for d in range(1, int(M ** 0.5) + 1) if M % d == 0)
    if h % 2 == 0 and h > 2:
        return 2, h // 2, M // h
    return 1, h, M // h


def plan_row_counts(plan_of_M, upto=160):
    """1, 15, 16, 17 and both sides of every M (a number of output pixels) up to `upto` at which the plan changes"""
    ms = {1, 15, 16, 17}
    def launch(M, N, K):       # the plan without the sizes of the implicit GEMM, which change with every M
        return {k: v for k, v in plan_of_M(M).items() if k not in ("M", "N", "K")}
    for t in W.plan_row_thresholds(launch, 0, 0, upto):
        ms |= {t - 1, t}
    return sorted(ms)


def qat_conv_model(with_linear=False):
    """Conv2d(16, 8, 3, padding=1) -> ReLU -> Conv2d(8, 4, 3, stride=2, bias=False) (-> Flatten -> Linear(36, 5)) with the
    README's qconfig for the weights (per-channel symmetric qint8), trained for three steps on 7 x 7 images; per-tensor quint8
    activation quantizers for the model's input, conv 2's input and the linear layer's input"""
    import torch.nn as nn
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver, MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    torch.manual_seed(4)
    layers = [nn.Conv2d(16, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 4, 3, stride=2, bias=False)]
    if with_linear:
        layers += [nn.Flatten(), nn.Linear(36, 5)]
    model = nn.Sequential(*layers)
    weight = LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                        qscheme=torch.per_channel_symmetric)
    act = LSQFakeQuantizer.with_args(observer=MovingAverageMinMaxObserver, otype="activation")
    model.qconfig = QConfig(activation=nn.Identity, weight=weight)
    model.train()
    prepare_qat(model, inplace=True)
    qs = [act() for _ in range(3 if with_linear else 2)]
    opt = torch.optim.SGD(list(model.parameters()), lr=1e-2)
    for _ in range(3):
        h = model[2](qs[1](model[1](model[0](qs[0](torch.randn(4, 16, 7, 7))))))
        if with_linear:
            h = model[4](qs[2](model[3](h)))
        loss = h.square().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    for q in qs:
        q.disable_observer()
    return (model.eval(),) + tuple(q.eval() for q in qs)
