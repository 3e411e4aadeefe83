"""What tests/test_qlinear_a8_cpu.py and tests/test_qlinear_a8_gpu.py share: activation levels, packed weights, the int64 /
float64 reference and the accuracy bound of the 8-bit-activation linear op (include/lsq_hip_qlinear_a8.h).

    I[m, n, g] = sum_{k in g} (lx[m, k] - zx) * (code[n, k] - qzero[n, g]),   r = s_x sum_g qscale I (+ bias),
    S = s_x sum_g qscale |I| (+ |bias|)

The bound is derived, not measured: |y - r| <= E + u (|r| + E) with E = (K / G + 8) 2^-24 S and u = 0 / 2^-8 / 2^-11 for
fp32 / bf16 / fp16 outputs (+ 2^-24 for fp16, its subnormal spacing).  One rounding converts I, one multiplies by qscale,
K / G - 1 additions follow, then s_x, then the bias, then the output rounding; the + 8 covers the handful beyond K / G.
qlinear_cases.worst_ratio / assert_exact apply as they are: they take (r, E).
"""
import torch

import qlinear_cases as C
from torchlsq.functional import PackedGroupTensor

DTYPES = C.DTYPES
# qlinear_cases' shapes -- (1, 17, 96, 32, 4) is also a ragged 64-k MFMA step, one and a half -- and one full 2-bit MFMA step
# under 16 rows
SHAPES = C.SHAPES + C.SHAPES_EXTRA + [(16, 16, 64, 64, 2)]
S_X_EXACT = 2.0 ** -4


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def levels(shape, lo, hi, seed=0):
    """uniform integer levels in lo..hi as the bytes the ops take: uint8 for a range in 0..255, int8 for -128..127"""
    v = torch.randint(lo, hi + 1, shape, generator=_gen(seed + 400))
    return v.to(torch.uint8) if hi > 127 else v.to(torch.int8)


def act(s_x, zx, device="cpu"):
    return torch.tensor([s_x], dtype=torch.float32, device=device), torch.tensor([zx], dtype=torch.int32, device=device)


def unpack(p):
    """codes [N, K] as int64"""
    per = 8 // p.bits
    c = p.codes.cpu().to(torch.int64)
    parts = [(c >> (j * p.bits)) & (2 ** p.bits - 1) for j in range(per)]
    return torch.stack(parts, dim=-1).reshape(p.shape[0], -1)


def reference(lx, s_x, zx, p, bias=None):
    """(r, E) in float64 from exact int64 group sums; lx [..., K] integer levels (any integer dtype), s_x / zx numbers"""
    N, K = p.shape[0], lx.shape[-1]
    G = p.group_size
    a = lx.cpu().to(torch.int64).reshape(-1, K // G, G) - int(zx)
    cz = unpack(p).reshape(N, K // G, G) - p.zero_point.cpu().to(torch.int64).reshape(N, K // G, 1)
    I = torch.einsum("mgk,ngk->mng", a.double(), cz.double())          # |I| < 2^53: exact in float64
    qs = p.scale.cpu().double().reshape(N, K // G)
    r = float(s_x) * (I * qs).sum(-1)
    S = float(s_x) * (I.abs() * qs).sum(-1)
    if bias is not None:
        r = r + bias.detach().cpu().double()
        S = S + bias.detach().cpu().double().abs()
    shape = tuple(lx.shape[:-1]) + (N,)
    return r.reshape(shape), ((K // G + 8) * 2.0 ** -24 * S).reshape(shape)


def wide_packed(N, K, G, bits, seed=0):
    """qlinear_cases.far_packed: zero points of 70000, -5000, 300 and 2^23 next to ordinary ones"""
    return C.far_packed(N, K, G, bits, seed)


def wide_exact_packed(N, K, G, bits, seed=0):
    """zero points of 2^23, 2^16 and -2^12 next to ordinary ones, every scale a power of two.  An ordinary group has scale
    2^-6.  A far group has all codes 0 and scale 2^-6 / |qzero|: its I = -qzero * sum(lx - zx) is a 13-bit integer times a power
    of two, and its term is that sum / 64 -- every product and partial sum is exact in fp32, while qzero * sum(lx - zx)
    overflows 32 bits."""
    p = C.exact_packed(N, K, G, bits, seed)
    zp, s = p.zero_point.clone(), p.scale.clone()
    codes = p.codes.clone().reshape(N, K // G, G * bits // 8)
    for start, step, val in ((0, 3, 1 << 23), (1, 7, 1 << 16), (2, 11, -(1 << 12))):
        zp.view(-1)[start::step] = val
    far = zp.abs() > 2 ** bits
    s[far] = 2.0 ** -6 / zp[far].abs().float()
    codes[far] = 0
    return PackedGroupTensor(codes.reshape(N, -1), s, zp, bits, G, 0, (N, K))


def special_x(M, K, dtype, scale, shift, qmin, qmax, seed=0):
    """random x over a bit more than the quantizer's range, with NaN, +-inf, -0.0, both borders and a tie in the first row"""
    x = torch.randn(M, K, generator=_gen(seed + 500)) * (qmax - qmin) * scale * 0.4 + ((qmax + qmin) * 0.5 * scale + shift)
    zp = -shift / scale
    x[0, :8] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, (qmin - zp) * scale, (qmax - zp) * scale,
                             (qmin + 2.5 - zp) * scale, 0.0])
    return x.to(dtype)
