"""What tests/test_qlinear_cpu.py and tests/test_qlinear_gpu.py share: packed weights on the CPU, the fp64 reference, the
accuracy bound and the exact-arithmetic inputs of the linear op on packed weights (include/lsq_hip_qlinear.h).

The bound is derived, not measured.  With r = x @ w^T (+ bias) in fp64, S = |x| @ |w|^T (+ |bias|), E = (K + 8) 2^-24 S and
u = 0 / 2^-8 / 2^-11 for fp32 / bf16 / fp16 outputs:  |y - r| <= E + u (|r| + E)  (+ 2^-24 for fp16, its subnormal spacing).
Any order of K fp32 additions of once-rounded products errs by at most gamma_K * sum|terms|; factoring the group's scale
and adding the bias are a handful of further roundings (the + 8); the output rounding is at most u |y|.
"""
import torch

from torchlsq.functional import PackedGroupTensor, lsq_pack_per_group

U = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# (M, N, K, G, bits): the smallest shapes at which the forms differ -- a ragged tile of 17 columns on one 16-byte packet row
# of three; 67 columns and groups of 4 packets; 2-bit codes over one full chunk of x; two generic formats (G below a packet);
# 16 rows on a full chunk with one packet per group
SHAPES = [(1, 17, 96, 32, 4), (16, 67, 384, 128, 4), (3, 5, 4096, 128, 2), (5, 9, 24, 8, 4), (2, 3, 8, 2, 4), (16, 64, 4096, 32, 4)]
# beyond one chunk of x (two chunks, the second partial) with groups of 3 packets (no power of two)
SHAPES_EXTRA = [(4, 33, 4800, 96, 4)]


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def random_packed(N, K, G, bits, seed=0):
    """a symmetric export (-8..7 / -2..1, shift +0.0) of a random weight"""
    g = _gen(seed)
    qmin, qmax = (-8, 7) if bits == 4 else (-2, 1)
    s = torch.rand(N, K // G, generator=g) * 0.05 + 0.01
    w = torch.randn(N, K, generator=g) * s.repeat_interleave(G, dim=1) * (qmax * 0.6)
    return lsq_pack_per_group(w, s, torch.zeros(N, K // G), G, bits, qmin, qmax, -128, 127)


def affine_packed(N, K, G, seed=0):
    """an affine 4-bit export in a -128..127 type whose shifts put the zero point, and with it qzero, near 100"""
    g = _gen(seed)
    s = torch.rand(N, K // G, generator=g) * 0.05 + 0.01
    zp = torch.randint(95, 106, (N, K // G), generator=g).to(torch.float32)
    w = (torch.rand(N, K, generator=g) * 15 - zp.repeat_interleave(G, dim=1)) * s.repeat_interleave(G, dim=1)
    p = lsq_pack_per_group(w, s, -zp * s, G, 4, 0, 15, -128, 127)
    assert int(p.zero_point.min()) >= 90 and int(p.zero_point.max()) <= 110 and len(p.codes.unique()) > 8
    return p


def far_packed(N, K, G, bits, seed=0):
    """zero points far outside the code range, both signs, next to ordinary ones (the format allows +-2^23)"""
    g = _gen(seed)
    codes = torch.randint(0, 256, (N, K * bits // 8), generator=g).to(torch.uint8)
    s = torch.rand(N, K // G, generator=g) * 1e-6 + 1e-7           # |w| up to 8: sums stay inside fp16
    zp = torch.randint(0, 2 ** bits, (N, K // G), generator=g).to(torch.int32)
    zp.view(-1)[::3] = 70000
    zp.view(-1)[1::7] = -5000
    zp.view(-1)[2::11] = 300
    zp.view(-1)[4::13] = (1 << 23)
    return PackedGroupTensor(codes, s, zp, bits, G, 0, (N, K))


def exact_packed(N, K, G, bits, seed=0):
    """codes and zero points random in [0, 2^bits), every scale 2^-6"""
    g = _gen(seed)
    codes = torch.randint(0, 256, (N, K * bits // 8), generator=g).to(torch.uint8)
    zp = torch.randint(0, 2 ** bits, (N, K // G), generator=g).to(torch.int32)
    return PackedGroupTensor(codes, torch.full((N, K // G), 2.0 ** -6), zp, bits, G, 0, (N, K))


def exact_x(shape, dtype, seed=0):
    """integers in [-8, 8]: with exact_packed and K <= 4096 every product and partial sum is exact in fp32"""
    return torch.randint(-8, 9, shape, generator=_gen(seed + 100)).to(dtype)


def random_x(shape, dtype, seed=0):
    return torch.randn(shape, generator=_gen(seed + 200)).to(dtype)


def random_bias(N, dtype, seed=0):
    return torch.randn(N, generator=_gen(seed + 300)).to(dtype)


def reference(x, p, bias=None):
    """(r, E): the fp64 result and the fp32-accumulation part of the bound, both [..., N] on the CPU"""
    w = p.dequantize(torch.float32).reshape(p.shape[0], -1).double()
    xd = x.detach().cpu().double()
    r = xd @ w.t()
    S = xd.abs() @ w.abs().t()
    if bias is not None:
        r = r + bias.detach().cpu().double()
        S = S + bias.detach().cpu().double().abs()
    return r, (w.shape[1] + 8) * 2.0 ** -24 * S


def worst_ratio(y, r, E, dtype):
    """max of |y - r| / bound (0 where both are 0): within the bound iff <= 1"""
    bound = E + U[dtype] * (r.abs() + E) + (2.0 ** -24 if dtype == torch.float16 else 0.0)
    err = (y.detach().cpu().double() - r).abs()
    assert y.dtype == dtype and tuple(y.shape) == tuple(r.shape)
    assert bool(torch.isfinite(y.detach().float()).all())
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(ratio.max())


def assert_within_bound(y, r, E, dtype, what=""):
    ratio = worst_ratio(y, r, E, dtype)
    print("%s: worst error / bound = %.3f" % (what, ratio))
    assert ratio <= 1.0, "%s: error is %.3f times the bound" % (what, ratio)


def assert_exact(y, r, dtype, what=""):
    """y is r rounded once (r is exact in fp32 here, so fp64 -> fp32 is exact and fp32 -> dtype is the one rounding)"""
    want = r.float().to(dtype)
    assert y.dtype == dtype and torch.equal(y.detach().cpu().view(INT[dtype]), want.view(INT[dtype])), \
        "%s: not the exact result rounded once (%d of %d values differ)" % (
            what, int((y.detach().cpu().view(INT[dtype]) != want.view(INT[dtype])).sum()), want.numel())
