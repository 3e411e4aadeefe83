"""What tests/test_qlinear_w8_cpu.py and tests/test_qlinear_w8_gpu.py share: activation levels, per-channel weight levels, the
int64 / float64 reference and the accuracy bound of the W8A8 linear op (include/lsq_hip_qlinear_w8.h).

    I[m, n] = sum_k (lx[m, k] - zx) * (lw[n, k] - zw[n]),   r = s_x s_w[n] I (+ bias[n])

The bound is derived, not measured: |y - r| <= E + u (|r| + E) with E = 9 * 2^-24 * (s_x s_w |I| + |bias|) and u = 0 / 2^-8 /
2^-11 for fp32 / bf16 / fp16 outputs (+ 2^-24 for fp16, its subnormal spacing): one rounding converts I, one multiplies by
s_w, one by s_x, one adds the bias (a 16-bit bias is exact in fp32) -- four roundings of 2^-24 relative each; 9 leaves room
for their compounding.  Then the output rounding.  qlinear_cases.worst_ratio / assert_exact apply as they are: they take (r, E).
"""
import torch

import qlinear_a8_cases as A
import qlinear_cases as C

DTYPES = C.DTYPES
LEVEL_RANGE = {torch.uint8: (0, 255), torch.int8: (-128, 127)}
S_X_EXACT = 2.0 ** -4

levels = A.levels          # (shape, lo, hi, seed) -> uint8 / int8 levels
act = A.act                # (s_x, zx, device) -> the two one-element tensors
special_x = A.special_x


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def weight(N, K, dtype=torch.int8, seed=0, zeros=None, exact=False):
    """(levels [N, K] of dtype, scale [N] float32, zero point [N] int32): uniform levels over the type's range; zero points
    near the middle of the range with `zeros` (a list) written over the first rows; exact=True: every scale 2^-6"""
    lo, hi = LEVEL_RANGE[dtype]
    g = _gen(seed + 800)
    lw = torch.randint(lo, hi + 1, (N, K), generator=g).to(dtype)
    s = torch.full((N,), 2.0 ** -6) if exact else torch.rand(N, generator=g) * 0.02 + 0.001
    mid = (lo + hi + 1) // 2
    z = torch.randint(mid - 9, mid + 10, (N,), generator=g).clamp(lo, hi).to(torch.int32)
    for i, v in enumerate(zeros or ()):
        if i < N:
            z[i] = v
    return lw, s.to(torch.float32), z


def random_bias(N, dtype, seed=0):
    return (torch.randn(N, generator=_gen(seed + 900)) * 0.5).to(dtype)


def exact_I(lx, zx, lw, zw):
    """[..., N] int64: the exact integer of the contract"""
    a = lx.cpu().to(torch.int64) - int(zx)
    wz = lw.cpu().to(torch.int64) - zw.cpu().to(torch.int64).reshape(-1, 1)
    return a @ wz.t()


def reference(lx, s_x, zx, lw, s_w, zw, bias=None):
    """(r, E) in float64 from the exact int64 I (|I| < 2^53: exact in float64 as well)"""
    I = exact_I(lx, zx, lw, zw).double()
    sw = s_w.cpu().double().reshape(-1)
    r = float(s_x) * sw * I
    S = float(s_x) * sw * I.abs()
    if bias is not None:
        r = r + bias.detach().cpu().double()
        S = S + bias.detach().cpu().double().abs()
    return r, 9 * 2.0 ** -24 * S


def plan_row_thresholds(plan, N, K, upto=160):
    """every M in 2..upto at which `plan(M, N, K)` differs from `plan(M - 1, N, K)` in anything but the grid's size"""
    def key(M):
        pl = plan(M, N, K)
        return tuple(v for k, v in sorted(pl.items()) if k not in ("grid", "lds_bytes"))
    return [M for M in range(2, upto + 1) if key(M) != key(M - 1)]


def qat_model():
    """Linear(64, 32) -> ReLU -> Linear(32, 8) with the README's qconfig for the weights (per-channel symmetric qint8),
    trained for three steps; per-tensor quint8 activation quantizers for the model's input and for layer 2's input"""
    import torch.nn as nn
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver, MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    torch.manual_seed(3)
    model = nn.Sequential(nn.Linear(64, 32), nn.ReLU(), nn.Linear(32, 8, bias=False))
    weight = LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                        qscheme=torch.per_channel_symmetric)
    act = LSQFakeQuantizer.with_args(observer=MovingAverageMinMaxObserver, otype="activation")
    model.qconfig = QConfig(activation=nn.Identity, weight=weight)
    model.train()
    prepare_qat(model, inplace=True)
    in_q, mid_q = act(), act()
    params = list(model.parameters())
    opt = torch.optim.SGD(params, lr=1e-2)
    for _ in range(3):
        x = torch.randn(4, 64)
        loss = model[2](mid_q(model[1](model[0](in_q(x))))).square().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    for q in (in_q, mid_q):
        q.disable_observer()
    return model.eval(), in_q.eval(), mid_q.eval()
