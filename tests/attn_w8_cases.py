"""What tests/test_attn_w8_cpu.py and tests/test_attn_w8_gpu.py share: inputs of the batched matmul and the softmax on 8-bit levels
(random full-range levels, padded rows whose padding holds 0xFF, views of one qkv buffer), output quantizers fitted to the values
an op actually produces, the ops run on a device of choice, and the attention core's quantizers.  Everything is seeded; the CPU
results are computed once per case and shared.
"""
import functools

import numpy as np
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
MIDS = (F32, BF16, F16)
U8, I8 = torch.uint8, torch.int8
PAD = 0xFF


def one(v, dtype=F32):
    return torch.tensor([v], dtype=dtype)


def bits(t):
    """a floating tensor as integers of its width: NaNs and the sign of zero compare too"""
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()]) if t.is_floating_point() else t


def gen(seed):
    return torch.Generator().manual_seed(1000 + seed)


def levels(shape, seed, dtype):
    raw = torch.randint(0, 256, tuple(shape), generator=gen(seed)).to(U8)
    return raw if dtype == U8 else raw.view(I8)


def padded(t, ld, fill=PAD):
    """the [.., cols] view with unit innermost stride of a buffer whose rows are `ld` apart, the padding filled with `fill`"""
    buf = torch.full(tuple(t.shape[:-1]) + (ld,), fill, dtype=U8).view(t.dtype)
    buf[..., :t.shape[-1]] = t
    return buf[..., :t.shape[-1]]


def zero_for(dtype, z_u8):
    """a zero point given on the 0..255 scale, for either level dtype"""
    return one(z_u8 if dtype == U8 else z_u8 - 128, torch.int32)


S_A, S_B = 0.043, 0.017


def bmm_operands(B, M, N, K, nt, seed=0, a_dtype=U8, b_dtype=I8, a_ld=None, b_ld=None, za=117, zb=131):
    """(a, s_a, z_a, b, s_b, z_b, nt) on the CPU; `a_ld` / `b_ld`: row strides beyond the rows, the padding holding 0xFF"""
    lead = (B,) if isinstance(B, int) else tuple(B)
    a = levels(lead + (M, K), 2 * seed, a_dtype)
    b = levels(lead + ((N, K) if nt else (K, N)), 2 * seed + 1, b_dtype)
    if a_ld:
        a = padded(a, a_ld)
    if b_ld:
        b = padded(b, b_ld)
    return (a, one(S_A), zero_for(a_dtype, za), b, one(S_B), zero_for(b_dtype, zb), bool(nt))


def fit_quantizer(values, unsigned):
    """an output quantizer (scale, shift, quant_min, quant_max, type_min, type_max) whose range the float32 `values` just overflow on
    both sides, so that both borders and the levels between them occur"""
    v = values.to(torch.float64)
    lo, hi = min(float(v.min()), 0.0), max(float(v.max()), 0.0)       # a zero point lies inside the type's range
    mid, half = (lo + hi) / 2, max((hi - lo) / 2, 1e-6) * 0.9
    rng = (0, 255, 0, 255) if unsigned else (-128, 127, -128, 127)
    scale = 2 * half / 255
    return (one(scale), one(mid - half - rng[0] * scale)) + rng


def place(t, dev, shift=0):
    """the byte tensor t on `dev` with its storage copied whole -- strides, padding and what the padding holds are kept -- and moved
    `shift` bytes off the allocation's base (1: every 16-byte alignment is lost)"""
    flat = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage())
    raw = torch.empty(flat.numel() + shift, dtype=t.dtype, device=dev)
    raw[shift:].copy_(flat)
    return raw.as_strided(tuple(t.shape), tuple(t.stride()), t.storage_offset() + shift)


def to(dev, args, shift=()):
    """`args` on `dev`: level tensors through `place` (those at the positions `shift` one byte off), the rest as they are"""
    if str(dev) == "cpu":
        return tuple(args)
    return tuple(place(a, dev, 1 if i in shift else 0) if isinstance(a, torch.Tensor) and a.dtype in (U8, I8) and a.dim() >= 2
                 else (a.to(dev) if isinstance(a, torch.Tensor) else a) for i, a in enumerate(args))


def run_bmm(dev, operands, q, mid, shift=()):
    ops = torch.ops.torchlsq
    a = to(dev, operands, shift)
    if q is None:
        return ops.lsq_bmm_w8_q8(*a, mid)
    return ops.lsq_bmm_w8_q8_q(*a, *to(dev, q), mid)


def bmm_int_reference(a, z_a, b, z_b, nt):
    """I by plain Python integers (tiny shapes only): a list of lists per batch"""
    a, b = a.reshape((-1,) + tuple(a.shape[-2:])).tolist(), b.reshape((-1,) + tuple(b.shape[-2:])).tolist()
    za, zb = int(z_a), int(z_b)
    out = []
    for ab, bb in zip(a, b):
        if not nt:
            bb = [list(col) for col in zip(*bb)]
        out.append([[sum((x - za) * (y - zb) for x, y in zip(row, col)) for col in bb] for row in ab])
    return out


# ---------------------------------------------------------------------------------------------------
# softmax
# ---------------------------------------------------------------------------------------------------
TRIALS = ((0.05, 1.0, 197), (0.1, 0.125, 197), (0.02, 1.0, 1024), (0.3, 1.0, 64), (0.004, 1.0, 65536))
PROB_Q = (one(1.0 / 255), one(0.0), 0, 255, 0, 255)


@functools.lru_cache(maxsize=None)
def table(s_x=0.05, alpha=1.0):
    """built ONCE on the CPU: the GPU tests move it"""
    from torchlsq.functional import lsq_softmax_table
    return lsq_softmax_table(one(s_x), alpha)


def table_with_zeros():
    t = table(0.3, 1.0).clone()
    assert int(t[0]) == 1 << 24 and int((t == 0).sum()) > 100
    return t


def full_table():
    return torch.full((256,), 1 << 24, dtype=torch.int32)


def score_rows(R, C, seed, dtype, spread=40):
    """rows of levels as attention scores are: a bulk of `spread` levels with a few rows' maxima far above it"""
    g = gen(seed)
    x = (torch.randn(R, C, generator=g) * spread / 4 + 128).round().clamp(0, 255)
    x[::2, 0] = 255
    raw = x.to(U8)
    return raw if dtype == U8 else (raw.to(torch.int16) - 128).to(I8)


def run_softmax(dev, x, tab, q, mid, row_pad=1, shift=()):
    ops = torch.ops.torchlsq
    x, = to(dev, (x,), shift)
    if q is None:
        return ops.lsq_softmax_w8_q8(x, tab.to(dev), mid)
    return ops.lsq_softmax_w8_q8_q(x, tab.to(dev), *to(dev, q), mid, row_pad)


def softmax_numpy(x, tab):
    """(E, S, p float32) of the definition step by step in numpy: int64 sums, one float32 division, one float32 multiply"""
    b = x.numpy().astype(np.int64)
    E = tab.numpy().astype(np.int64)[b.max(-1, keepdims=True) - b]
    S = E.sum(-1, keepdims=True)
    r = np.float32(1.0) / S.astype(np.float32)
    return E, S, E.astype(np.float32) * r


def softmax_bound(p, p_star, S, C):
    """the header's bound on |p - p*|, p* the softmax in real arithmetic (here: float64): 2^-22 p + (1 + C p*) / (2 S); the factor
    covers the last place of the float64 exp behind an entry (far below 2^-20 of half a unit)"""
    return 2.0 ** -22 * p + (1 + C * p_star) / (2 * S) * (1 + 2.0 ** -20)


# ---------------------------------------------------------------------------------------------------
# the attention core
# ---------------------------------------------------------------------------------------------------
def trained(lo, hi):
    """a per-tensor quint8 LSQFakeQuantizer that has seen one batch, its scale and shift set to cover lo..hi, observer off, eval"""
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    q = LSQFakeQuantizer(observer=MovingAverageMinMaxObserver, otype="activation").train()
    q(torch.tensor([float(lo), float(hi)]))
    with torch.no_grad():
        q.scale.fill_((hi - lo) / (q.quant_max - q.quant_min))
        q.shift.fill_(lo)
    q.disable_observer()
    return q.eval()


QKV_S, QKV_Z = 0.03, 125


def qkv_heads(qkv, dev="cpu"):
    """q, k, v LevelsTensors [B, H, T, D] as views of one [B, T, 3, H, D] buffer"""
    from torchlsq.functional import LevelsTensor
    buf = qkv if str(dev) == "cpu" else qkv.to(dev)
    s, z = one(QKV_S).to(dev), one(QKV_Z, torch.int32).to(dev)
    return [LevelsTensor(buf[:, :, i].permute(0, 2, 1, 3), s, z, 0, 255) for i in range(3)]


@functools.lru_cache(maxsize=None)
def core_case(B, H, T, D, seed=0):
    """(the module on the CPU, the qkv buffer, the CPU core's LevelsTensor); the softmax table is built here, once"""
    from torchlsq.quantized import AttentionCoreW8Q
    span = 6.0 * QKV_S * QKV_S * 74 * 74 * D ** 0.5          # six sigma of a score of uniform levels
    core = AttentionCoreW8Q(trained(-span, span), trained(0.0, 1.0), trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16)
    qkv = levels((B, T, 3, H, D), 50 + seed, U8)
    return core, qkv, core(*qkv_heads(qkv))
