"""What tests/test_rope_w8_cpu.py and tests/test_rope_w8_gpu.py share: seeded levels, constants, tables and output sides, the ops run
on a device of choice, an independent numpy restatement of include/lsq_hip_rope_w8.h's formulas (np.float32 steps, the roundings to
mid through torch), the placement in plain Python, and the trained quantizers of the decode case.
"""
import numpy as np
import torch

F32, BF16, F16, U8, I8 = torch.float32, torch.bfloat16, torch.float16, torch.uint8, torch.int8
GUARD = 0xA5


def one(v, dtype=torch.float32):
    return torch.tensor([v], dtype=dtype)


OUT_U8 = (one(8.0 / 255), one(-4.0), 0, 255, 0, 255)               # covers -4 .. 4, zero point 128
OUT_I8 = (one(10.0 / 255), one(-5.0), -128, 127, -128, 127)        # zero point 0 in -128..127
SIDES = ((OUT_U8, BF16), (OUT_I8, F32), (OUT_U8, F16), (None, F32), (None, BF16), (None, F16))
UNIT = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}         # the unit roundoff of mid


def levels(shape, seed, dtype=U8):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(0, 256, tuple(shape), generator=g).to(torch.uint8).view(dtype if dtype == U8 else I8)


def constants(dtype):
    """(s_x, zx): real values within about -3.2 .. 3.2"""
    return (one(0.025), one(131, torch.int32)) if dtype == U8 else (one(0.025), one(-3, torch.int32))


def tables(R, P, mid, base=10000.0):
    from torchlsq.functional import lsq_rope_tables
    return lsq_rope_tables(R, P, base, mid)


def to(dev, ts):
    return tuple(t.to(dev) if isinstance(t, torch.Tensor) else t for t in ts)


def pos_tensor(positions, dev="cpu"):
    return None if positions is None else torch.tensor([int(v) for v in positions], dtype=torch.int32, device=dev)


def qkv_views(B, T, H, D, seed, dtype=U8, dev="cpu"):
    """the q and k views [B, T, H, D] of one [B, T, 3 H D] buffer"""
    buf = levels((B, T, 3 * H * D), seed, dtype).to(dev)
    v = buf.view(B, T, 3, H, D)
    return v[:, :, 0], v[:, :, 1]


def cache_view(B, H, Tmax, D, dtype, dev="cpu"):
    """(the whole buffer with GUARD bytes around a [B, H, Tmax, D] cache, the cache's [B, Tmax, H, D] view); the cache's first
    element is 64 elements into the buffer, so its base stays 16-byte aligned for every element size"""
    n = B * H * Tmax * D
    buf = torch.zeros(n + 128, dtype=dtype, device=dev)
    buf.view(torch.uint8).fill_(GUARD)
    return buf, buf[64:64 + n].view(B, H, Tmax, D).permute(0, 2, 1, 3)


def run_rope(dev, x, consts, cos, sin, q, mid, positions=None, interleaved=False, out=None, scatter=False):
    """the rotating ops on `dev` (with `out`: the host functions, as the functional layer calls them)"""
    from torchlsq import extension as E
    ops = torch.ops.torchlsq
    pt = positions.to(dev) if isinstance(positions, torch.Tensor) else pos_tensor(positions, dev)
    args = (x.to(dev),) + to(dev, consts) + (cos.to(dev), sin.to(dev))
    if out is not None:
        if q is None:
            return E.rope_w8(*args, mid, pt, interleaved, out=out, scatter=scatter)
        return E.rope_w8_q(*args, *to(dev, q), mid, pt, interleaved, out=out, scatter=scatter)
    if q is None:
        return ops.lsq_rope_w8_q8(*args, mid, pt, interleaved)
    return ops.lsq_rope_w8_q8_q(*args, *to(dev, q), mid, pt, interleaved)


def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same(got, want, note=""):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (note, got.dtype, want.dtype, got.shape, want.shape)
    assert torch.equal(bits(got.cpu().contiguous()), bits(want.cpu().contiguous())), note


def _rm(a, mid):
    """np.float32 array -> rounded to mid by torch -> np.float32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(mid).to(torch.float32).numpy()


def numpy_value(x, consts, cos, sin, mid, positions=None, interleaved=False):
    """u of the header's definition, np.float32 [B, T, H, D] (NaN rows for tokens whose position lies outside the tables): loops
    over pairs, one np.float32 operation per step"""
    B, T, H, D = x.shape
    P, half = cos.shape
    R = 2 * half
    s_x, zx = np.float32(consts[0].item()), np.float32(consts[1].item())
    d = _rm((x.numpy().astype(np.float32) - zx) * s_x, mid)
    c_t, s_t = cos.numpy(), sin.numpy()
    u = np.full((B, T, H, D), np.nan, dtype=np.float32)
    for b in range(B):
        for t in range(T):
            p = t + (0 if positions is None else int(positions[b]))
            if p < 0 or p >= P:
                continue
            u[b, t, :, R:] = d[b, t, :, R:]
            for col in range(half):
                i, j = (2 * col, 2 * col + 1) if interleaved else (col, col + half)
                c, s = c_t[p, col], s_t[p, col]
                di, dj = d[b, t, :, i], d[b, t, :, j]
                u[b, t, :, i] = _rm(_rm(di * c, mid) - _rm(dj * s, mid), mid)
                u[b, t, :, j] = _rm(_rm(dj * c, mid) + _rm(di * s, mid), mid)
    return u


def finish(u, q, mid):
    """u (np.float32 or a tensor) through the output side with the EXISTING levels op, or as mid"""
    u = (torch.from_numpy(u) if isinstance(u, np.ndarray) else u).to(mid)
    if q is None:
        return u
    lv = torch.ops.torchlsq.lsq_levels_per_tensor(u.contiguous(), *q, 0)
    return lv.view(U8) if max(q[3], q[5]) > 127 else lv


def placed(y0, val, positions, limit, scatter):
    """the placement of the definition, token by token in Python: a copy of y0 [B, Tout, H, D] with val's tokens where they go"""
    y = y0.clone()
    B, T = val.shape[:2]
    Tout = y.shape[1]
    for b in range(B):
        for t in range(T):
            p = t + (0 if positions is None else int(positions[b]))
            if p < 0 or p >= limit or (scatter and p >= Tout):
                continue
            y[b, p if scatter else t] = val[b, t]
    return y


def hf_composed(x, consts, cos, sin, q, mid, positions=None):
    """the composition of EXISTING ops, HF style: dequantize(mid) -> x * cos + rotate_half(x) * sin in mid -> lsq_levels_per_tensor;
    every position must lie inside the tables; partial rotary passes the rest through"""
    from torchlsq.functional import LevelsTensor
    B, T, H, D = x.shape
    R = 2 * cos.shape[1]
    d = LevelsTensor(x, consts[0], consts[1], 0, 255).dequantize(mid)
    p = torch.arange(T).reshape(1, T) + (0 if positions is None else torch.tensor(positions).reshape(B, 1))
    c = torch.cat((cos[p], cos[p]), -1).to(mid).unsqueeze(2)
    s = torch.cat((sin[p], sin[p]), -1).to(mid).unsqueeze(2)
    xr = d[..., :R]
    rh = torch.cat((-xr[..., R // 2:], xr[..., :R // 2]), -1)
    return finish(torch.cat((xr * c + rh * s, d[..., R:]), -1), q, mid)


def trained(lo, hi):
    """a per-tensor quint8 activation quantizer that has seen one batch, its scale and shift set to cover lo..hi"""
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    fq = LSQFakeQuantizer(observer=MovingAverageMinMaxObserver, otype="activation").train()
    fq(torch.tensor([lo, hi]))
    with torch.no_grad():
        fq.scale.fill_((hi - lo) / (fq.quant_max - fq.quant_min))
        fq.shift.fill_(lo)
    fq.disable_observer()
    return fq.eval()


_DECODE = {}


def decode_case():
    """B 2, H 3, T 7, D 32: the qkv levels, the modules, and the prefill's context [B, T, H D] on the CPU -- computed once"""
    if not _DECODE:
        from torchlsq.functional import LevelsTensor
        from torchlsq.quantized import AttentionCoreW8Q, RotaryW8Q
        B, H, T, D = 2, 3, 7, 32
        qkv = levels((B, T, 3, H, D), 77)
        consts = constants(U8)
        rot = RotaryW8Q(trained(-4.0, 4.0), D, 16, mid_dtype=BF16)
        core = AttentionCoreW8Q(trained(-60.0, 60.0), trained(0.0, 1.0), trained(-3.0, 3.0), alpha=D ** -0.5, mid_dtype=BF16, causal=True)
        q, k, v = (LevelsTensor(qkv[:, :, i], *consts, 0, 255) for i in range(3))
        rq, rk = rot(q), rot(k)
        heads = lambda lt: LevelsTensor(lt.levels.permute(0, 2, 1, 3), lt.scale, lt.zero_point, lt.quant_min, lt.quant_max)   # noqa: E731
        prefill = core(heads(rq), heads(rk), heads(v)).levels
        _DECODE.update(B=B, H=H, T=T, D=D, Tmax=16, qkv=qkv, consts=consts, rot=rot, core=core, prefill=prefill)
    return _DECODE


def decode_step(case, rot, core, cache, t, dev="cpu"):
    """step t of the decode on `dev`: q and k of token t rotated at the cache's lengths, k and v appended, the masked core on the
    cache -> the context's levels [B, 1, H D]"""
    from torchlsq.functional import LevelsTensor
    tok = case["qkv"][:, t:t + 1].to(dev)
    q, k, v = (LevelsTensor(tok[:, :, i], *to(dev, case["consts"]), 0, 255) for i in range(3))
    rq = rot(q, positions=cache.lengths)
    kl, vl, lens = cache.append(k, v, rotary=rot)
    return core(LevelsTensor(rq.levels.permute(0, 2, 1, 3), rq.scale, rq.zero_point, rq.quant_min, rq.quant_max), kl, vl, key_lengths=lens).levels
