"""The decode-shape W8A8 linears with an 8-bit output (include/lsq_hip_lindec_w8.h) on CPU tensors, and what the GPU tests share:
`lsq_linear_w8_q8_dec_q` / `lsq_linear_w8_q8_dec_add_q` define nothing new, so the reference is PLAIN: an int64 matmul of
(lx - zx)(lw - zw), then the contract's float32 steps written out in torch.  Every comparison is on the bytes."""
import functools

import pytest
import torch

import qlinear_w8_cases as W
import requant_w8_cases as R
from torchlsq import extension, functional as F

OPS = torch.ops.torchlsq
U8, I8 = torch.uint8, torch.int8
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NONE, RES, PRE = 0, 1, 2            # no residual / a residual / a residual and the layer's own pre-quantizer


def _level(u, sc, sh, rng):
    """lsq_math.hpp's make_qparams and level() in float32 torch ops"""
    s = sc.abs().clamp_min(torch.finfo(F32).eps)
    inv = 1.0 / s
    zp = torch.fmin(torch.full_like(s, rng[3]), torch.fmax(torch.full_like(s, rng[2]), -sh * inv)).round()
    return torch.fmin(torch.full_like(s, rng[1]), torch.fmax(torch.full_like(s, rng[0]), u.float() * inv + zp)).round(), zp, s


def reference(c):
    """the bytes of one case from the exact int64 integer and the float32 steps of lsq_hip_requant_w8.h / lsq_hip_resadd_w8.h"""
    lx, s, z, lw, s_w, zw, bias, osc, osh, rng, relu, mid = c["lin"]
    I = (lx.to(torch.int64) - int(z)) @ (lw.to(torch.int64) - zw.to(torch.int64).reshape(-1, 1)).t()
    v = (s_w.reshape(1, -1) * I.to(F32)) * s
    if bias is not None:
        v = v + bias.float()
    u = v.to(mid)
    if c["res"] is not None:
        rl, rs, rz, psc, psh, p0, p1, p2, p3 = c["res"]
        if psc is not None:
            lv, zp, ps = _level(u, psc, psh, (p0, p1, p2, p3))
            u = ((lv - zp) * ps).to(mid)
        d = ((rl.float() - rz.float()) * rs).to(mid)
        u = (u.float() + d.float()).to(mid)
    if relu:
        u = torch.where(u < 0, torch.zeros_like(u), u)
    lv = _level(u, osc, osh, rng)[0].to(torch.int64)
    return lv.to(U8) if rng[1] > 127 else lv.to(I8)


@functools.lru_cache(maxsize=None)
def case(M, N, K, kind=NONE, x_dt=U8, w_dt=I8, r_dt=U8, unsigned=True, mid=BF16, relu=False, bias="f32", seed=0):
    """CPU operands of one case, built once and left unchanged: `lin` (the twelve of R.linear_case), `res` (the nine residual
    arguments or None), `want` (the plain reference's bytes, held to requant_w8_cases' condition)"""
    zx = 117 if x_dt == U8 else -11
    lin = R.linear_case(M, N, K, (x_dt, zx, w_dt, None, None, bias), (unsigned, relu, mid), seed)
    res = None
    if kind != NONE:
        lo, hi = W.LEVEL_RANGE[r_dt]
        osc, wide = lin[7], (2.2 if relu else 1.1)      # the pre-quantizer's range reaches past the output's borders
        res = (W.levels((M, N), lo, hi, seed + 7), 0.4 * osc, torch.tensor([(lo + hi + 1) // 2], dtype=torch.int32)) + \
            ((wide * osc, -128 * wide * osc, 0, 255, 0, 255) if kind == PRE else (None, None, 0, 255, 0, 255))
    c = dict(lin=lin, res=res)
    c["want"] = reference(c)
    R.assert_not_vacuous(c["want"], lin[9], (M, N, K, kind))
    return c


@functools.lru_cache(maxsize=None)
def extreme_lin(N=16):
    """The twelve operands of the K = 65536, M = 16 case at the borders of what is served, on N weight rows (row n as row n % 16):
    row m of x holds level 0 on its first 4096 (m + 1) k and 255 after them, against zx = 255; an even row of w holds -128 on a prefix
    and 127 after it against zw = 127, an odd one 127 and then -128 against zw = -128.  So (15, 14) has every raw product at 2^14, the
    raw int32 sum at 2^30 and I = 65536 * 255 * 255 > 2^31, and (15, 15) has I = -65536 * 255 * 255"""
    K, k = 65536, torch.arange(65536)
    m, n = torch.arange(16).reshape(16, 1), (torch.arange(N) % 16).reshape(N, 1)
    lx = torch.where(k < (m + 1) * 4096, 0, 255).to(U8)
    even = n % 2 == 0
    lw = torch.where((k < (n // 2 * 2 + 2) * 4096) == even, -128, 127).to(I8)
    s, z = torch.tensor([2.0 ** -10]), torch.tensor([255], dtype=torch.int32)
    s_w, zw = torch.full((N,), 2.0 ** -12), torch.where(even.flatten(), 127, -128).to(torch.int32)
    I = (lx.long() - 255) @ (lw.long() - zw.long().reshape(-1, 1)).t()
    assert int(I[15, 14]) == K * 255 * 255 > 2 ** 31 and int(I[15, 15]) == -K * 255 * 255 and int((lx[15].long() - 128) @ lw[14].long()) == 2 ** 30
    bias = torch.zeros(N)
    osc, osh, rng = R.out_quantizer((s_w * I.float()) * s + bias, True, False)
    return (lx, s, z, lw, s_w, zw, bias, osc, osh, rng, False, F32)


def moved(c, device):
    res = None if c["res"] is None else tuple(R.to(device, *c["res"][:5])) + tuple(c["res"][5:])
    return dict(lin=tuple(R.to(device, *c["lin"][:9])) + tuple(c["lin"][9:]), res=res)


def run(c, device="cpu", dec=True, out=None):
    """the new (dec) or the existing op on the case's operands moved to `device`"""
    c = moved(c, device)
    lin, res = list(c["lin"]), c["res"]
    args = lin[:9] + list(lin[9]) + lin[10:]
    if res is None:
        return (extension.lindec_w8_linear_levels if dec else extension.requant_w8_linear_levels)(*args, out=out)
    return (extension.lindec_w8_linear_levels_add if dec else extension.resadd_w8_linear_levels)(*args, *res, out=out)


CPU_CASES = [(3, 40, 272, NONE, U8, I8, U8, True, F32, False, "f32"),
             (16, 16, 64, NONE, I8, U8, U8, False, BF16, False, None),
             (16, 1024, 64, NONE, U8, I8, U8, True, F16, True, "f32"),
             (3, 40, 272, RES, U8, I8, I8, True, BF16, False, "f32"),
             (16, 16, 64, RES, I8, U8, U8, False, F32, False, None),
             (3, 40, 272, PRE, U8, I8, U8, True, F16, False, "f32"),
             (16, 1024, 64, PRE, U8, I8, I8, True, BF16, True, "f32")]


@pytest.mark.parametrize("spec", CPU_CASES, ids=lambda s: "-".join(str(v).replace("torch.", "") for v in s))
def test_cpu_ops_equal_the_plain_reference(spec):
    c = case(*spec)
    lin, res = c["lin"], c["res"]
    if res is None:
        got = OPS.lsq_linear_w8_q8_dec_q(*lin[:9], *lin[9], *lin[10:])
    else:
        got = OPS.lsq_linear_w8_q8_dec_add_q(*lin[:9], *lin[9], *lin[10:], *res)
    assert got.dtype == c["want"].dtype and torch.equal(got, c["want"])
    assert torch.equal(run(c, dec=False), c["want"])


@pytest.mark.parametrize("args, want", [
    ((16, 4096, 4096), dict(served=True, block=1024, chunks=1, x_resident=True, store="packets", res_load="packets",
                            lds_bytes=18432 + 256 + 16 * 4112)),
    ((1, 4096, 4112), dict(served=True, chunks=2, x_resident=False, lds_bytes=18432 + 256 + 4112)),
    ((3, 40, 272), dict(served=True, grid=3, chunks=1, store="bytes", res_load="bytes", lds_bytes=18432 + 256 + 3 * (512 + 16))),
    ((17, 4096, 4096), dict(served=False, grid=0, block=0, lds_bytes=0)),
    ((16, 16, 65536), dict(served=True, grid=1, chunks=16)),
    ((16, 16, 65552), dict(served=False)),
    ((1, 64, 24), dict(served=False)),
    ((1, 64, 4096, False), dict(served=False)),
    ((1, 64, 4096, True, False, True), dict(served=True, grid=4, store="bytes", res_load="packets")),
    ((1, 64, 4096, True, True, False), dict(served=True, store="packets", res_load="bytes")),
])
def test_plan(args, want):
    pl = extension.lindec_w8_plan(*args)
    assert {k: pl[k] for k in want} == want, pl


@pytest.mark.parametrize("kind", [NONE, PRE])
def test_decode_switch_keeps_the_old_ops_result(kind, monkeypatch):
    """decode=True with 17 rows and decode=False never reach the new ops; with 16 rows decode=True and a True default do"""
    c17, c16 = case(17, 40, 64, kind), case(16, 40, 64, kind)
    called = []
    monkeypatch.setattr(F, "_takes_decode", lambda d, lv, f=F._takes_decode: called.append(f(d, lv)) or called[-1])

    def call(c, decode):
        lx, s, z, lw, s_w, zw, bias, osc, osh, rng, relu, mid = c["lin"]
        wq = torch._make_per_channel_quantized_tensor(lw, s_w.double(), zw.to(torch.int64), 0)
        kw = dict(out_scale=osc, out_shift=osh, out_quant_min=rng[0], out_quant_max=rng[1], relu=relu, mid_dtype=mid, decode=decode)
        x = F.LevelsTensor(lx, s, z, 0, 255)
        if c["res"] is None:
            return F.lsq_linear_w8a8_q(x, wq, bias, **kw).levels
        rl, rs, rz, psc, psh = c["res"][:5]
        return F.lsq_linear_w8a8_add_q(x, wq, bias, F.LevelsTensor(rl, rs, rz, 0, 255), pre_scale=psc, pre_shift=psh, pre_quant_min=0,
                                       pre_quant_max=255, **kw).levels

    for c, decode, taken in ((c17, True, False), (c17, False, False), (c16, False, False), (c16, None, F.W8A8_DECODE_DEFAULT), (c16, True, True)):
        assert torch.equal(call(c, decode), c["want"]) and called[-1] is taken, (decode, called[-1])


def test_module_keeps_decode_in_its_state():
    from torchlsq.quantized import LinearW8A8AddQ, LinearW8A8Q
    for cls in (LinearW8A8Q, LinearW8A8AddQ):
        m = cls(32, 16)
        assert m.decode is None
        old = {k: v for k, v in m.get_extra_state().items() if k != "decode"}
        m.decode = True
        n = cls(32, 16)
        n.load_state_dict(m.state_dict())
        assert n.decode is True
        n.set_extra_state(old)              # a state dict from before the attribute
        assert n.decode is None
