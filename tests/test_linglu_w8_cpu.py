"""The gate and up linears of a gated MLP's decode step with the gated product in their epilogue (include/lsq_hip_linglu_w8.h) on
CPU tensors, and what the GPU tests share.  `lsq_linear_w8_q8_dec_glu_q` defines nothing new, so the reference is PLAIN:
tests/test_lindec_w8_cpu.py's `reference` (an int64 matmul and the contract's float32 steps) gives the gate and the up bytes, and
tests/glu_w8_cases.py's numpy arithmetic the product on them.  Every comparison is on the bytes."""
import functools

import numpy as np
import pytest
import torch

import eltwise_w8_cases as E
import glu_w8_cases as G
import requant_w8_cases as R
import test_lindec_w8_cpu as L
from torchlsq import extension, functional as F

OPS = torch.ops.torchlsq
U8, I8 = torch.uint8, torch.int8
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


@functools.lru_cache(maxsize=None)
def case(M, C, K, x_dt=U8, w_dt=I8, gate_u=True, up_u=True, out_u=True, mid=BF16, bias="f32", fn="silu", act_q=False, fused=True):
    """CPU operands of one case, built once and left unchanged: `gate` and `up` (the twelve of R.linear_case on ONE x; `fused`: the
    two weights are the halves of one [2 C, K] tensor and up takes gate's quantizer), `up_q` (the constants of up's levels),
    `table`, `out` (the product's quantizer, chosen from the reference values), `want` (the plain reference's bytes)"""
    zx = 117 if x_dt == U8 else -11
    gate = R.linear_case(M, C, K, (x_dt, zx, w_dt, None, None, bias), (gate_u, False, mid), 0)
    up = R.linear_case(M, C, K, (x_dt, zx, w_dt, None, None, bias), (up_u, False, mid), 50)
    up = gate[:3] + up[3:]
    if fused:
        both = [None if a is None else torch.cat((a, b)) for a, b in zip(gate[3:7], up[3:7])]
        gate = gate[:3] + tuple(None if t is None else t[:C] for t in both) + gate[7:]
        up = gate[:3] + tuple(None if t is None else t[C:] for t in both) + gate[7:]
    return _with_product(gate, up, out_u, mid, fn, act_q, (M, C, K))


@functools.lru_cache(maxsize=None)
def extreme_case():
    """K = 65536, M = C = 16 on tests/test_lindec_w8_cpu.py's `extreme_lin`: the gate strip is its 16 weight rows, the up strip the same
    rows in reverse order, so the outputs (15, 14) and (15, 15) of the gate and (15, 1) and (15, 0) of the up projection have the raw
    int32 sum at 2^30 and |I| = 65536 * 255 * 255 > 2^31"""
    gate = L.extreme_lin()
    up = gate[:3] + tuple(t.flip(0).contiguous() for t in gate[3:7]) + gate[7:]
    return _with_product(gate, up, True, F32, "silu", False, "K = 65536")


def _with_product(gate, up, out_u, mid, fn, act_q, note):
    """the case of two projections' operands: the product's table, its quantizer and the plain reference's bytes"""
    gb, ub = L.reference(dict(lin=gate, res=None)), L.reference(dict(lin=up, res=None))
    s_g, z_g = F._act_constants(gate[7], gate[8], *gate[9][2:])
    s_u, z_u = F._act_constants(up[7], up[8], *up[9][2:])
    act = None
    if act_q:                                       # a uint8 quantizer on the activation's values over the 256 gate levels
        call, _ = F.act_function(fn)
        v = call(F.LevelsTensor(torch.arange(256, dtype=U8).view(gb.dtype), s_g, z_g, 0, 255).dequantize(F32))
        act = (E.one(float(v.max() - v.min()) / 255.0), E.one(float(v.min())), 0, 255, 0, 255)
    table = F.lsq_glu_table(fn, s_g, z_g, gb.dtype, act, mid)
    f = np.float32                                  # glu_w8_cases.numpy_value's steps on the two byte tensors
    a = E.round_to(table.numpy(), mid)[gb.view(U8).numpy().astype(np.int64)]
    d = E.round_to(((ub.numpy().astype(f) - f(int(z_u))) * f(float(s_u))).astype(f), mid)
    t = E.round_to((a * d).astype(f), mid)
    osc, osh, rng = G.out_quantizer(torch.from_numpy(t), out_u)
    lv = torch.from_numpy(E.numpy_levels(t, osc, osh, rng))
    c = dict(gate=gate, up=up, up_q=(s_u, z_u), table=table, out=(osc, osh, rng), mid=mid, want=lv.to(U8) if out_u else lv.to(I8))
    R.assert_not_vacuous(c["want"], rng, note)
    return c


def args_of(c, device="cpu"):
    """the op's arguments, the tensors on `device`; the halves of a fused weight stay views of ONE tensor there"""
    g, u = c["gate"], c["up"]
    if g[3].untyped_storage().data_ptr() == u[3].untyped_storage().data_ptr():
        both = [None if a is None else a.as_strided((2 * a.shape[0],) + tuple(a.shape[1:]), a.stride()).to(device) for a in g[3:7]]
        C = g[3].shape[0]
        gw, uw = [None if t is None else t[:C] for t in both], [None if t is None else t[C:] for t in both]
    else:
        gw, uw = R.to(device, *g[3:7]), R.to(device, *u[3:7])
    gq, uq = R.to(device, *g[7:9]), R.to(device, *u[7:9])
    return (*R.to(device, *g[:3]), *gw, *gq, *g[9], *uw, *(gq if g[7] is u[7] else uq), *u[9], *R.to(device, *c["up_q"], c["table"], *c["out"][:2]),
            *c["out"][2], c["mid"])


def two_launches(args):
    """the route of before: `lsq_linear_w8_q8_dec_q` on gate and on up, then `lsq_glu_w8_q8_q`"""
    x, mid = args[:3], args[-1]
    gl = OPS.lsq_linear_w8_q8_dec_q(*x, *args[3:13], False, mid)
    ul = OPS.lsq_linear_w8_q8_dec_q(*x, *args[13:23], False, mid)
    return OPS.lsq_glu_w8_q8_q(gl, ul, *args[23:])


# (M, C, K, x, weight, gate / up / product levels unsigned, mid_dtype, bias, function, activation quantizer, fused)
CPU_CASES = [(3, 40, 272, U8, I8, True, True, True, F32, "f32", "silu", False, True),
             (16, 48, 16, I8, U8, False, True, False, BF16, None, "gelu_tanh", True, False),
             (16, 16, 4112, U8, I8, True, False, True, F16, "f32", "silu", True, False)]


@pytest.mark.parametrize("spec", CPU_CASES, ids=lambda s: "-".join(str(v).replace("torch.", "") for v in s))
def test_cpu_op_equals_the_plain_reference(spec):
    c = case(*spec)
    got = OPS.lsq_linear_w8_q8_dec_glu_q(*args_of(c))
    assert got.dtype == c["want"].dtype and torch.equal(got, c["want"])
    assert torch.equal(two_launches(args_of(c)), c["want"])


@pytest.mark.parametrize("args, want", [
    ((16, 4096, 4096), dict(served=True, block=1024, chunks=1, x_resident=True, store="packets", lds_bytes=35840 + 768 + 1024 + 16 * 4112)),
    ((1, 4096, 4112), dict(served=True, chunks=2, x_resident=False, lds_bytes=35840 + 768 + 1024 + 4112)),
    ((3, 40, 272), dict(served=True, grid=3, chunks=1, store="bytes", lds_bytes=35840 + 768 + 1024 + 3 * (512 + 16))),
    ((1, 64, 4096, True, False), dict(served=True, grid=4, store="bytes")),
    ((17, 4096, 4096), dict(served=False, grid=0, block=0, lds_bytes=0)),
    ((16, 16, 65536), dict(served=True, grid=1, chunks=16)),
    ((16, 16, 65552), dict(served=False)),
    ((1, 64, 24), dict(served=False)),
    ((1, 64, 4096, False), dict(served=False)),
])
def test_plan(args, want):
    pl = extension.linglu_w8_plan(*args)
    assert {k: pl[k] for k in want} == want, pl


def _mlp(shared):
    from torchlsq.quantized import convert_w8a8_glu
    net, qs, x = G.mlp_block(shared=shared)
    return convert_w8a8_glu(net, {"mlp": G.mlp_quantizers(qs)}, mid_dtype=BF16, glu_epilogue=None).mlp, \
        F.LevelsTensor.from_quantized(qs["in"].quantize(x))


@pytest.mark.parametrize("shared", [True, False], ids=["fused", "pair"])
def test_switch_keeps_the_old_ops_result(shared, monkeypatch):
    """glu_epilogue=True with 17 rows and glu_epilogue=False never reach the new op; with 16 rows True and a True default do"""
    mlp, x = _mlp(shared)
    assert mlp.fused is shared and mlp.glu_epilogue is None
    calls = []
    monkeypatch.setattr(type(mlp), "_product_in_epilogue", lambda self, xl, f=type(mlp)._product_in_epilogue: calls.append(1) or f(self, xl))
    x17, x16 = (F.LevelsTensor(x.levels[:n], x.scale, x.zero_point, x.quant_min, x.quant_max) for n in (17, 16))
    mlp.glu_epilogue = False
    want17, want16 = mlp(x17, x17).levels, mlp(x16, x16).levels
    for xl, want, flag, taken in ((x17, want17, True, False), (x16, want16, False, False), (x16, want16, None, F.W8A8_GLU_EPILOGUE_DEFAULT),
                                 (x16, want16, True, True)):
        mlp.glu_epilogue, n = flag, len(calls)
        assert torch.equal(mlp(xl, xl).levels, want) and (len(calls) > n) is taken, (flag, taken)


def test_module_keeps_glu_epilogue_in_its_state():
    a, _ = _mlp(True)
    old = {k: v for k, v in a.state_dict().items() if k != "_extra_state"}      # a state dict from before the attribute
    a.glu_epilogue = True
    b, _ = _mlp(True)
    b.load_state_dict(a.state_dict())
    assert b.glu_epilogue is True and set(a.state_dict()) - set(old) == {"_extra_state"}
    b.load_state_dict(old)
    assert b.glu_epilogue is None
