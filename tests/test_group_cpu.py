"""CPU: the group-wise ops (include/lsq_hip_group.h, liblsq_hip_group.so, torchlsq.functional.lsq_per_group) without a GPU.

  * the group library exports exactly what its header declares (the single and the fused calls), ABI 2, nothing named
    lsq_hip_*, and reads no environment;
  * its gfx950 code objects follow the main library's device-code rules (tests/test_device_code.py);
  * argument validation and the launch plan, host only;
  * the CPU op is, bit for bit, the oracle's per-channel op on the [numel // G, G] view;
  * LSQFakeQuantizer(group_size=...): construction errors, parameter shapes, state_dict round trip.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from helpers import assert_bits_equal, assert_reduction_close, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_group.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_group.so")


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lsq_\w+)\s*\(", text)))


def test_group_library_exports_its_eight_entry_points():
    from torchlsq import extension as E
    names = _declared()
    assert names == sorted(["lsq_group_abi_version", "lsq_group_last_error", "lsq_group_forward", "lsq_group_backward",
                            "lsq_group_plan", "lsq_group_multi_forward", "lsq_group_multi_backward", "lsq_group_multi_plan"])
    assert sorted(E.C_ABI_GROUP) == names
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == names
    assert "lsq_hip_" not in nm and "debug" not in nm
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und and "lsq_hip_" not in und and "lsq_group_" not in und
    lib = E.group_library()
    assert lib.lsq_group_abi_version() == E.GROUP_ABI_VERSION == 2
    assert re.search(r"#define LSQ_GROUP_MULTI_ITEMS (\d+)", open(HEADER).read()).group(1) == str(E.GROUP_MULTI_ITEMS)
    # the main library's ABI is untouched: its ctypes table has no group symbol
    assert not [n for n in E.C_ABI if "group" in n]


@pytest.fixture(scope="module")
def group_kernels(tmp_path_factory):
    every = gfx950_kernels(LIB, str(tmp_path_factory.mktemp("grpcode")))
    # the library holds the single-tensor kernels and the fused calls' (tests/test_group_foreach_cpu.py), nothing else
    assert all(re.search(r"(fwd|bwd)_grp_(multi_)?kernel", n) for n in every), sorted(every)
    out = {n: v for n, v in every.items() if "_grp_kernel" in n}
    # 4 storage types x (forward: init x levels x form = 8; backward: 6 mode combinations x 3 reductions = 18)
    assert len([n for n in out if "fwd_grp_kernel" in n]) == 32 and len([n for n in out if "bwd_grp_kernel" in n]) == 72, sorted(out)
    return out


def _ops(body):
    return re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)


def test_group_kernels_follow_the_device_code_rules(group_kernels):
    """no scratch, no v_fma_mix, contraction off (FMAs only inside the correctly rounded division), 16-byte packets"""
    packets = 0
    for name, (body, scratch) in group_kernels.items():
        ops = _ops(body)
        assert scratch == 0 and not [o for o in ops if o.startswith("scratch_")], "%s uses %d bytes of scratch" % (name, scratch)
        assert not [o for o in ops if o.startswith("v_fma_mix") or o.startswith("v_mad_mix")], name
        n_fma = sum(1 for o in ops if re.fullmatch(r"v_(fma|fmac|mad|mac)_f(32|64)(_e32|_e64)?", o))
        n_div = sum(1 for o in ops if o.startswith("v_div_fmas_f"))
        assert n_fma <= 5 * n_div, "%s: %d FMAs for %d divisions" % (name, n_fma, n_div)
        # packet form (forward PACKET = true: template argument Lb1E; backward modes 0 and 1): dwordx4 in and out
        packet = re.search(r"fwd_grp_kernelI.*Lb1EEEv", name) or re.search(r"bwd_grp_kernelI.*Li[01]EEEv", name)
        if packet:
            assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops, name
            packets += 1
    assert packets >= 16 + 48


def _lib():
    from torchlsq import extension as E
    return E, E.group_library()


def test_argument_validation_without_a_gpu():
    E, lib = _lib()
    p = E.LsqParams(-8, 7, -128, 127, 1, 1, 0, 0, 1.0, 0)
    ok = 1 << 20

    def fwd(code=E.LSQ_F32, x=ok, y=ok, n=256, G=32, sc=ok, sh=ok, pp=ctypes.byref(p), ex=None):
        return lib.lsq_group_forward(code, x, y, n, G, sc, sh, pp, ex, None)

    def bwd(code=E.LSQ_F32, g=ok, x=ok, dx=ok, ds=ok, db=ok, n=256, G=32, sc=ok, sh=ok, pp=ctypes.byref(p)):
        return lib.lsq_group_backward(code, g, x, dx, ds, db, n, G, sc, sh, pp, None)

    def err():
        return lib.lsq_group_last_error()

    for call in (fwd, bwd):
        assert call(G=0) == -1 and b"group_size" in err()
        assert call(G=-4) == -1 and b"group_size" in err()
        assert call(n=250) == -1 and b"multiple of group_size" in err()
        assert call(n=-32) == -1 and b"negative" in err()
        assert call(code=7) == -1 and b"dtype" in err()
        assert call(pp=None) == -1 and b"NULL" in err()
        assert call(x=None) == -1 and b"NULL" in err()
        assert call(sc=None) == -1 and b"NULL" in err()
        assert call(x=ok + 2) == -1 and b"element-aligned" in err()
        assert call(code=E.LSQ_F64, x=ok + 4) == -1 and b"element-aligned" in err()
        assert call(sc=ok + 2) == -1 and b"element-aligned" in err()
    assert fwd(y=ok + 1, code=E.LSQ_BF16) == -1 and b"element-aligned" in err()
    assert bwd(dx=ok + 2) == -1 and bwd(g=ok + 2) == -1 and bwd(ds=None) == -1 and bwd(db=ok + 1) == -1
    assert fwd(y=None) == -1 and b"NULL" in err()                                  # y == NULL needs levels
    wide = E.LsqParams(-200, 127, -200, 255, 1, 0, 0, 0, 1.0, 0)
    ex = E.LsqFwdExtras(ok, 0, 0)
    assert fwd(y=None, pp=ctypes.byref(wide), ex=ctypes.byref(ex)) == -1 and b"neither int8 nor uint8" in err()
    bad = E.LsqParams(7, -8, -128, 127, 1, 1, 0, 0, 1.0, 0)
    assert fwd(pp=ctypes.byref(bad)) == -1 and b"quant_min" in err()
    # nothing to do is not an error (no launch)
    assert fwd(n=0) == 0 and bwd(n=0) == 0


def test_plan_reports_the_form_and_the_reduction():
    from torchlsq import extension as E
    for dtype, V in ((torch.float32, 4), (torch.float64, 2), (torch.bfloat16, 8), (torch.float16, 8)):
        for G in (8, 16, 32, 64, 128, 256, 4096, 24 * V):
            n = G * 8192
            p = E.group_plan(dtype, n, G)
            assert p["form"] == "packet" and p["lanes_per_group"] == G // V and p["vec"] == V and p["block"] == 256, (dtype, G, p)
            pow2 = (G // V) & (G // V - 1) == 0
            assert p["reduction"] == ("butterfly" if pow2 else "scan"), (dtype, G, p)
            assert 1 <= p["fwd_grid"] <= 256 * 16 and 1 <= p["bwd_grid"]
        for G in (1, 3, 7, V + 1):
            p = E.group_plan(dtype, G * 7 * 1024, G)
            assert p["form"] == "element" and p["reduction"] == "scan" and p["lanes_per_group"] == G
    with pytest.raises(RuntimeError, match="multiple of group_size"):
        E.group_plan(torch.float32, 100, 32)


def _oracle_case(dtype, G, rows, K, seed, qmin=-8, qmax=7, tmin=-128, tmax=127):
    rng = np.random.default_rng(seed)
    npd = {torch.float32: np.float32, torch.float64: np.float64}[dtype]
    x = (rng.standard_normal((rows, K)) * 0.3).astype(npd)
    x.reshape(-1)[::97] = 0.0
    ng = rows * K // G
    s = (rng.random(ng) * 0.05 + 0.01).astype(npd)
    s[::5] *= -1.0
    b = (rng.standard_normal(ng) * 0.02).astype(npd)
    g = rng.standard_normal((rows, K)).astype(npd)
    return x, s, b, g, ng


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("G", [1, 3, 8, 32, 128, 384])
@pytest.mark.parametrize("mode", ["affine", "sym", "init", "eval"])
def test_cpu_op_equals_the_oracle_on_the_reshape(dtype, G, mode):
    from oracle import lsq_oracle as O
    from torchlsq import extension  # noqa: F401
    rows, K = 6, 768
    x, s, b, g, ng = _oracle_case(dtype, G, rows, K, G * 7 + len(mode))
    qmin, qmax, tmin, tmax = (-8, 7, -128, 127) if mode == "sym" else (0, 15, 0, 255)
    sym, init, ev = mode == "sym", mode == "init", mode == "eval"
    shape_p = (rows, K // G)
    y = torch.ops.torchlsq.lsq_forward_per_group(torch.from_numpy(x), torch.from_numpy(s).reshape(shape_p),
                                                 torch.from_numpy(b).reshape(shape_p), G, qmin, qmax, tmin, tmax, True, 0.5, sym,
                                                 ev, init)
    oy = O.fwd_pc(x, s, b, 1, ng, G, qmin, qmax, tmin, tmax, init_mode=init)
    assert_bits_equal(y.numpy(), oy.reshape(rows, K), "y")
    dx, ds, db = torch.ops.torchlsq.lsq_backward_per_group(torch.from_numpy(g), torch.from_numpy(x),
                                                           torch.from_numpy(s).reshape(shape_p), torch.from_numpy(b).reshape(shape_p),
                                                           G, qmin, qmax, tmin, tmax, True, 0.5, sym, ev, init)
    r = O.bwd_pc(g, x, s, b, 1, ng, G, qmin, qmax, tmin, tmax, True, 0.5, sym, ev, init)
    assert ds.shape == shape_p and db.shape == shape_p
    assert_bits_equal(dx.numpy(), r.dx.reshape(rows, K), "dx")
    assert_reduction_close(ds.numpy(), r.ds_wide, r.abs_ds, "d_scale")
    assert_reduction_close(db.numpy(), r.db_wide, r.abs_db, "d_shift")
    lv = torch.ops.torchlsq.lsq_levels_per_group(torch.from_numpy(x), torch.from_numpy(s), torch.from_numpy(b), G, qmin, qmax,
                                                 tmin, tmax, 0)
    assert np.array_equal(lv.numpy().astype(np.int32).reshape(-1),
                          O.levels_pc(x, s, b, 1, ng, G, qmin, qmax, tmin, tmax).reshape(-1))


def test_functional_matches_per_channel_lsq_and_repeats_scalar_parameters():
    from torchlsq.functional import lsq, lsq_per_group
    torch.manual_seed(0)
    x = torch.randn(4, 3, 64)
    s = torch.rand(4, 3, 2) * 0.05 + 0.01
    b = torch.randn(4, 3, 2) * 0.01
    xs, ss, bs = (t.clone().requires_grad_() for t in (x, s, b))
    y = lsq_per_group(xs, ss, bs, 32, -8, 7, use_grad_scaling=True, grad_scaler=0.7)
    gout = torch.randn_like(x)
    y.backward(gout)
    x2, s2, b2 = x.reshape(-1, 32).clone().requires_grad_(), s.reshape(-1).clone().requires_grad_(), b.reshape(-1).clone().requires_grad_()
    y2 = lsq(x2, s2, b2, -8, 7, axis=0, is_perchannel=True, grad_scaler=0.7)
    y2.backward(gout.reshape(-1, 32))
    assert torch.equal(y, y2.reshape(x.shape)) and torch.equal(xs.grad, x2.grad.reshape(x.shape))
    assert ss.grad.shape == s.shape and torch.equal(ss.grad.reshape(-1), s2.grad) and torch.equal(bs.grad.reshape(-1), b2.grad)
    # one-element parameters are repeated once per group; their gradient is the sum
    s1, b1 = torch.tensor([0.02], requires_grad=True), torch.tensor([0.001], requires_grad=True)
    y = lsq_per_group(x, s1, b1, 16, 0, 15)
    y.sum().backward()
    ng = x.numel() // 16
    s3, b3 = torch.full((ng,), 0.02, requires_grad=True), torch.full((ng,), 0.001, requires_grad=True)
    lsq_per_group(x, s3, b3, 16, 0, 15).sum().backward()
    assert s1.grad.shape == (1,) and torch.allclose(s1.grad, s3.grad.sum(), rtol=1e-5)
    with pytest.raises(RuntimeError, match="not a multiple of group_size"):
        lsq_per_group(x, s, b, 48)
    with pytest.raises(RuntimeError, match="elements"):
        lsq_per_group(x, s[..., :1], b, 32)
    with pytest.raises(RuntimeError, match="double backwards"):
        xx, sg, bg = x.clone().requires_grad_(), s.clone().requires_grad_(), b.clone().requires_grad_()
        yy = torch.ops.torchlsq.lsq_forward_per_group(xx, sg, bg, 32, 0, 15, 0, 15, True, 1.0, False, False, False)
        gg = torch.ones_like(yy, requires_grad=True)
        (gx,) = torch.autograd.grad(yy, xx, gg, create_graph=True)
        gx.sum().backward()


def test_module_construction_shapes_and_state_dict():
    from torchlsq.quantized import LSQFakeQuantizer
    from torch.ao.quantization.observer import PerChannelMinMaxObserver

    def make(**kw):
        args = dict(observer=PerChannelMinMaxObserver, otype="weight", dtype=torch.qint8, qscheme=torch.per_channel_symmetric,
                    quant_min=-8, quant_max=7)
        args.update(kw)
        return LSQFakeQuantizer(**args)
    with pytest.raises(ValueError, match="otype='weight'"):
        LSQFakeQuantizer(PerChannelMinMaxObserver, "activation", qscheme=torch.per_channel_affine, group_size=32)
    with pytest.raises(ValueError, match="learn_params"):
        make(group_size=32, learn_params=False)
    with pytest.raises(ValueError, match="per-channel"):
        make(qscheme=torch.per_tensor_symmetric, group_size=32)
    with pytest.raises(ValueError, match="positive"):
        make(group_size=0)
    q = make(group_size=32)
    with pytest.raises(ValueError, match="does not divide"):
        q(torch.randn(16, 3, 3, 3))                     # rows of 27
    torch.manual_seed(1)
    w = torch.randn(16, 8, 3, 3) * 0.1                   # rows of 72: groups of 24
    q = make(group_size=24)
    assert torch.equal(q(w), w)                          # the creating call passes through
    assert q.scale.shape == (16, 3) and q.shift.shape == (16, 3)
    mu, sd = w.reshape(-1, 24).mean(1), w.reshape(-1, 24).std(1)
    want = (torch.max((mu - 3 * sd).abs(), (mu + 3 * sd).abs()) / 2 ** 3).reshape(16, 3)
    assert torch.equal(q.scale.detach(), want)
    scale, zp = q.calculate_qparams()
    assert scale.shape == (16, 3) and zp.shape == (16, 3)
    y = q(w)
    assert y.shape == w.shape and not torch.equal(y, w)
    levels, s, zp = q.quantize(w)
    assert levels.dtype == torch.int8 and levels.shape == w.shape and s.shape == (16, 3) and zp.dtype == torch.int64
    deq = (levels.reshape(16, 3, 24).float() - zp.unsqueeze(-1).float()) * s.unsqueeze(-1)
    assert torch.equal(deq.reshape(w.shape), y)
    with torch.no_grad():
        q.scale.mul_(1.5)
    q2 = make(group_size=24)
    q2(w)
    q2.load_state_dict(q.state_dict())
    assert torch.equal(q2.scale, q.scale) and torch.equal(q2.shift, q.shift) and torch.equal(q2(w), q(w))
    # group_size=None is the per-channel quantizer as before
    qc = make()
    qc(w)
    assert qc.scale.shape == (16,) and qc.group_size is None
