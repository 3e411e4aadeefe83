"""CPU: the packed export of group-wise weights (include/lsq_hip_pack.h, liblsq_hip_pack.so,
torchlsq.functional.lsq_pack_per_group / LSQFakeQuantizer.export_packed) without a GPU.

  * the pack library exports exactly what its header declares, ABI 1, imports nothing of the two other HIP libraries and reads
    no environment;
  * its gfx950 code objects follow the device-code rules of the group library (tests/test_group_cpu.py);
  * argument validation and the launch plan, host only;
  * CPU tensors: the codes are the numpy packing of the oracle's levels, dequantize() is the CPU lsq_per_group forward bit
    for bit, levels() is lsq_levels_per_group, the constants are those LSQFakeQuantizer._quantize_groups derives;
  * the module surface: export_packed errors and bit selection, state() round trip, LSQWeightGroup.export_packed().

Inputs.  Codes cannot carry the sign of a zero: with quant_min < 0 a position in [-0.5, 0) rounds to the level -0.0, and the
forward's (-0.0 - zp) * s is -0.0 when zp is +0.0 where (code - zero_point) * scale is +0.0.  dequantize() is therefore
bit-identical to the forward iff quant_min >= 0 or no zero point is +0.0 (include/lsq_hip_pack.h), and the bit-exact
comparisons run on the bit-safe cases: affine ranges (0..15, 0..3 in a 0..255 type) with random shifts; symmetric ranges
(-8..7, -2..1) with shift +0.0 (zero point -0.0, what LSQFakeQuantizer gives these two ranges) and with shifts whose zero
point is a non-zero integer.  The corner itself is pinned down as it is -- equal values, bits differing only where the
forward is -0.0 -- by test_the_sign_of_a_zero_is_not_carried (the functional op) and
test_module_ranges_with_a_minus_zero_shift (LSQFakeQuantizer at -7..7 and -1..1, whose shift is -0.0).
"""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from helpers import assert_bits_equal, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_pack.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_pack.so")
NAMES = sorted(["lsq_pack_abi_version", "lsq_pack_last_error", "lsq_pack_quantize", "lsq_pack_dequantize", "lsq_pack_unpack",
                "lsq_pack_plan"])


def np_pack(codes, bits):
    """the format of include/lsq_hip_pack.h in numpy: flat codes -> bytes, element 0 in the low bits"""
    per = 8 // bits
    c = np.asarray(codes, dtype=np.uint8).reshape(-1, per)
    out = np.zeros(c.shape[0], dtype=np.uint8)
    for j in range(per):
        out |= (c[:, j] << (j * bits)).astype(np.uint8)
    return out


def test_pack_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_\w+)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_PACK) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    assert "lsq_hip_" not in nm and "lsq_group_" not in nm and "debug" not in nm
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und and "lsq_hip_" not in und and "lsq_group_" not in und
    assert E.pack_library().lsq_pack_abi_version() == E.PACK_ABI_VERSION == 1
    assert re.search(r"#define LSQ_PACK_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    # the other libraries' tables have no pack symbol
    assert not [n for n in list(E.C_ABI) + list(E.C_ABI_GROUP) + list(E.C_ABI_CPU) if "pack" in n]


@pytest.fixture(scope="module")
def pack_kernels(tmp_path_factory):
    every = gfx950_kernels(LIB, str(tmp_path_factory.mktemp("packcode")))
    assert all(re.search(r"pack_(quantize|dequantize|unpack)_kernel", n) for n in every), sorted(every)
    # 4 storage types x 2 widths x 2 forms each way, and the unpack kernels (2 widths x 2 forms)
    assert len([n for n in every if "pack_quantize_kernel" in n]) == 16
    assert len([n for n in every if "pack_dequantize_kernel" in n]) == 16
    assert len([n for n in every if "pack_unpack_kernel" in n]) == 4
    return every


def test_pack_kernels_follow_the_device_code_rules(pack_kernels):
    """no scratch, no v_fma_mix, contraction off (FMAs only inside the correctly rounded division), 16-byte packets on the
    wide side of the packet forms"""
    packets = 0
    for name, (body, scratch) in pack_kernels.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0 and not [o for o in ops if o.startswith("scratch_")], "%s uses %d bytes of scratch" % (name, scratch)
        assert not [o for o in ops if o.startswith("v_fma_mix") or o.startswith("v_mad_mix")], name
        n_fma = sum(1 for o in ops if re.fullmatch(r"v_(fma|fmac|mad|mac)_f(32|64)(_e32|_e64)?", o))
        n_div = sum(1 for o in ops if o.startswith("v_div_fmas_f"))
        assert n_fma <= 5 * n_div, "%s: %d FMAs for %d divisions" % (name, n_fma, n_div)
        # plain vector stores only: nothing goes through the scalar unit
        assert not [o for o in ops if re.match(r"s_(buffer_|scratch_)?(store|atomic)", o)], name
        if re.search(r"pack_quantize_kernelI.*Lb1EEEv", name):
            assert "global_load_dwordx4" in ops, name
            packets += 1
        if re.search(r"pack_dequantize_kernelI.*Lb1EEEv", name):
            assert "global_store_dwordx4" in ops, name
            packets += 1
        if re.search(r"pack_unpack_kernelILi\dELb1EEEv", name):
            assert "global_store_dwordx4" in ops, name
            packets += 1
    assert packets == 8 + 8 + 2


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.pack_library()
    p = E.LsqParams(-8, 7, -128, 127, 1, 1, 0, 0, 1.0, 0)
    ok = 1 << 20

    def quant(code=E.LSQ_F32, x=ok, n=256, G=32, sc=ok, sh=ok, pp=ctypes.byref(p), bits=4, codes=ok, qs=ok, qz=ok):
        return lib.lsq_pack_quantize(code, x, n, G, sc, sh, pp, bits, codes, qs, qz, None)

    def deq(code=E.LSQ_F32, codes=ok, n=256, G=32, bits=4, qs=ok, qz=ok, y=ok):
        return lib.lsq_pack_dequantize(code, codes, n, G, bits, qs, qz, y, None)

    def unpack(codes=ok, n=256, bits=4, qmin=-8, bias=0, levels=ok):
        return lib.lsq_pack_unpack(codes, n, bits, qmin, bias, levels, None)

    def err():
        return lib.lsq_pack_last_error()

    for call in (quant, deq):
        assert call(bits=3) == -1 and b"bits must be 4 or 2" in err()
        assert call(bits=8) == -1 and b"bits" in err()
        assert call(G=0) == -1 and b"group_size" in err()
        assert call(n=250) == -1 and b"multiple of group_size" in err()
        assert call(n=-32) == -1 and b"negative" in err()
        assert call(code=7) == -1 and b"dtype" in err()
        assert call(n=255, G=1) == -1 and b"byte boundary" in err()            # G % (8 / bits) != 0
        assert call(n=258, G=2, bits=2) == -1 and b"byte boundary" in err()
        assert call(codes=None) == -1 and b"NULL" in err()
        assert call(qs=None) == -1 and b"NULL" in err()
        assert call(qz=ok + 2) == -1 and b"element-aligned" in err()
        assert call(n=0) == 0                                                  # nothing to do is not an error (no launch)
    assert quant(x=None) == -1 and b"NULL" in err()
    assert quant(sc=None) == -1 and b"NULL" in err()
    assert quant(pp=None) == -1 and b"NULL" in err()
    assert quant(x=ok + 2) == -1 and b"element-aligned" in err()
    assert quant(code=E.LSQ_BF16, x=ok + 1) == -1 and b"element-aligned" in err()
    assert deq(y=None) == -1 and b"NULL" in err()
    assert deq(code=E.LSQ_F64, y=ok + 4) == -1 and b"element-aligned" in err()
    wide = E.LsqParams(-8, 8, -128, 127, 1, 1, 0, 0, 1.0, 0)
    assert quant(pp=ctypes.byref(wide)) == -1 and b"more than the 16 levels of 4-bit codes" in err()
    assert quant(bits=2) == -1 and b"more than the 4 levels of 2-bit codes" in err()
    bad = E.LsqParams(7, -8, -128, 127, 1, 1, 0, 0, 1.0, 0)
    assert quant(pp=ctypes.byref(bad)) == -1 and b"quant_min" in err()
    for huge in (E.LsqParams(-8, 7, -2 ** 23 - 1, 127, 1, 1, 0, 0, 1.0, 0), E.LsqParams(0, 15, 0, 2 ** 24, 1, 1, 0, 0, 1.0, 0),
                 E.LsqParams(2 ** 23 + 1, 2 ** 23 + 9, 0, 255, 1, 1, 0, 0, 1.0, 0)):
        assert quant(pp=ctypes.byref(huge)) == -1 and b"within +-2^23" in err()        # the integers must stay exact in fp32
    sharded = E.LsqParams(-8, 7, -128, 127, 1, 1, 0, 0, 1.0, 4096)
    assert quant(pp=ctypes.byref(sharded)) == -1 and b"numel_for_scaler must be 0" in err()
    assert unpack(bits=1) == -1 and b"bits must be 4 or 2" in err()
    assert unpack(n=255) == -1 and b"not a multiple of 2" in err()
    assert unpack(n=254, bits=2) == -1 and b"not a multiple of 4" in err()
    assert unpack(codes=None) == -1 and b"NULL" in err()
    assert unpack(levels=None) == -1 and b"NULL" in err()
    assert unpack(qmin=-200) == -1 and b"neither int8 nor uint8" in err()
    assert unpack(qmin=120, bias=-130) == -1 and b"neither int8 nor uint8" in err()
    assert unpack(n=0) == 0
    out = (ctypes.c_int32 * 8)()
    assert lib.lsq_pack_plan(E.LSQ_F32, 256, 32, 4, None) == -1 and b"NULL" in err()
    assert lib.lsq_pack_plan(E.LSQ_F32, 256, 32, 5, ctypes.byref(out)) == -1 and b"bits" in err()
    assert lib.lsq_pack_plan(E.LSQ_F32, 250, 32, 4, ctypes.byref(out)) == -1 and b"multiple of group_size" in err()


def test_plan_reports_the_forms():
    from torchlsq import extension as E
    for dtype, V in ((torch.float32, 4), (torch.float64, 2), (torch.bfloat16, 8), (torch.float16, 8)):
        for bits in (4, 2):
            lane = max(V, 8 // bits)
            for G in (8, 32, 128, 4096, 24 * V):
                p = E.pack_plan(dtype, G * 8192, G, bits)
                assert p["quantize_form"] == "packet" and p["dequantize_form"] == "packet" and p["block"] == 256, (dtype, bits, G, p)
                assert p["quantize_elems"] == lane and p["dequantize_elems"] == V
                for k in ("quantize_grid", "dequantize_grid", "unpack_grid"):
                    assert 1 <= p[k] <= 256 * 16, (k, p)
            G = 8 // bits                                   # the smallest group: a byte
            p = E.pack_plan(dtype, G * 7 * 1024, G, bits)
            assert p["quantize_form"] == ("packet" if G % lane == 0 else "byte")
            assert p["dequantize_form"] == ("packet" if G % V == 0 else "element")
    p = E.pack_plan(torch.float32, 12 * 1024, 12, 4)        # 12 % 4 == 0: packets; bf16: 12 % 8 != 0
    assert p["quantize_form"] == "packet"
    p = E.pack_plan(torch.bfloat16, 12 * 1024, 12, 4)
    assert p["quantize_form"] == "byte" and p["dequantize_form"] == "element"
    assert E.pack_plan(torch.float32, 0, 32, 4)["quantize_grid"] == 1
    with pytest.raises(RuntimeError, match="multiple of group_size"):
        E.pack_plan(torch.float32, 100, 32, 4)
    with pytest.raises(RuntimeError, match="byte boundary"):
        E.pack_plan(torch.float32, 99, 3, 4)


RANGES = {(4, "sym"): (-8, 7, -128, 127), (2, "sym"): (-2, 1, -128, 127), (4, "affine"): (0, 15, 0, 255), (2, "affine"): (0, 3, 0, 255)}
RANGES.update({(4, "sym_shift"): RANGES[(4, "sym")], (2, "sym_shift"): RANGES[(2, "sym")]})


def _case(dtype, G, rows, K, seed, scheme):
    rng = np.random.default_rng(seed)
    npd = {torch.float32: np.float32, torch.float64: np.float64}[dtype]
    x = (rng.standard_normal((rows, K)) * 0.3).astype(npd)
    x.reshape(-1)[::97] = 0.0
    x.reshape(-1)[5] = np.nan
    x.reshape(-1)[11] = np.inf
    x.reshape(-1)[K + 3] = -np.inf
    x.reshape(-1)[7] = -0.0
    ng = rows * K // G
    s = (rng.random(ng) * 0.05 + 0.01).astype(npd)
    s[::5] *= -1.0
    # the bit-safe shifts of the module docstring: +0.0; a zero point of 1 .. 5 in a range with quant_min < 0; a learned
    # shift around half an affine range
    if scheme == "sym":
        b = np.zeros(ng, dtype=npd)
    elif scheme == "sym_shift":
        b = (-rng.integers(1, 6, ng) * np.abs(s)).astype(npd)
    else:
        b = (-(rng.random(ng) * 6 + 1) * np.abs(s)).astype(npd)
    return x, s, b, ng


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("bits", [4, 2])
@pytest.mark.parametrize("G", ["byte", 8, 24, 96, 128])
@pytest.mark.parametrize("scheme", ["sym", "sym_shift", "affine"])
def test_cpu_pack_equals_the_oracle_and_round_trips(dtype, bits, G, scheme):
    from oracle import lsq_oracle as O
    from torchlsq.functional import lsq_levels_per_group, lsq_pack_per_group, lsq_per_group
    G = 8 // bits if G == "byte" else G
    rows, K = 5, G * 4 if G >= 24 else G * 48
    qmin, qmax, tmin, tmax = RANGES[(bits, scheme)]
    x, s, b, ng = _case(dtype, G, rows, K, G * 11 + bits, scheme)
    pshape = (rows, K // G)
    xt, st, bt = torch.from_numpy(x), torch.from_numpy(s).reshape(pshape), torch.from_numpy(b).reshape(pshape)
    packed = lsq_pack_per_group(xt, st, bt, G, bits, qmin, qmax, tmin, tmax)
    assert packed.codes.dtype == torch.uint8 and packed.codes.shape == (rows, K * bits // 8)
    assert packed.scale.shape == pshape and packed.zero_point.shape == pshape and packed.zero_point.dtype == torch.int32
    assert (packed.bits, packed.group_size, packed.quant_min, tuple(packed.shape)) == (bits, G, qmin, (rows, K))
    olv = O.levels_pc(x, s, b, 1, ng, G, qmin, qmax, tmin, tmax).reshape(-1).astype(np.int64)
    assert olv.min() >= qmin and olv.max() <= qmax and olv[5] == qmin                      # the NaN sits on quant_min
    assert np.array_equal(packed.codes.numpy().reshape(-1), np_pack(olv - qmin, bits))
    y = lsq_per_group(xt, st, bt, G, qmin, qmax, tmin, tmax, is_affine=(scheme == "affine"))
    assert_bits_equal(packed.dequantize(dtype).numpy(), y.numpy(), "dequantize() vs lsq_per_group")
    assert_bits_equal(y.numpy(), O.fwd_pc(x, s, b, 1, ng, G, qmin, qmax, tmin, tmax).reshape(rows, K), "lsq_per_group vs the oracle")
    for qd in (torch.qint8, torch.quint8):
        if qd == torch.quint8 and qmin < 0:
            continue
        assert torch.equal(packed.levels(qd), lsq_levels_per_group(xt, st, bt, G, qmin, qmax, tmin, tmax, dtype=qd))
    # the constants LSQFakeQuantizer._quantize_groups derives: s = max(|scale|, eps), zp = round(clamp(-shift * (1 / s)))
    sq = st.abs().clamp_min(torch.finfo(dtype).eps)
    zp = torch.fmin(torch.full_like(sq, tmax), torch.fmax(torch.full_like(sq, tmin), -bt * (1.0 / sq))).round()
    assert torch.equal(packed.scale, sq) and torch.equal(packed.zero_point.to(torch.int64), zp.to(torch.int64) - qmin)


def test_the_sign_of_a_zero_is_not_carried():
    """quant_min < 0 and a shift whose zero point rounds to +0.0: the forward's -0.0 (level -0.0 minus +0.0) comes back as
    +0.0; every other element keeps its bits"""
    from torchlsq.functional import lsq_pack_per_group, lsq_per_group
    x, s, b, ng = _case(torch.float32, 32, 8, 256, 3, "sym")
    b = (-0.2 * np.abs(s)).astype(np.float32)                # -shift / s = 0.2: zp = +0.0
    xt, st, bt = torch.from_numpy(x), torch.from_numpy(s), torch.from_numpy(b)
    y = lsq_per_group(xt, st, bt, 32, -8, 7, -128, 127)
    d = lsq_pack_per_group(xt, st, bt, 32, 4, -8, 7, -128, 127).dequantize(torch.float32)
    assert torch.equal(d, y)                                  # as numbers
    differ = d.view(torch.int32) != y.view(torch.int32)
    minus_zero = (y == 0) & torch.signbit(y)
    assert differ.any() and torch.equal(differ, minus_zero) and not torch.signbit(d[differ]).any()


def test_functional_checks_and_views():
    from torchlsq.functional import lsq_dequantize_per_group, lsq_pack_per_group, lsq_unpack_per_group
    torch.manual_seed(0)
    x = torch.randn(4, 3, 64)
    s = torch.rand(4, 3, 2) * 0.05 + 0.01
    b = torch.zeros(4, 3, 2)
    p = lsq_pack_per_group(x, s, b, 32, 4, -8, 7)
    assert p.codes.shape == (4, 3, 32) and p.scale.shape == (4, 3, 2) and tuple(p.shape) == (4, 3, 64)
    # a non-contiguous x is made contiguous; a scalar parameter is repeated once per group
    xt = x.transpose(0, 1).contiguous().transpose(0, 1)
    assert not xt.is_contiguous() and torch.equal(lsq_pack_per_group(xt, s, b, 32, 4, -8, 7).codes, p.codes)
    p1 = lsq_pack_per_group(x, torch.tensor([0.02]), torch.tensor([0.0]), 16, 2, -2, 1)
    assert p1.scale.shape == (x.numel() // 16,) and p1.codes.shape == (4, 3, 16)
    # codes at an odd byte offset
    buf = torch.zeros(p.codes.numel() + 3, dtype=torch.uint8)
    view = buf[1:1 + p.codes.numel()].view(p.codes.shape)
    view.copy_(p.codes)
    assert torch.equal(lsq_dequantize_per_group(view, p.scale, p.zero_point, 32, 4), p.dequantize())
    assert torch.equal(lsq_unpack_per_group(view, 4, -8), p.levels())
    assert p.dequantize(torch.bfloat16).dtype == torch.bfloat16
    assert torch.equal(p.dequantize(torch.bfloat16), p.dequantize(torch.float32).to(torch.bfloat16))
    # empty
    e = lsq_pack_per_group(torch.empty(0, 64), torch.empty(0, 2), torch.empty(0, 2), 32, 4, -8, 7)
    assert e.codes.shape == (0, 32) and e.dequantize().shape == (0, 64) and e.levels().shape == (0, 64)
    with pytest.raises(RuntimeError, match="bits must be 4 or 2"):
        lsq_pack_per_group(x, s, b, 32, 3, -4, 3)
    with pytest.raises(RuntimeError, match="more than the 4 levels of 2-bit codes"):
        lsq_pack_per_group(x, s, b, 32, 2, -8, 7)
    with pytest.raises(RuntimeError, match="byte boundary"):
        lsq_pack_per_group(torch.randn(4, 9), torch.rand(4, 3), torch.zeros(4, 3), 3, 4, -8, 7)
    with pytest.raises(RuntimeError, match="not a multiple of group_size"):
        lsq_pack_per_group(x, s, b, 48, 4, -8, 7)
    with pytest.raises(RuntimeError, match="elements"):
        lsq_pack_per_group(x, s[..., :1], b, 32, 4, -8, 7)
    with pytest.raises(RuntimeError, match="float64 scale dequantizes to float64"):
        p.dequantize(torch.float64)
    with pytest.raises(RuntimeError, match="need 24 elements"):
        lsq_dequantize_per_group(p.codes, p.scale.reshape(-1)[:5], p.zero_point.reshape(-1)[:5], 32, 4)


def test_torch_compile_fullgraph_of_dequantize_equals_eager():
    from torchlsq.functional import lsq_pack_per_group
    torch.manual_seed(1)
    x = torch.randn(16, 128)
    p = lsq_pack_per_group(x, torch.rand(16, 4) * 0.05 + 0.01, torch.zeros(16, 4), 32, 4, -8, 7)

    def f(codes, scale, zp):
        return torch.ops.torchlsq.lsq_dequantize_per_group(codes, scale, zp, 32, 4, torch.float32) * 0.5

    ref = f(p.codes, p.scale, p.zero_point)
    out = torch.compile(f, backend="inductor", fullgraph=True)(p.codes, p.scale, p.zero_point)
    assert torch.equal(out, ref) and torch.equal(ref, p.dequantize() * 0.5)


def _make(**kw):
    from torch.ao.quantization.observer import PerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    args = dict(observer=PerChannelMinMaxObserver, otype="weight", dtype=torch.qint8, qscheme=torch.per_channel_symmetric,
                quant_min=-8, quant_max=7)
    args.update(kw)
    return LSQFakeQuantizer(**args)


def test_module_export_packed():
    from torchlsq.functional import PackedGroupTensor
    torch.manual_seed(2)
    w = torch.randn(16, 8, 3, 3) * 0.1                   # rows of 72: groups of 24
    qc = _make()
    qc(w)
    with pytest.raises(ValueError, match="group-wise quantizers"):
        qc.export_packed(w)
    q8 = _make(group_size=24, quant_min=-128, quant_max=127, avoid_torch_overflow=False)      # an 8-bit range
    q8(w)
    with pytest.raises(ValueError, match=r"quantize\(\)"):
        q8.export_packed(w)
    q = _make(group_size=24)
    q(w)
    with pytest.raises(ValueError, match="does not fit 2-bit codes"):
        q.export_packed(w, bits=2)
    with pytest.raises(ValueError, match=r"quantize\(\)"):
        q.export_packed(w, bits=8)
    with torch.no_grad():
        q.scale.mul_(1.3)
        q.scale[::3] *= -1
    p = q.export_packed(w)
    assert p.bits == 4 and p.group_size == 24 and tuple(p.shape) == (16, 8, 3, 3) and p.codes.shape == (16, 36)
    y = q(w)
    assert_bits_equal(p.dequantize(w.dtype).numpy(), y.detach().numpy(), "export_packed().dequantize() vs the module")
    levels, s, zp = q.quantize(w)
    assert torch.equal(p.levels(torch.qint8), levels) and torch.equal(p.scale, s)
    assert torch.equal(p.zero_point.to(torch.int64), zp - q.quant_min)
    q2 = _make(group_size=24, quant_min=-2, quant_max=1)
    q2(w)
    p2 = q2.export_packed(w)
    assert p2.bits == 2 and p2.codes.shape == (16, 18)
    assert q2.export_packed(w, bits=4).bits == 4          # a wider container on request
    assert_bits_equal(p2.dequantize(w.dtype).numpy(), q2(w).detach().numpy(), "2-bit")
    # state() / from_state() through torch.save / torch.load
    f = io.BytesIO()
    torch.save(p.state(), f)
    f.seek(0)
    st = torch.load(f, weights_only=True)
    assert sorted(st) == ["bits", "codes", "group_size", "quant_min", "scale", "shape", "zero_point"]
    r = PackedGroupTensor.from_state(st)
    assert (r.bits, r.group_size, r.quant_min, tuple(r.shape)) == (4, 24, -8, (16, 8, 3, 3))
    assert torch.equal(r.codes, p.codes) and torch.equal(r.dequantize(), p.dequantize()) and torch.equal(r.levels(), p.levels())


@pytest.mark.parametrize("qrange", [(-7, 7), (-1, 1)], ids=["-7..7", "-1..1"])
def test_module_ranges_with_a_minus_zero_shift(qrange):
    """LSQFakeQuantizer gives a symmetric range with quant_min == -quant_max the shift -0.0, hence the zero point +0.0: the
    module's -0.0 (x / scale in [-0.5, 0)) comes back as +0.0.  Equal values; no other bit differs; levels and constants are
    the module's."""
    torch.manual_seed(4)
    w = torch.randn(16, 64) * 0.1
    q = _make(group_size=32, quant_min=qrange[0], quant_max=qrange[1])
    q(w)
    assert float(q.shift.flatten()[0]) == 0.0 and torch.signbit(q.shift).all()       # -0.0
    p = q.export_packed(w)
    assert p.bits == (4 if qrange[1] == 7 else 2)
    y = q(w).detach()
    d = p.dequantize(w.dtype)
    assert torch.equal(d, y)                                  # as numbers
    differ = d.view(torch.int32) != y.view(torch.int32)
    minus_zero = (y == 0) & torch.signbit(y)
    assert minus_zero.any() and torch.equal(differ, minus_zero) and not torch.signbit(d[differ]).any()
    levels, s, zp = q.quantize(w)
    assert torch.equal(p.levels(torch.qint8), levels) and torch.equal(p.scale, s)
    assert torch.equal(p.zero_point.to(torch.int64), zp - q.quant_min)


def test_weight_group_export_packed_on_a_two_layer_model():
    import torch.nn as nn
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver, MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer, LSQWeightGroup
    torch.manual_seed(3)
    model = nn.Sequential(nn.Linear(64, 32), nn.ReLU(), nn.Linear(32, 8))
    model.qconfig = QConfig(
        activation=LSQFakeQuantizer.with_args(observer=MovingAverageMinMaxObserver, otype="activation", init_batches=1),
        weight=LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                          qscheme=torch.per_channel_symmetric, quant_min=-8, quant_max=7, group_size=16))
    model.train()
    prepare_qat(model, inplace=True)
    group = LSQWeightGroup(model)
    model(torch.randn(4, 64))
    model(torch.randn(4, 64))
    out = group.export_packed()
    assert sorted(out) == ["0", "2"]
    for name, layer in (("0", model[0]), ("2", model[2])):
        p = out[name]
        assert p.bits == 4 and tuple(p.shape) == tuple(layer.weight.shape)
        assert p.codes.shape == (layer.weight.shape[0], layer.weight.shape[1] // 2)
        assert p.scale.shape == (layer.weight.shape[0], layer.weight.shape[1] // 16)
        y = layer.weight_fake_quant(layer.weight)
        assert_bits_equal(p.dequantize(torch.float32).numpy(), y.detach().numpy(), "layer " + name)
    group.remove()
