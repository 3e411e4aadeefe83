"""CPU: the 8-bit-activation linear op on packed group-wise weights (include/lsq_hip_qlinear_a8.h, liblsq_hip_qlinear_a8.so,
torch.ops.torchlsq.lsq_linear_packed_q8 / lsq_linear_packed_a8, torchlsq.quantized.PackedLinearA8 / convert_packed_a8)
without a GPU.

  * the library exports exactly what its header declares, ABI 1, imports nothing of the four other HIP libraries and reads
    no environment; its kernels are the two forms, integer MFMAs, no scratch, no atomics;
  * argument validation and the launch plan, host only;
  * CPU tensors: the bound and the exact-arithmetic tests of tests/qlinear_a8_cases.py, wide zero points, and the fused
    op == the levels op on lsq_levels_per_tensor's bytes;
  * the module surface: PackedLinearA8.from_packed / from_float, the state_dict round trip, convert_packed_a8.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import qlinear_a8_cases as A
import qlinear_cases as C
from helpers import gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_qlinear_a8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_qlinear_a8.so")
NAMES = sorted(["lsq_qlinear_a8_abi_version", "lsq_qlinear_a8_last_error", "lsq_qlinear_a8_forward_levels", "lsq_qlinear_a8_forward",
                "lsq_qlinear_a8_plan"])
_id = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))


def q8(lx, s_x, zx, p, bias, dtype):
    s, z = A.act(s_x, zx, lx.device)
    return torch.ops.torchlsq.lsq_linear_packed_q8(lx, s, z, p.codes, p.scale.reshape(-1), p.zero_point.reshape(-1), bias,
                                                   p.group_size, p.bits, dtype)


def test_a8_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_\w+)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_QLINEAR_A8) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_forward", "lsq_qlinear_plan"):
        assert other not in und and other not in nm, other
    assert "getenv" not in und and "debug" not in nm
    assert E.qlinear_a8_library().lsq_qlinear_a8_abi_version() == E.QLINEAR_A8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_QLINEAR_A8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    assert re.search(r"#define LSQ_QLINEAR_A8_MAX_ROWS (\d+)", open(HEADER).read()).group(1) == str(E.QLINEAR_A8_MAX_ROWS) == "16"
    assert not [n for n in list(E.C_ABI) + list(E.C_ABI_GROUP) + list(E.C_ABI_PACK) + list(E.C_ABI_CPU) + list(E.C_ABI_QLINEAR)
                if "a8" in n]


def test_a8_kernels(tmp_path):
    """per activation source (levels; bf16, fp16, fp32 x) and output type: the matrix-core form at 2 bits, at 4 bits with one
    and with two packets per MFMA, and the generic form at both widths; no scratch, no atomics, the code stream in 16-byte
    packets and integer MFMAs in the matrix-core form"""
    every = gfx950_kernels(LIB, str(tmp_path))
    assert all(re.search(r"qlinear_a8_(mfma|generic)_kernel", n) for n in every), sorted(every)
    assert len([n for n in every if "qlinear_a8_mfma_kernel" in n]) == 6 * 3
    assert len([n for n in every if "qlinear_a8_generic_kernel" in n]) == 6 * 2
    for name, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0 and not [o for o in ops if o.startswith("scratch_")], "%s uses %d bytes of scratch" % (name, scratch)
        assert not [o for o in ops if "atomic" in o], name
        if "qlinear_a8_mfma_kernel" in name:
            assert "global_load_dwordx4" in ops and "v_mfma_i32_16x16x64_i8" in ops, name
            assert not [o for o in ops if o.startswith("v_mfma_f32")], name
            assert "v_permlane32_swap_b32_e32" in ops and "v_permlane16_swap_b32_e32" in ops, name


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qlinear_a8_library()
    ok = 1 << 20

    def lv(ld=E.LSQ_A8_U8, x=ok, M=1, s=ok, z=ok, codes=ok, N=8, K=256, G=32, bits=4, qs=ok, qz=ok, bias=None, bd=E.LSQ_F32, y=ok,
           yd=E.LSQ_BF16):
        return lib.lsq_qlinear_a8_forward_levels(ld, x, M, s, z, codes, N, K, G, bits, qs, qz, bias, bd, y, yd, None)

    def fu(code=E.LSQ_BF16, x=ok, M=1, s=ok, b=ok, r=(0, 255, 0, 255), codes=ok, N=8, K=256, G=32, bits=4, qs=ok, qz=ok, bias=None,
           bd=E.LSQ_F32, y=ok):
        return lib.lsq_qlinear_a8_forward(code, x, M, s, b, r[0], r[1], r[2], r[3], codes, N, K, G, bits, qs, qz, bias, bd, y, None)

    def err():
        return lib.lsq_qlinear_a8_last_error()

    for f in (lv, fu):
        assert f(bits=3) == -1 and b"bits must be 4 or 2" in err()
        assert f(G=0) == -1 and b"group_size" in err()
        assert f(K=250) == -1 and b"multiple of group_size" in err()
        assert f(K=255, G=1) == -1 and b"one byte" in err()
        assert f(M=0) == -1 and b"rows of x" in err()
        assert f(M=17) == -1 and b"serves 1 to 16" in err()
        assert f(N=-1) == -1 and b"negative" in err()
        for null in ("x", "codes", "qs", "qz", "y", "s"):
            assert f(**{null: None}) == -1 and b"NULL" in err(), null
        assert f(qz=ok + 2) == -1 and b"element-aligned" in err()
        assert f(bias=ok, bd=E.LSQ_F16) == -1 and b"bias" in err()
        assert f(bias=ok + 2, bd=E.LSQ_F32) == -1 and b"element-aligned" in err()
        assert f(N=0) == 0                                                 # nothing to do, nothing launched
    assert lv(ld=2) == -1 and b"level_dtype" in err()
    assert lv(yd=E.LSQ_F64) == -1 and b"float64" in err()
    assert lv(yd=9) == -1 and b"dtype" in err()
    assert lv(z=None) == -1 and b"NULL" in err()
    assert lv(s=ok + 2) == -1 and b"element-aligned" in err()
    assert fu(code=E.LSQ_F64) == -1 and b"float64" in err()
    assert fu(x=ok + 1) == -1 and b"element-aligned" in err()
    assert fu(b=None) == -1 and b"NULL" in err()
    for r in ((-1, 255, 0, 255), (0, 256, 0, 256), (-128, 127, 0, 255), (5, 4, 0, 255), (-129, 127, -129, 127)):
        assert fu(r=r) == -1 and b"0..255 or within -128..127" in err(), r


def test_plan_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qlinear_a8_library()
    out = (ctypes.c_int32 * 8)()
    assert lib.lsq_qlinear_a8_plan(1, 64, 250, 32, 4, ctypes.byref(out)) == -1
    assert b"multiple of group_size" in lib.lsq_qlinear_a8_last_error()
    assert lib.lsq_qlinear_a8_plan(1, 64, 256, 32, 4, None) == -1 and b"NULL" in lib.lsq_qlinear_a8_last_error()
    assert lib.lsq_qlinear_a8_plan(17, 64, 256, 32, 4, ctypes.byref(out)) == -1
    # G a multiple of one 16-byte code packet (32 elements at 4 bits, 64 at 2) whose run of whole groups and whole load steps
    # fits one chunk of x: the matrix-core form, whatever the types of x and y
    for G, bits, form, chunk in ((32, 4, "mfma", 4096), (128, 4, "mfma", 4096), (96, 4, "mfma", 3840), (128, 2, "mfma", 4096),
                                 (64, 2, "mfma", 4096), (1024, 4, "mfma", 4096), (32, 2, "generic", 0), (8, 4, "generic", 0),
                                 (2, 4, "generic", 0), (8192, 4, "generic", 0)):
        for M in (1, 5, 16):
            K = {96: 4800, 8192: 8192}.get(G, 4096)
            pl = E.qlinear_a8_plan(M, 4096, K, G, bits)
            assert pl["form"] == form and pl["native_rows"] == 16 == E.QLINEAR_A8_MAX_ROWS and pl["chunk"] == chunk, (G, bits, pl)
            if form == "mfma":      # 256 tiles of 16 columns on (at least) 256 compute units; LDS grows with the rows of x
                assert pl["grid"] == 256 and pl["block"] == 1024 and pl["cols_per_tile"] == 16 and pl["waves_per_tile"] == 16
                assert pl["lds_bytes"] == 16384 + M * (chunk + 16) + M * (chunk // G) * 4 <= 160 * 1024
            else:
                assert pl["block"] == 256 and pl["grid"] == 1024 and pl["lds_bytes"] == 0
    assert E.qlinear_a8_plan(1, 17, 96, 32, 4)["grid"] == 2
    # every test shape's form
    forms = {s: E.qlinear_a8_plan(*s)["form"] for s in A.SHAPES}
    assert [forms[s] for s in A.SHAPES] == ["mfma", "mfma", "mfma", "generic", "generic", "mfma", "mfma", "mfma"]


@pytest.mark.parametrize("dtype", A.DTYPES, **_id)
@pytest.mark.parametrize("shape", A.SHAPES, **_id)
def test_cpu_path_meets_the_bound_and_is_exact(shape, dtype):
    M, N, K, G, bits = shape
    p = C.random_packed(N, K, G, bits, seed=M)
    for lo, hi, zx in ((0, 255, 3), (-128, 127, -7)):
        lx = A.levels((M, K), lo, hi, seed=N)
        for bias in (None, C.random_bias(N, torch.float32, seed=K), C.random_bias(N, dtype, seed=K)):
            r, E = A.reference(lx, 0.02, zx, p, bias)
            C.assert_within_bound(q8(lx, 0.02, zx, p, bias, dtype), r, E, dtype, "cpu %s levels %d..%d" % (shape, lo, hi))
    if K <= 4096:
        pe = C.exact_packed(N, K, G, bits, seed=M)
        # 0..255 with zx = 0 (lx - zx does not fit a byte), with zx = 131 (it does), and -128..127 with a negative zx
        for lo, hi, zx in ((0, 255, 0), (0, 255, 131), (-128, 127, -5)):
            lx = A.levels((M, K), lo, hi, seed=N)
            r, _ = A.reference(lx, A.S_X_EXACT, zx, pe)
            C.assert_exact(q8(lx, A.S_X_EXACT, zx, pe, None, dtype), r, dtype, "cpu exact %s zx %d" % (shape, zx))


@pytest.mark.parametrize("dtype", A.DTYPES, **_id)
def test_cpu_wide_zero_points(dtype):
    for p in (A.wide_packed(19, 256, 32, 4), A.wide_packed(7, 256, 64, 2), A.wide_packed(5, 48, 8, 4)):
        lx = A.levels((2, 3, p.shape[1]), 0, 255)
        r, E = A.reference(lx, 0.5, 128, p)
        y = q8(lx, 0.5, 128, p, None, dtype)
        assert y.shape == (2, 3, p.shape[0])
        C.assert_within_bound(y, r, E, dtype, "cpu zero points up to %d" % int(p.zero_point.max()))
    for pe in (A.wide_exact_packed(19, 256, 32, 4), A.wide_exact_packed(7, 256, 64, 2)):
        assert int(pe.zero_point.max()) == 1 << 23
        lx = A.levels((3, 256), 0, 255, seed=1)
        r, _ = A.reference(lx, A.S_X_EXACT, 0, pe)
        C.assert_exact(q8(lx, A.S_X_EXACT, 0, pe, None, dtype), r, dtype, "cpu exact, wide zero points")


QUANTIZERS = [(0.05, 0.0, -128, 127, -128, 127), (0.03, -1.7, 0, 255, 0, 255), (0.04, 0.6, 0, 127, 0, 255)]


@pytest.mark.parametrize("dtype", A.DTYPES, **_id)
@pytest.mark.parametrize("quant", QUANTIZERS, **_id)
def test_cpu_fused_form_is_the_levels_form(quant, dtype):
    from torchlsq.functional import lsq_linear_packed_a8
    scale, shift, qmin, qmax, tmin, tmax = quant
    p = C.random_packed(17, 96, 32, 4)
    x = A.special_x(3, 96, dtype, scale, shift, qmin, qmax)
    sc, sh = torch.tensor([scale]), torch.tensor([shift])
    bias = C.random_bias(17, torch.float32)
    y = lsq_linear_packed_a8(x, p, bias, sc, sh, qmin, qmax, tmin, tmax)
    lv = torch.ops.torchlsq.lsq_levels_per_tensor(x, sc, sh, qmin, qmax, tmin, tmax, 0)
    assert int(lv[0, 0]) == (qmin if qmin < 128 else qmin - 256)                   # the NaN went to quant_min
    lv = lv.view(torch.uint8) if tmax > 127 else lv
    zx = int(torch.tensor(-shift / scale).clamp(tmin, tmax).round())
    want = q8(lv, scale, zx, p, bias, dtype)
    assert y.dtype == dtype and torch.equal(y.view(C.INT[dtype]), want.view(C.INT[dtype]))
    assert torch.equal(y, p.linear_a8(x, bias, sc, sh, qmin, qmax, tmin, tmax))
    r, E = A.reference(lv, scale, zx, p, bias)
    C.assert_within_bound(y, r, E, dtype, "cpu fused")
    # a real quantized tensor as x
    if dtype == torch.float32:
        from torchlsq.functional import lsq_quantize
        xq = lsq_quantize(x, sc, sh, qmin, qmax, tmin, tmax, dtype=torch.quint8 if tmax > 127 else torch.qint8)
        assert torch.equal(lsq_linear_packed_a8(xq, p, bias, out_dtype=torch.float32), want)


def test_errors_on_the_cpu_and_empty_shapes():
    from torchlsq.functional import lsq_linear_packed_a8
    p = C.random_packed(8, 64, 32, 4)
    x = C.random_x((2, 64), torch.float32)
    sc, sh = torch.tensor([0.05]), torch.tensor([0.0])
    with pytest.raises(RuntimeError, match="K = 64"):
        lsq_linear_packed_a8(x[:, :32], p, None, sc, sh, 0, 255)
    with pytest.raises(RuntimeError, match="K = 64"):
        q8(A.levels((2, 32), 0, 255), 0.1, 0, p, None, torch.float32)
    with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
        lsq_linear_packed_a8(x.double(), p, None, sc.double(), sh.double(), 0, 255)
    with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
        q8(A.levels((2, 64), 0, 255), 0.1, 0, p, None, torch.float64)
    with pytest.raises(RuntimeError, match="uint8 .* or int8"):
        q8(A.levels((2, 64), 0, 255).to(torch.int32), 0.1, 0, p, None, torch.float32)
    with pytest.raises(RuntimeError, match="0..255 or within -128..127"):
        lsq_linear_packed_a8(x, p, None, sc, sh, -8, 255)
    with pytest.raises(RuntimeError, match="bias needs 8 values"):
        lsq_linear_packed_a8(x, p, torch.zeros(7), sc, sh, 0, 255)
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_linear_packed_a8(x.clone().requires_grad_(True), p, None, sc, sh, 0, 255)
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_linear_packed_a8(x, p, None, sc.clone().requires_grad_(True), sh, 0, 255)
    with torch.no_grad():
        assert lsq_linear_packed_a8(x.clone().requires_grad_(True), p, None, sc, sh, 0, 255).shape == (2, 8)
    assert lsq_linear_packed_a8(x[:0], p, None, sc, sh, 0, 255).shape == (0, 8)
    empty = type(p)(p.codes[:0], p.scale[:0], p.zero_point[:0], 4, 32, -8, (0, 64))
    assert lsq_linear_packed_a8(x, empty, None, sc, sh, 0, 255).shape == (2, 0)
    assert q8(A.levels((0, 64), 0, 255), 0.1, 0, p, None, torch.bfloat16).shape == (0, 8)


def test_fake_kernels_trace_shape_and_dtype():
    p = C.random_packed(8, 64, 32, 4)
    w = (p.codes, p.scale.reshape(-1), p.zero_point.reshape(-1), torch.zeros(8))

    def f(x, sc, sh, codes, scale, zp, bias):
        return torch.ops.torchlsq.lsq_linear_packed_a8(x, sc, sh, 0, 255, 0, 255, codes, scale, zp, bias, 32, 4) * 2

    def g(lx, s, z, codes, scale, zp, bias):
        return torch.ops.torchlsq.lsq_linear_packed_q8(lx, s, z, codes, scale, zp, bias, 32, 4, torch.float16) * 2

    x = C.random_x((2, 3, 64), torch.bfloat16)
    args = (x, torch.tensor([0.05]), torch.tensor([0.3])) + w
    out = torch.compile(f, backend="aot_eager", fullgraph=True)(*args)
    assert out.shape == (2, 3, 8) and out.dtype == torch.bfloat16 and torch.equal(out, f(*args))
    args = (A.levels((2, 3, 64), 0, 255),) + A.act(0.05, 3) + w
    out = torch.compile(g, backend="aot_eager", fullgraph=True)(*args)
    assert out.shape == (2, 3, 8) and out.dtype == torch.float16 and torch.equal(out, g(*args))


def _qat_model():
    """Linear(64, 32) -> ReLU -> Linear(32, 8): group-wise 4-bit weight quantizers, per-tensor activation quantizers (levels 0..127 in a 0..255 type)
    after the ReLU (layer 2's input) and, apart from the model, one for the model's input"""
    import torch.nn as nn
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver, MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    torch.manual_seed(3)
    model = nn.Sequential(nn.Linear(64, 32), nn.ReLU(), nn.Linear(32, 8, bias=False))
    weight = LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                        qscheme=torch.per_channel_symmetric, quant_min=-8, quant_max=7, group_size=32)
    act = LSQFakeQuantizer.with_args(observer=MovingAverageMinMaxObserver, otype="activation", dtype=torch.quint8,
                                     qscheme=torch.per_tensor_affine, quant_min=0, quant_max=127)
    model.qconfig = QConfig(activation=nn.Identity, weight=weight)
    model.train()
    prepare_qat(model, inplace=True)
    in_q, mid_q = act(), act()
    for _ in range(3):
        x = torch.randn(4, 64)
        model[2](mid_q(model[1](model[0](in_q(x)))))
    for q in (in_q, mid_q):             # trained: the observer no longer rewrites scale and shift on every call
        q.disable_observer()
    return model.eval(), in_q.eval(), mid_q.eval()


def test_packed_linear_a8_from_packed_from_float_and_state_dict():
    from torchlsq.quantized import LSQFakeQuantizer, PackedLinear, PackedLinearA8
    model, in_q, _ = _qat_model()
    p = C.random_packed(8, 64, 32, 4)
    bias = C.random_bias(8, torch.float32)
    x = C.random_x((3, 64), torch.float32)
    m = PackedLinearA8.from_packed(p, bias, in_q)
    assert isinstance(m, PackedLinear)
    assert sorted(k for k, _ in m.named_buffers()) == ["codes", "input_scale", "input_shift", "scale", "zero_point"]
    assert [k for k, _ in m.named_parameters()] == ["bias"]
    assert m.input_range == (0, 127, 0, 255) and torch.equal(m.input_scale, in_q.scale.detach().reshape(1))
    want = p.linear_a8(x, bias, in_q.scale.detach(), in_q.shift.detach(), 0, 127, 0, 255)
    assert torch.equal(m(x), want) and m.codes.data_ptr() != p.codes.data_ptr()
    assert torch.equal(m(in_q.quantize(x)), want)                           # a quantized tensor in: the levels form
    other = PackedLinearA8(64, 8, bits=4, group_size=32, quant_min=0, bias=True, input_range=(-128, 127, -128, 127))
    assert not torch.equal(other(x), m(x))
    other.load_state_dict(m.state_dict())
    assert other.quant_min == -8 and other.input_range == (0, 127, 0, 255) and torch.equal(other(x), m(x))
    assert sorted(k for k in m.state_dict() if not k.endswith("_extra_state")) == ["bias", "codes", "input_scale", "input_shift",
                                                                                   "scale", "zero_point"]
    layer = model[0]
    f = PackedLinearA8.from_float(layer, in_q)
    wq = layer.weight_fake_quant.export_packed(layer.weight)
    assert torch.equal(f.codes, wq.codes) and torch.equal(f.scale, wq.scale) and torch.equal(f.bias, layer.bias)
    assert (f.bits, f.group_size, f.quant_min, f.in_features, f.out_features) == (4, 32, -8, 64, 32)
    with pytest.raises(ValueError, match="group-wise"):
        PackedLinearA8.from_float(torch.nn.Linear(4, 4), in_q)
    with pytest.raises(ValueError, match="per-tensor"):
        PackedLinearA8.from_float(layer, layer.weight_fake_quant)            # a group-wise quantizer
    from torch.ao.quantization.observer import MovingAveragePerChannelMinMaxObserver
    pc = LSQFakeQuantizer(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                          qscheme=torch.per_channel_symmetric, quant_min=-64, quant_max=63)
    pc(torch.randn(8, 64))
    with pytest.raises(ValueError, match="per-tensor"):
        PackedLinearA8.from_packed(p, bias, pc)                               # a per-channel quantizer
    with pytest.raises(ValueError, match="LSQFakeQuantizer"):
        PackedLinearA8.from_packed(p, bias, None)


def test_convert_packed_a8_on_a_two_layer_model():
    import torch.nn as nn
    import torch.nn.functional as F
    from torchlsq.quantized import PackedLinear, PackedLinearA8, convert_packed_a8
    model, in_q, mid_q = _qat_model()
    conv = convert_packed_a8(model, {"0": in_q, "2": mid_q})
    assert conv is not model and isinstance(model[0], nn.Linear) and not isinstance(model[0], PackedLinear)
    assert [type(m).__name__ for m in conv] == ["PackedLinearA8", "ReLU", "PackedLinearA8"]
    only = convert_packed_a8(model, {"2": mid_q})
    assert isinstance(only[0], nn.Linear) and not isinstance(only[0], PackedLinear) and isinstance(only[2], PackedLinearA8)
    for m in (conv[0], conv[2]):                    # no float weight is left in a converted module
        assert [k for k, _ in m.named_parameters()] in (["bias"], [])
        assert not [k for k, v in m.state_dict().items() if torch.is_tensor(v) and v.is_floating_point() and v.dim() == 2 and
                    v.shape == (m.out_features, m.in_features)]
        assert not [k for k in m.state_dict() if "weight" in k]
    x = torch.randn(5, 64)
    with torch.no_grad():
        h = x
        for i, q in ((0, in_q), (2, mid_q)):
            # The op against the exact int64 reference on the levels and constants behind input_quantizer(h), within the bound.
            # F.linear(input_quantizer(h), dequantize(float32)) in float64 is that reference up to ITS OWN roundings: both
            # of its operands were rounded to fp32 once per element, (level - zx) * s_x and (code - qzero) * qscale, so it
            # lies within 2 * 2^-24 * |x_q| @ |w|^T of r -- a sum over |terms|, which the E of the bound (a sum over |I|, after
            # the cancellation inside a group) does not cover.  Both are asserted; together they bound |y - F.linear(...)|.
            pk = conv[i].packed()
            xq = q.quantize(h)
            r, E = A.reference(xq.int_repr(), xq.q_scale(), xq.q_zero_point(), pk, model[i].bias)
            w64 = pk.dequantize(torch.float32).double()
            want = F.linear(q(h).double(), w64, None if model[i].bias is None else model[i].bias.double())
            own = 2 * 2.0 ** -24 * (q(h).double().abs() @ w64.abs().t())
            assert bool(((want - r).abs() <= own).all())
            y = conv[i](h)
            C.assert_within_bound(y, r, E, torch.float32, "converted layer %d" % i)
            C.assert_within_bound(y, want, E + own, torch.float32, "converted layer %d against F.linear" % i)
            h = torch.relu(y)
    with pytest.raises(ValueError, match="not a linear layer"):
        convert_packed_a8(model, {"1": in_q})
    same = convert_packed_a8(model, {"0": in_q}, inplace=True)
    assert same is model and isinstance(model[0], PackedLinearA8) and type(model[2]).__name__ != "PackedLinearA8"


def test_row_blocks_of_a_call_beyond_one_launch():
    """more than 16 rows are cut into launches of at most 16 that cover every row once, in order"""
    from torchlsq._qlinear_a8_host import _row_blocks
    assert _row_blocks(1) == [(0, 1)] and _row_blocks(16) == [(0, 16)] and _row_blocks(17) == [(0, 16), (16, 1)]
    assert _row_blocks(33) == [(0, 16), (16, 16), (32, 1)] and _row_blocks(0) == []
