"""CPU: the linear op on packed group-wise weights (include/lsq_hip_qlinear.h, liblsq_hip_qlinear.so,
torchlsq.functional.lsq_linear_packed, torchlsq.quantized.PackedLinear / convert_packed) without a GPU.

  * the library exports exactly what its header declares, ABI 1, imports nothing of the three other HIP libraries and reads
    no environment; its kernels are the two forms for every storage type and width;
  * argument validation and the launch plan, host only;
  * CPU tensors: the accuracy bound and the exact-arithmetic test of tests/qlinear_cases.py;
  * the module surface: PackedLinear.from_packed / from_float, the state_dict round trip, convert_packed.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import qlinear_cases as C
from helpers import gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_qlinear.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_qlinear.so")
NAMES = sorted(["lsq_qlinear_abi_version", "lsq_qlinear_last_error", "lsq_qlinear_forward", "lsq_qlinear_plan"])


def test_qlinear_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_\w+)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_QLINEAR) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    assert "lsq_hip_" not in nm and "lsq_group_" not in nm and "lsq_pack_" not in nm and "debug" not in nm
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und and "lsq_hip_" not in und and "lsq_group_" not in und and "lsq_pack_" not in und
    assert E.qlinear_library().lsq_qlinear_abi_version() == E.QLINEAR_ABI_VERSION == 1
    assert re.search(r"#define LSQ_QLINEAR_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    assert re.search(r"#define LSQ_QLINEAR_MAX_ROWS (\d+)", open(HEADER).read()).group(1) == str(E.QLINEAR_MAX_ROWS)
    assert not [n for n in list(E.C_ABI) + list(E.C_ABI_GROUP) + list(E.C_ABI_PACK) + list(E.C_ABI_CPU) if "qlinear" in n]


def test_qlinear_kernels(tmp_path):
    """the matrix-core form for the two 16-bit types, the generic form for all three, each at both widths; no scratch, the
    code stream in 16-byte packets, MFMAs and no atomics in the matrix-core form"""
    every = gfx950_kernels(LIB, str(tmp_path))
    assert all(re.search(r"qlinear_(mfma|generic)_kernel", n) for n in every), sorted(every)
    assert len([n for n in every if "qlinear_mfma_kernel" in n]) == 4
    assert len([n for n in every if "qlinear_generic_kernel" in n]) == 6
    for name, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0 and not [o for o in ops if o.startswith("scratch_")], "%s uses %d bytes of scratch" % (name, scratch)
        assert not [o for o in ops if "atomic" in o], name
        if "qlinear_mfma_kernel" in name:
            assert "global_load_dwordx4" in ops and [o for o in ops if o.startswith("v_mfma_f32_16x16x32")], name
            assert "v_permlane32_swap_b32_e32" in ops and "v_permlane16_swap_b32_e32" in ops, name


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qlinear_library()
    ok = 1 << 20

    def fwd(code=E.LSQ_BF16, x=ok, M=1, codes=ok, N=8, K=256, G=32, bits=4, qs=ok, qz=ok, bias=None, bd=E.LSQ_F32, y=ok):
        return lib.lsq_qlinear_forward(code, x, M, codes, N, K, G, bits, qs, qz, bias, bd, y, None)

    def err():
        return lib.lsq_qlinear_last_error()

    assert fwd(bits=3) == -1 and b"bits must be 4 or 2" in err()
    assert fwd(bits=8) == -1 and b"bits" in err()
    assert fwd(G=0) == -1 and b"group_size" in err()
    assert fwd(K=250) == -1 and b"multiple of group_size" in err()
    assert fwd(K=255, G=1) == -1 and b"one byte" in err()                 # G % (8 / bits) != 0
    assert fwd(K=258, G=2, bits=2) == -1 and b"one byte" in err()
    assert fwd(M=0) == -1 and b"rows of x" in err()
    assert fwd(M=-3) == -1 and b"rows of x" in err()
    assert fwd(M=17) == -1 and b"serves 1 to 16" in err()
    assert fwd(N=-1) == -1 and b"negative" in err()
    assert fwd(code=7) == -1 and b"dtype" in err()
    assert fwd(code=E.LSQ_F64) == -1 and b"float64" in err()
    for null in ("x", "codes", "qs", "qz", "y"):
        assert fwd(**{null: None}) == -1 and b"NULL" in err(), null
    assert fwd(x=ok + 1) == -1 and b"element-aligned" in err()
    assert fwd(qz=ok + 2) == -1 and b"element-aligned" in err()
    assert fwd(bias=ok, bd=E.LSQ_F16) == -1 and b"bias" in err()           # neither float32 nor x's type
    assert fwd(bias=ok + 2, bd=E.LSQ_F32) == -1 and b"element-aligned" in err()
    assert fwd(N=0) == 0                                                   # nothing to do, nothing launched


def test_plan_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qlinear_library()
    out = (ctypes.c_int32 * 8)()
    assert lib.lsq_qlinear_plan(E.LSQ_BF16, 1, 64, 250, 32, 4, ctypes.byref(out)) == -1
    assert b"multiple of group_size" in lib.lsq_qlinear_last_error()
    assert lib.lsq_qlinear_plan(E.LSQ_BF16, 1, 64, 256, 32, 4, None) == -1 and b"NULL" in lib.lsq_qlinear_last_error()
    assert lib.lsq_qlinear_plan(E.LSQ_BF16, 17, 64, 256, 32, 4, ctypes.byref(out)) == -1
    # 16-bit x and G a multiple of one 16-byte code packet (32 elements at 4 bits, 64 at 2): the matrix-core form
    for dtype, G, bits, form in ((torch.bfloat16, 32, 4, "mfma"), (torch.float16, 128, 4, "mfma"), (torch.float16, 96, 4, "mfma"),
                                 (torch.bfloat16, 128, 2, "mfma"), (torch.bfloat16, 32, 2, "generic"), (torch.float16, 8, 4, "generic"),
                                 (torch.bfloat16, 2, 4, "generic"), (torch.float32, 128, 4, "generic"), (torch.float32, 32, 2, "generic")):
        for M in (1, 5, 16):
            pl = E.qlinear_plan(dtype, M, 4096, 4096 if G != 96 else 4800, G, bits)
            assert pl["form"] == form and pl["native_rows"] == 16 == E.QLINEAR_MAX_ROWS, (dtype, G, bits, pl)
            if form == "mfma":      # 256 tiles of 16 columns on (at least) 256 compute units; LDS grows with the rows of x
                assert pl["grid"] == 256 and pl["block"] == 1024 and pl["cols_per_tile"] == 16 and pl["waves_per_tile"] == 16
                assert pl["chunk"] == 4096 and pl["lds_bytes"] == 16384 + M * (2 * 4096 + 16) <= 160 * 1024
            else:
                assert pl["block"] == 256 and pl["grid"] == 1024 and pl["lds_bytes"] == 0
    assert E.qlinear_plan(torch.bfloat16, 1, 17, 96, 32, 4)["grid"] == 2


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("shape", C.SHAPES + C.SHAPES_EXTRA, ids=lambda s: "x".join(map(str, s)))
def test_cpu_path_meets_the_bound_and_is_exact(shape, dtype):
    from torchlsq.functional import lsq_linear_packed
    M, N, K, G, bits = shape
    p = C.random_packed(N, K, G, bits, seed=M)
    x = C.random_x((M, K), dtype, seed=N)
    for bias in (None, C.random_bias(N, torch.float32, seed=K), C.random_bias(N, dtype, seed=K)):
        r, E = C.reference(x, p, bias)
        y = lsq_linear_packed(x, p, bias)
        C.assert_within_bound(y, r, E, dtype, "cpu %s bias %s" % (shape, None if bias is None else bias.dtype))
        assert torch.equal(y, p.linear(x, bias))
    if K <= 4096:
        pe, xe = C.exact_packed(N, K, G, bits, seed=M), C.exact_x((M, K), dtype, seed=N)
        r, _ = C.reference(xe, pe)
        C.assert_exact(lsq_linear_packed(xe, pe), r, dtype, "cpu exact %s" % (shape,))


def test_cpu_far_zero_points_affine_export_and_float64():
    from torchlsq.functional import lsq_linear_packed
    for p in (C.affine_packed(19, 256, 32), C.far_packed(19, 256, 32, 4), C.far_packed(7, 256, 64, 2)):
        for dtype in C.DTYPES:
            x = C.random_x((2, 3, 256), dtype)
            r, E = C.reference(x, p)
            y = lsq_linear_packed(x, p)
            assert y.shape == (2, 3, p.shape[0])
            C.assert_within_bound(y, r, E, dtype, "cpu zero points up to %d" % int(p.zero_point.max()))
    # a float64 scale computes in float64 on the CPU
    p = C.random_packed(9, 64, 32, 4)
    p64 = type(p)(p.codes, p.scale.double(), p.zero_point, p.bits, p.group_size, p.quant_min, p.shape)
    x = C.random_x((3, 64), torch.float64)
    y = lsq_linear_packed(x, p64)
    assert y.dtype == torch.float64 and torch.allclose(y, x @ p64.dequantize(torch.float64).t(), rtol=1e-13, atol=1e-13)


def test_errors_on_the_cpu():
    from torchlsq.functional import lsq_linear_packed
    p = C.random_packed(8, 64, 32, 4)
    x = C.random_x((2, 64), torch.float32)
    with pytest.raises(RuntimeError, match="K = 64"):
        lsq_linear_packed(C.random_x((2, 32), torch.float32), p)
    with pytest.raises(RuntimeError, match="bits must be 4 or 2"):
        torch.ops.torchlsq.lsq_linear_packed(x, p.codes, p.scale.reshape(-1), p.zero_point.reshape(-1), None, 32, 3)
    with pytest.raises(RuntimeError, match="bias needs 8 values"):
        lsq_linear_packed(x, p, torch.zeros(7))
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_linear_packed(x.clone().requires_grad_(True), p)
    with torch.no_grad():
        assert lsq_linear_packed(x.clone().requires_grad_(True), p).shape == (2, 8)
    assert not lsq_linear_packed(x, p).requires_grad


def test_fake_kernel_traces_shape_and_dtype():
    p = C.random_packed(8, 64, 32, 4)

    def f(x, codes, scale, zp, bias):
        return torch.ops.torchlsq.lsq_linear_packed(x, codes, scale, zp, bias, 32, 4) * 2

    x = C.random_x((2, 3, 64), torch.bfloat16)
    args = (x, p.codes, p.scale.reshape(-1), p.zero_point.reshape(-1), torch.zeros(8))
    out = torch.compile(f, backend="aot_eager", fullgraph=True)(*args)
    assert out.shape == (2, 3, 8) and out.dtype == torch.bfloat16 and torch.equal(out, f(*args))


def _qat_model(group_size=32):
    import torch.nn as nn
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    torch.manual_seed(3)
    model = nn.Sequential(nn.Linear(64, 32), nn.ReLU(), nn.Linear(32, 8, bias=False), nn.LayerNorm(8))
    model.qconfig = QConfig(
        activation=nn.Identity,
        weight=LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                          qscheme=torch.per_channel_symmetric, quant_min=-8, quant_max=7, group_size=group_size))
    model.train()
    prepare_qat(model, inplace=True)
    model(torch.randn(4, 64))
    model(torch.randn(4, 64))
    return model


def test_packed_linear_from_packed_from_float_and_state_dict():
    from torchlsq.quantized import PackedLinear
    p = C.random_packed(8, 64, 32, 4)
    bias = C.random_bias(8, torch.float32)
    x = C.random_x((3, 64), torch.float32)
    m = PackedLinear.from_packed(p, bias)
    assert sorted(k for k, _ in m.named_buffers()) == ["codes", "scale", "zero_point"]
    assert [k for k, _ in m.named_parameters()] == ["bias"]
    assert torch.equal(m(x), p.linear(x, bias)) and torch.equal(PackedLinear.from_packed(p)(x), p.linear(x))
    assert m.codes.data_ptr() != p.codes.data_ptr()
    # the state dict round-trips into a layer built with other settings of the same shapes
    other = PackedLinear(64, 8, bits=4, group_size=32, quant_min=0, bias=True)
    assert not torch.equal(other(x), m(x))
    other.load_state_dict(m.state_dict())
    assert other.quant_min == -8 and torch.equal(other(x), m(x))
    assert sorted(k for k in m.state_dict() if not k.endswith("_extra_state")) == ["bias", "codes", "scale", "zero_point"]
    # from_float: a QAT linear layer with a trained group-wise weight quantizer
    model = _qat_model().eval()
    layer = model[0]
    f = PackedLinear.from_float(layer)
    want = layer.weight_fake_quant.export_packed(layer.weight)
    assert torch.equal(f.codes, want.codes) and torch.equal(f.scale, want.scale) and torch.equal(f.bias, layer.bias)
    assert (f.bits, f.group_size, f.quant_min, f.in_features, f.out_features) == (4, 32, -8, 64, 32)
    with pytest.raises(ValueError, match="group-wise"):
        PackedLinear.from_float(torch.nn.Linear(4, 4))


def test_convert_packed_on_a_two_layer_model():
    import torch.nn as nn
    from torchlsq.quantized import PackedLinear, convert_packed
    model = _qat_model().eval()
    conv = convert_packed(model)
    assert conv is not model and isinstance(model[0], nn.Linear) and not isinstance(model[0], PackedLinear)
    assert [type(m).__name__ for m in conv] == ["PackedLinear", "ReLU", "PackedLinear", "LayerNorm"]
    assert conv[2].bias is None and torch.equal(conv[3].weight, model[3].weight)
    # no converted module keeps a floating-point weight, as a parameter or anywhere else in its state
    for m in (conv[0], conv[2]):
        assert [k for k, _ in m.named_parameters()] in (["bias"], [])
        assert not [k for k, v in m.state_dict().items() if torch.is_tensor(v) and v.is_floating_point() and v.dim() == 2 and
                    v.shape == (m.out_features, m.in_features)]
        assert not [k for k in m.state_dict() if "weight" in k]
    # each converted layer meets the bound against the QAT layer's eval output: the QAT weight is lsq_per_group(w), which
    # is dequantize() as numbers
    x = torch.randn(5, 64)
    with torch.no_grad():
        for i, inp in ((0, x), (2, torch.relu(model[0](x)))):
            layer = model[i]
            wq = layer.weight_fake_quant(layer.weight)
            assert torch.equal(wq, conv[i].packed().dequantize(torch.float32))
            r, E = C.reference(inp, conv[i].packed(), layer.bias)
            C.assert_within_bound(conv[i](inp), r, E, torch.float32, "converted layer %d" % i)
            C.assert_within_bound(layer(inp), r, E, torch.float32, "QAT layer %d" % i)
        assert torch.allclose(conv(x), model(x), rtol=1e-4, atol=1e-5)
    same = convert_packed(model, inplace=True)
    assert same is model and isinstance(model[0], PackedLinear)
    # a model without group-wise layers is left alone
    plain = nn.Sequential(nn.Linear(4, 4))
    assert type(convert_packed(plain)[0]) is nn.Linear
