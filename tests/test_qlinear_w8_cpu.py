"""CPU: the W8A8 linear op on per-channel 8-bit weight levels (include/lsq_hip_qlinear_w8.h, liblsq_hip_qlinear_w8.so,
torch.ops.torchlsq.lsq_linear_w8_q8 / lsq_linear_w8_a8, torchlsq.functional.lsq_linear_w8a8, torchlsq.quantized.LinearW8A8 /
convert_w8a8) without a GPU.

  * the library exports exactly what its header declares, ABI 1, imports nothing of the other HIP libraries and reads no
    environment; its kernels are gfx950, integer MFMAs in the matrix-core form, no scratch, no atomics;
  * the launch plan and argument validation, host only: nothing is launched;
  * CPU tensors: the derived bound of tests/qlinear_w8_cases.py, the exact-arithmetic case, and the fused op == the levels
    op on lsq_levels_per_tensor's bytes;
  * through torch's own quantized tensors: lsq_linear_w8a8 against float64 F.linear on the dequantized tensors;
  * the module surface: LinearW8A8.from_quantized / from_float, the state_dict round trip, convert_w8a8.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import qlinear_cases as C
import qlinear_w8_cases as W
from helpers import demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_qlinear_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_qlinear_w8.so")
NAMES = sorted(["lsq_qlinear_w8_abi_version", "lsq_qlinear_w8_last_error", "lsq_qlinear_w8_forward_levels", "lsq_qlinear_w8_forward",
                "lsq_qlinear_w8_plan"])
LSQ_EINVAL = -1
_id = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))


def q8(lx, s_x, zx, lw, s_w, zw, bias, dtype):
    s, z = W.act(s_x, zx, lx.device)
    return torch.ops.torchlsq.lsq_linear_w8_q8(lx, s, z, lw, s_w, zw, bias, dtype)


def f32(v):
    return torch.tensor(v, dtype=torch.float32).item()


def test_w8_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_\w+)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_QLINEAR_W8) == NAMES and len(NAMES) == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_"):
        assert other not in und, other
    for other in ("lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qgemm_", "lsq_qlinear_a8", "lsq_qlinear_forward", "lsq_qlinear_plan", "debug"):
        assert other not in nm, other
    assert E.qlinear_w8_library().lsq_qlinear_w8_abi_version() == E.QLINEAR_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_QLINEAR_W8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    others = (list(E.C_ABI) + list(E.C_ABI_GROUP) + list(E.C_ABI_PACK) + list(E.C_ABI_CPU) + list(E.C_ABI_QLINEAR) +
              list(E.C_ABI_QLINEAR_A8) + list(E.C_ABI_QGEMM) + list(E.C_ABI_QGEMM_A8))
    assert not [n for n in others if "w8" in n]


def test_w8_kernels(tmp_path):
    """the decode kernel, the tiled kernel in 2 / 4 / 8 sub-tiles wide and split over K, the generic kernel and the pre-pass of
    the fused form per type of x: gfx950, no scratch, no atomics; integer MFMAs fed by 16-byte weight loads and ds_read_b128"""
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    tiles, levels, single = set(), set(), set()
    for sym, dm in names.items():
        m = re.match(r"^void lsq::qlinear_w8_tiles_kernel<(?:\(int\))?([248]), (?:\(bool\))?(true|false|0|1)>\(", dm)
        if m:
            tiles.add((int(m.group(1)), m.group(2) in ("true", "1")))
            continue
        m = re.match(r"^void lsq::qlinear_w8_levels_kernel<lsq::io_(bf16|f16|f32)>\(", dm)
        if m:
            levels.add(m.group(1))
            continue
        m = re.match(r"^lsq::qlinear_w8_(decode|generic)_kernel\(", dm)
        assert m, "not a kernel of this library: %s" % dm
        single.add(m.group(1))
    assert tiles == {(s, k) for s in (2, 4, 8) for k in (False, True)}
    assert levels == {"bf16", "f16", "f32"} and single == {"decode", "generic"}
    for sym, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0 and not [o for o in ops if o.startswith("scratch_")], "%s uses %d bytes of scratch" % (sym, scratch)
        assert not [o for o in ops if "atomic" in o], sym
        mfma = [o for o in ops if o.startswith("v_mfma")]
        if "tiles_kernel" in names[sym] or "decode_kernel" in names[sym]:
            assert mfma and all(o == "v_mfma_i32_16x16x64_i8" for o in mfma), sym
            assert "global_load_dwordx4" in ops and "ds_read_b128" in ops, sym
        else:
            assert not mfma, sym


def test_plan_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qlinear_w8_library()
    out = (ctypes.c_int32 * 8)()
    assert lib.lsq_qlinear_w8_plan(17, 64, 256, 1, None) == LSQ_EINVAL and b"NULL" in lib.lsq_qlinear_w8_last_error()
    assert lib.lsq_qlinear_w8_plan(0, 64, 256, 1, ctypes.byref(out)) == LSQ_EINVAL and b"rows of x" in lib.lsq_qlinear_w8_last_error()
    assert lib.lsq_qlinear_w8_plan(1, -1, 256, 1, ctypes.byref(out)) == LSQ_EINVAL
    # form 1 or 0 by K % 16, K > 65536 and alignment
    for K, aligned, form in ((64, True, "mfma"), (80, True, "mfma"), (4160, True, "mfma"), (65536, True, "mfma"), (16, True, "mfma"),
                             (72, True, "generic"), (8, True, "generic"), (65552, True, "generic"), (131072, True, "generic"),
                             (64, False, "generic"), (4096, False, "generic")):
        for M in (1, 16, 17, 2048):
            pl = E.qlinear_w8_plan(M, 4096, K, aligned)
            assert pl["form"] == form and (pl["shape"] == "generic") == (form == "generic"), (K, aligned, M, pl)
    # the launch shapes (256 compute units are assumed without a device)
    for M in (1, 2, 15, 16):
        pl = E.qlinear_w8_plan(M, 4096, 4096)
        assert pl["shape"] == "decode" and pl["grid"] == 256 and pl["block"] == 1024 and pl["k_split"] == 16 and pl["cols_per_tile"] == 16
        assert pl["lds_bytes"] == 16 * 256 * 4 + 2 * 16 * 16 * 4 + M * (4096 + 16)
    assert E.qlinear_w8_plan(1, 5, 64)["grid"] == 1 and E.qlinear_w8_plan(1, 11008, 4096)["grid"] == 256
    assert E.qlinear_w8_plan(3, 64, 80)["lds_bytes"] == 16 * 256 * 4 + 2 * 16 * 16 * 4 + 3 * (256 + 16)
    for M in (17, 32, 33, 64, 65, 128, 512, 2048):
        subs = 2 if M <= 32 else 4 if M <= 64 else 8
        pl = E.qlinear_w8_plan(M, 4096, 4096)
        row_tiles = -(-M // (16 * subs))
        split = row_tiles * 64 < 256
        assert pl["shape"] == ("tiles_split_k" if split else "tiles") and pl["rows_per_tile"] == 16 * subs and pl["block"] == 256
        assert pl["cols_per_tile"] == (16 if split else 64) and pl["k_split"] == (4 if split else 1)
        assert pl["grid"] == row_tiles * -(-4096 // pl["cols_per_tile"]) >= 256
        assert pl["lds_bytes"] == 16 * subs * (256 + 16) + 16 * subs * 16 + 256 <= 64 * 1024
    assert W.plan_row_thresholds(E.qlinear_w8_plan, 4096, 4096, upto=600) == [17, 33, 65, 385]


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qlinear_w8_library()
    ok = 1 << 20

    def lv(ld=E.LSQ_W8_U8, x=ok, M=17, s=ok, z=ok, wd=E.LSQ_W8_I8, w=ok, N=8, K=256, ws=ok, wz=ok, bias=None, bd=E.LSQ_F32, y=ok,
           yd=E.LSQ_BF16):
        return lib.lsq_qlinear_w8_forward_levels(ld, x, M, s, z, wd, w, N, K, ws, wz, bias, bd, y, yd, None)

    def fu(code=E.LSQ_BF16, x=ok, M=17, s=ok, b=ok, r=(0, 255, 0, 255), wd=E.LSQ_W8_I8, w=ok, N=8, K=256, ws=ok, wz=ok, bias=None,
           bd=E.LSQ_F32, y=ok, lws=ok):
        return lib.lsq_qlinear_w8_forward(code, x, M, s, b, r[0], r[1], r[2], r[3], wd, w, N, K, ws, wz, bias, bd, y, lws, None)

    def err():
        return lib.lsq_qlinear_w8_last_error()

    for f in (lv, fu):
        assert f(M=0) == LSQ_EINVAL and b"rows of x" in err()
        assert f(M=-3) == LSQ_EINVAL and b"rows of x" in err()
        assert f(M=1 << 62) == LSQ_EINVAL and b"64-bit offsets" in err()
        assert f(M=1 << 40, N=1 << 20) == LSQ_EINVAL and b"31-bit grid" in err()
        assert f(N=-1) == LSQ_EINVAL and b"negative" in err()
        assert f(K=-16) == LSQ_EINVAL and b"negative" in err()
        assert f(wd=2) == LSQ_EINVAL and b"w_level_dtype" in err()
        for null in ("x", "w", "ws", "wz", "y", "s"):
            assert f(**{null: None}) == LSQ_EINVAL and b"NULL" in err(), null
        assert f(wz=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(ws=ok + 1) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(y=ok + 1) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(bias=ok, bd=E.LSQ_F16) == LSQ_EINVAL and b"bias" in err()
        assert f(bias=ok + 2, bd=E.LSQ_F32) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(N=0) == 0                                                 # nothing to do, nothing launched
    assert lv(ld=2) == LSQ_EINVAL and b"level_dtype" in err()
    assert lv(yd=E.LSQ_F64) == LSQ_EINVAL and b"float64" in err()
    assert lv(yd=9) == LSQ_EINVAL and b"dtype" in err()
    assert lv(z=None) == LSQ_EINVAL and b"NULL" in err()
    assert lv(s=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
    assert lv(z=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
    assert fu(code=E.LSQ_F64) == LSQ_EINVAL and b"float64" in err()
    assert fu(x=ok + 1) == LSQ_EINVAL and b"element-aligned" in err()
    assert fu(b=None) == LSQ_EINVAL and b"NULL" in err()
    assert fu(b=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
    assert fu(lws=None) == LSQ_EINVAL and b"levels_ws" in err()
    assert fu(lws=ok + 8) == LSQ_EINVAL and b"levels_ws" in err()
    for r in ((-1, 255, 0, 255), (0, 256, 0, 256), (-128, 127, 0, 255), (5, 4, 0, 255), (-129, 127, -129, 127)):
        assert fu(r=r) == LSQ_EINVAL and b"0..255 or within -128..127" in err(), r


def test_host_checks_of_the_ops():
    lw, s_w, zw = W.weight(7, 32)
    lx = W.levels((3, 32), 0, 255)
    s, z = W.act(0.05, 3)
    op = torch.ops.torchlsq.lsq_linear_w8_q8
    with pytest.raises(RuntimeError, match="uint8 .* or int8"):
        op(lx.to(torch.int32), s, z, lw, s_w, zw, None, torch.float32)
    with pytest.raises(RuntimeError, match="weight levels must be int8"):
        op(lx, s, z, lw.to(torch.int16), s_w, zw, None, torch.float32)
    with pytest.raises(RuntimeError, match="w_scale must be 7 float32"):
        op(lx, s, z, lw, s_w.double(), zw, None, torch.float32)
    with pytest.raises(RuntimeError, match="w_zero must be 7 int32"):
        op(lx, s, z, lw, s_w, zw[:6], None, torch.float32)
    with pytest.raises(RuntimeError, match="K = 32"):
        op(lx[:, :31], s, z, lw, s_w, zw, None, torch.float32)
    with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
        op(lx, s, z, lw, s_w, zw, None, torch.float64)
    with pytest.raises(RuntimeError, match="bias"):
        op(lx, s, z, lw, s_w, zw, torch.zeros(7, dtype=torch.float16), torch.float32)
    with pytest.raises(RuntimeError, match="one float32 value"):
        op(lx, torch.ones(2), z, lw, s_w, zw, None, torch.float32)
    fused = torch.ops.torchlsq.lsq_linear_w8_a8
    x = torch.randn(3, 32)
    sc, sh = torch.tensor([0.05]), torch.tensor([-3.0])
    with pytest.raises(RuntimeError, match="0..255 or within -128..127"):
        fused(x, sc, sh, -1, 255, 0, 255, lw, s_w, zw, None)
    with pytest.raises(RuntimeError, match="floating-point"):
        fused(lx, sc, sh, 0, 255, 0, 255, lw, s_w, zw, None)
    assert op(lx[:0], s, z, lw, s_w, zw, None, torch.float16).shape == (0, 7)
    assert fused(x.reshape(3, 1, 32), sc, sh, 0, 255, 0, 255, lw, s_w, zw, None).shape == (3, 1, 7)


@pytest.mark.parametrize("dtype", C.DTYPES, **_id)
@pytest.mark.parametrize("shape", [(3, 5, 64), (17, 17, 80), (2, 67, 4160), (5, 9, 72), (1, 3, 1)], **_id)
def test_cpu_levels_op_is_within_the_derived_bound(shape, dtype):
    M, N, K = shape
    for x_dt, zx, w_dt, zeros, bias_dt in ((torch.uint8, 125, torch.int8, (-7, 127), torch.float32), (torch.int8, -128, torch.uint8, (0, 255), dtype),
                                           (torch.uint8, 3, torch.uint8, (131,), None)):
        lw, s_w, zw = W.weight(N, K, w_dt, M + K, zeros)
        bias = None if bias_dt is None else W.random_bias(N, bias_dt, K)
        lx = W.levels((M, K), *W.LEVEL_RANGE[x_dt], seed=K)
        y = q8(lx, 0.0371, zx, lw, s_w, zw, bias, dtype)
        r, E = W.reference(lx, f32(0.0371), zx, lw, s_w, zw, bias)
        C.assert_within_bound(y, r, E, dtype, "w8 %s %s" % (shape, dtype))
    lx3 = W.levels((2, 3, K), 0, 255, seed=1)                                  # leading dims
    lw, s_w, zw = W.weight(N, K)
    assert torch.equal(q8(lx3, 0.05, 7, lw, s_w, zw, None, dtype), q8(lx3.reshape(6, K), 0.05, 7, lw, s_w, zw, None, dtype).reshape(2, 3, N))


@pytest.mark.parametrize("dtype", C.DTYPES, **_id)
def test_cpu_levels_op_is_exact_for_power_of_two_scales_and_small_I(dtype):
    """levels within +-15 of the zero points over K = 48: |I| <= 48 * 15 * 15 < 2^14, scales 2^-6 and 2^-4, a bias that is a
    multiple of 2^-10 below 4: every fp32 step is exact, so y is the float64 result rounded once"""
    N, K = 9, 48
    lw = torch.randint(-15, 16, (N, K), generator=torch.Generator().manual_seed(1)).to(torch.int8)
    zw = torch.randint(-3, 4, (N,), generator=torch.Generator().manual_seed(2)).to(torch.int32)
    s_w = torch.full((N,), 2.0 ** -6)
    lx = torch.randint(100, 131, (5, K), generator=torch.Generator().manual_seed(3)).to(torch.uint8)
    bias = (torch.randint(-4096, 4096, (N,), generator=torch.Generator().manual_seed(4)).float() * 2.0 ** -10)
    for b in (None, bias):
        y = q8(lx, W.S_X_EXACT, 115, lw, s_w, zw, b, dtype)
        r, _ = W.reference(lx, W.S_X_EXACT, 115, lw, s_w, zw, b)
        C.assert_exact(y, r, dtype, "exact %s" % dtype)
    # the border of the 32-bit raw sum, still exact: I = -255 * 255 * 33040 < -2^31 at scales 2^-9 * 2^-7
    lw = torch.full((2, 33040), -128, dtype=torch.int8)
    lx = torch.full((1, 33040), 255, dtype=torch.uint8)
    y = q8(lx, 2.0 ** -7, 0, lw, torch.full((2,), 2.0 ** -9), torch.full((2,), 127, dtype=torch.int32), None, torch.float32)
    I = -255 * 255 * 33040
    assert I < -2 ** 31 and torch.equal(y, torch.full((1, 2), float(torch.tensor(I, dtype=torch.int64).float()) * 2.0 ** -16))


@pytest.mark.parametrize("dtype", C.DTYPES, **_id)
@pytest.mark.parametrize("rng", [(0, 127, 0, 255), (0, 255, 0, 255), (-128, 127, -128, 127), (-64, 63, -128, 127)], **_id)
def test_cpu_fused_op_equals_the_levels_op_on_the_levels_forward_bytes(rng, dtype):
    qmin, qmax, tmin, tmax = rng
    scale, shift = 0.05, -3.0 if tmin == 0 else 0.4
    N, K = 9, 80
    lw, s_w, zw = W.weight(N, K, torch.int8, 3, (-7, 127))
    bias = W.random_bias(N, dtype, 3)
    x = W.special_x(6, K, dtype, scale, shift, qmin, qmax)
    sc, sh = torch.tensor([scale]), torch.tensor([shift])
    y = torch.ops.torchlsq.lsq_linear_w8_a8(x, sc, sh, qmin, qmax, tmin, tmax, lw, s_w, zw, bias)
    lv = torch.ops.torchlsq.lsq_levels_per_tensor(x, sc, sh, qmin, qmax, tmin, tmax, 0)
    lv = lv.view(torch.uint8) if tmax > 127 else lv
    assert int(lv.view(torch.uint8 if tmax > 127 else torch.int8)[0, 0]) == qmin          # the NaN went to quant_min
    s_x = sc.abs().clamp_min(torch.finfo(torch.float32).eps)
    zx = torch.fmin(torch.full_like(s_x, tmax), torch.fmax(torch.full_like(s_x, tmin), -sh * (1.0 / s_x))).round().to(torch.int32)
    want = torch.ops.torchlsq.lsq_linear_w8_q8(lv, s_x, zx, lw, s_w, zw, bias, dtype)
    assert y.dtype == dtype and torch.equal(y.view(C.INT[dtype]), want.view(C.INT[dtype]))
    assert bool(torch.isfinite(y.float()).all())


def _pow2_quantizers():
    """a per-tensor quint8 activation quantizer and a per-channel qint8 weight quantizer, run on one batch and then given
    power-of-two scales and shifts that are integer multiples of them: dequantize() of their tensors, (level - zp) * s in
    fp32, is then exact, so float64 F.linear on the dequantized tensors carries no error of its own"""
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver, MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    torch.manual_seed(5)
    m_x = LSQFakeQuantizer(observer=MovingAverageMinMaxObserver, otype="activation")
    m_w = LSQFakeQuantizer(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                           qscheme=torch.per_channel_symmetric)
    w = torch.randn(12, 96) * 0.1
    x = torch.randn(7, 96)
    m_x(x)
    m_w(w)
    with torch.no_grad():
        m_x.scale.fill_(2.0 ** -6)
        m_x.shift.fill_(-117 * 2.0 ** -6)
        m_w.scale.copy_(torch.tensor([2.0 ** -(9 + i % 3) for i in range(12)]))
        m_w.shift.copy_(torch.tensor([float(i % 5 - 2) for i in range(12)]) * m_w.scale)
    m_x.disable_observer()
    m_w.disable_observer()
    return m_x.eval(), m_w.eval(), x, w


def test_through_torch_quantized_tensors_against_f_linear_on_the_dequantized_ones():
    """The independent check: lsq_linear_w8a8(m_x.quantize(x), m_w.quantize(w), bias) against float64
    F.linear(xq.dequantize(), wq.dequantize(), bias) within the derived bound.  The quantizers have power-of-two scales
    (_pow2_quantizers), so the dequantized tensors are exact; with arbitrary scales each element of them carries an fp32
    rounding of its own, a sum over |terms| that the bound on the op -- a sum after the cancellation in I -- does not cover."""
    import torch.nn.functional as F
    from torchlsq.functional import lsq_linear_w8a8
    m_x, m_w, x, w = _pow2_quantizers()
    bias = torch.randn(12)
    xq, wq = m_x.quantize(x), m_w.quantize(w)
    assert xq.dtype == torch.quint8 and wq.dtype == torch.qint8 and wq.qscheme() in (torch.per_channel_affine, torch.per_channel_symmetric)
    assert len(wq.q_per_channel_zero_points().unique()) > 2 and xq.q_zero_point() == 117
    lv = wq.int_repr().to(torch.int64) - wq.q_per_channel_zero_points().reshape(-1, 1)
    assert torch.equal(wq.dequantize().double(), lv.double() * wq.q_per_channel_scales().reshape(-1, 1))        # exact
    want = F.linear(xq.dequantize().double(), wq.dequantize().double(), bias.double())
    I = W.exact_I(xq.int_repr(), xq.q_zero_point(), wq.int_repr(), wq.q_per_channel_zero_points())
    E = 9 * 2.0 ** -24 * (xq.q_scale() * wq.q_per_channel_scales().reshape(1, -1) * I.abs().double() + bias.double().abs())
    for dtype in C.DTYPES:
        y = lsq_linear_w8a8(xq, wq, bias, out_dtype=dtype)
        C.assert_within_bound(y, want, E, dtype, "through quantized tensors, %s" % dtype)
    # the floating form with the quantizer's constants: the same bits as the quantized-tensor form
    y = lsq_linear_w8a8(x, wq, bias, m_x.scale.detach(), m_x.shift.detach(), m_x.quant_min, m_x.quant_max, 0, 255)
    assert torch.equal(y, lsq_linear_w8a8(xq, wq, bias))
    # a per-tensor weight quantizer: its one pair repeated N times
    wt = torch.quantize_per_tensor(w, 2.0 ** -9, 3, torch.qint8)
    want = F.linear(xq.dequantize().double(), wt.dequantize().double(), None)
    I = W.exact_I(xq.int_repr(), 117, wt.int_repr(), torch.full((12,), 3))
    C.assert_within_bound(lsq_linear_w8a8(xq, wt), want, 9 * 2.0 ** -24 * xq.q_scale() * 2.0 ** -9 * I.abs().double(), torch.float32, "per-tensor weight")
    with pytest.raises(AssertionError, match="axis 0"):
        lsq_linear_w8a8(xq, torch.quantize_per_channel(w, torch.ones(96), torch.zeros(96, dtype=torch.int64), 1, torch.qint8))


def test_an_x_that_requires_grad_raises():
    from torchlsq.functional import lsq_linear_w8a8
    m_x, m_w, x, w = _pow2_quantizers()
    wq = m_w.quantize(w)
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_linear_w8a8(xg, wq, None, m_x.scale.detach(), m_x.shift.detach(), 0, 255)
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_linear_w8a8(x, wq, None, m_x.scale, m_x.shift.detach(), 0, 255)          # the scale parameter wants a gradient
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_linear_w8a8(m_x.quantize(x), wq, torch.zeros(12, requires_grad=True))
    with torch.no_grad():
        assert lsq_linear_w8a8(xg, wq, None, m_x.scale, m_x.shift, 0, 255).shape == (7, 12)


def test_linear_w8a8_from_quantized_from_float_and_state_dict():
    from torchlsq.functional import lsq_linear_w8a8
    from torchlsq.quantized import LinearW8A8
    model, in_q, _ = W.qat_model()
    layer = model[0]
    wq = layer.weight_fake_quant.quantize(layer.weight.detach())
    x = torch.randn(3, 64)
    m = LinearW8A8.from_quantized(wq, layer.bias, in_q)
    assert sorted(k for k, _ in m.named_buffers()) == ["input_scale", "input_shift", "weight_levels", "weight_scale", "weight_zero_point"]
    assert [k for k, _ in m.named_parameters()] == ["bias"]
    assert m.weight_levels.dtype == torch.int8 and m.weight_scale.dtype == torch.float32 and m.weight_zero_point.dtype == torch.int32
    rng = (in_q.quant_min, in_q.quant_max, 0, 255)
    assert m.input_range == rng and rng[0] == 0 and torch.equal(m.input_scale, in_q.scale.detach().reshape(1))
    with torch.no_grad():
        want = lsq_linear_w8a8(x, wq, layer.bias, in_q.scale.detach(), in_q.shift.detach(), *rng)
        assert torch.equal(m(x), want) and torch.equal(m(in_q.quantize(x)), want)      # a quantized tensor in: the levels form
        other = LinearW8A8(64, 32, bias=True, weight_dtype=torch.uint8, input_range=(-128, 127, -128, 127))
        assert not torch.equal(other(x), m(x))
        other.load_state_dict(m.state_dict())
        assert other.input_range == rng and other.weight_levels.dtype == torch.int8 and torch.equal(other(x), m(x))
        assert sorted(k for k in m.state_dict() if not k.endswith("_extra_state")) == [
            "bias", "input_scale", "input_shift", "weight_levels", "weight_scale", "weight_zero_point"]
        f = LinearW8A8.from_float(layer, in_q)
        assert torch.equal(f.weight_levels, wq.int_repr()) and torch.equal(f.bias, layer.bias) and torch.equal(f(x), want)
        assert torch.equal(f.weight_scale, wq.q_per_channel_scales().float())
        assert (f.in_features, f.out_features) == (64, 32)
    with pytest.raises(ValueError, match="per-tensor"):
        LinearW8A8.from_float(layer, layer.weight_fake_quant)                  # a per-channel input quantizer
    with pytest.raises(ValueError, match="LSQFakeQuantizer"):
        LinearW8A8.from_quantized(wq, None, None)
    with pytest.raises(ValueError, match="per-channel or per-tensor"):
        LinearW8A8.from_float(torch.nn.Linear(4, 4), in_q)


def test_convert_w8a8_on_a_two_layer_model():
    import torch.nn as nn
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver, MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LinearW8A8, LSQFakeQuantizer, convert_w8a8
    model, in_q, mid_q = W.qat_model()
    conv = convert_w8a8(model, {"0": in_q, "2": mid_q})
    assert conv is not model and isinstance(model[0], nn.Linear)
    assert [type(m).__name__ for m in conv] == ["LinearW8A8", "ReLU", "LinearW8A8"]
    only = convert_w8a8(model, {"2": mid_q})                                   # exactly the listed layers
    assert isinstance(only[0], nn.Linear) and isinstance(only[2], LinearW8A8)
    for m in (conv[0], conv[2]):                    # no float weight is left in a converted module
        assert [k for k, _ in m.named_parameters()] in (["bias"], [])
        assert not [k for k, v in m.state_dict().items() if torch.is_tensor(v) and v.is_floating_point() and v.dim() == 2]
    x = torch.randn(5, 64)
    with torch.no_grad():
        h = x
        for i, q in ((0, in_q), (2, mid_q)):
            xq = q.quantize(h)
            wq = model[i].weight_fake_quant.quantize(model[i].weight.detach())
            r, E = W.reference(xq.int_repr(), f32(xq.q_scale()), xq.q_zero_point(), wq.int_repr(), wq.q_per_channel_scales().float(),
                               wq.q_per_channel_zero_points(), model[i].bias)
            y = conv[i](h)
            C.assert_within_bound(y, r, E, torch.float32, "converted layer %d" % i)
            h = torch.relu(y)
    with pytest.raises(ValueError, match="not a linear layer"):
        convert_w8a8(model, {"1": in_q})                                       # a ReLU
    with pytest.raises(ValueError, match="per-tensor"):
        convert_w8a8(model, {"0": model[0].weight_fake_quant})                 # a per-channel input quantizer
    grouped = nn.Linear(64, 8)
    grouped.weight_fake_quant = LSQFakeQuantizer(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                                 qscheme=torch.per_channel_symmetric, quant_min=-8, quant_max=7, group_size=32)
    grouped.weight_fake_quant(grouped.weight.detach())
    with pytest.raises(ValueError, match="not a linear layer"):
        convert_w8a8(nn.Sequential(grouped), {"0": in_q})                      # a group-wise layer
    fresh = nn.Linear(64, 8)
    fresh.weight_fake_quant = LSQFakeQuantizer(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                               qscheme=torch.per_channel_symmetric)
    with pytest.raises(ValueError, match="not a linear layer"):
        convert_w8a8(nn.Sequential(fresh), {"0": in_q})                        # an untrained weight quantizer
    raw = LSQFakeQuantizer(observer=MovingAverageMinMaxObserver, otype="activation")
    with pytest.raises(ValueError, match="has not seen a batch"):
        convert_w8a8(model, {"0": raw})                                        # an untrained input quantizer
    same = convert_w8a8(model, {"0": in_q}, inplace=True)
    assert same is model and isinstance(model[0], LinearW8A8) and isinstance(model[2], nn.Linear)
