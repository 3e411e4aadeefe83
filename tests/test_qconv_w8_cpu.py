"""CPU: the W8A8 conv2d op on channels-last 8-bit levels (include/lsq_hip_qconv_w8.h, liblsq_hip_qconv_w8.so,
torch.ops.torchlsq.lsq_conv2d_w8_q8 / lsq_conv2d_w8_a8, torchlsq.functional.lsq_conv2d_w8a8, torchlsq.quantized.Conv2dW8A8 /
convert_w8a8) without a GPU.

  * the library exports exactly what its header declares, ABI 1, imports nothing of the other HIP libraries and reads no
    environment; its kernels are gfx950, integer MFMAs fed by 16-byte loads and ds_read_b128 in the matrix-core form, at most 128
    VGPRs, no scratch, no atomics;
  * the launch plan and argument validation, host only: nothing is launched;
  * CPU tensors: the derived bound of tests/qconv_w8_cases.py, the exact-arithmetic case, an independent restatement of the
    integers (F.unfold), and the fused op == the levels op on lsq_levels_per_tensor's bytes, channels-last or not;
  * through torch's own quantized tensors; the module surface: Conv2dW8A8.from_quantized / from_float, the state_dict round
    trip, convert_w8a8 on convolutions and on a mixed model, and its refusals.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import qconv_w8_cases as V
import qlinear_cases as C
import qlinear_w8_cases as W
from helpers import LLVM, demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_qconv_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_qconv_w8.so")
NAMES = sorted(["lsq_qconv_w8_abi_version", "lsq_qconv_w8_last_error", "lsq_qconv_w8_forward_levels", "lsq_qconv_w8_forward",
                "lsq_qconv_w8_plan"])
LSQ_EINVAL = -1
CL = torch.channels_last


def q8(lx, s_x, zx, lw, s_w, zw, bias, stride, padding, dilation, dtype):
    s, z = W.act(s_x, zx, lx.device)
    return torch.ops.torchlsq.lsq_conv2d_w8_q8(lx, s, z, lw, s_w, zw, bias, list(stride), list(padding), list(dilation), dtype)


def f32(v):
    return torch.tensor(v, dtype=torch.float32).item()


def bits(t):
    return t.detach().cpu().contiguous().view(C.INT[t.dtype])


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_\w+)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_QCONV_W8) == NAMES and len(NAMES) == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_"):
        assert other not in und, other
    for other in ("lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qgemm_", "lsq_qlinear_", "debug"):
        assert other not in nm, other
    assert E.qconv_w8_library().lsq_qconv_w8_abi_version() == E.QCONV_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_QCONV_W8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    assert ctypes.sizeof(E.LsqQconvW8Geom) == 13 * 8
    fields = re.search(r"typedef struct lsq_qconv_w8_geom \{\s*int64_t ([^;]+);", open(HEADER).read()).group(1)
    assert [f.strip() for f in fields.split(",")] == [f[0] for f in E.LsqQconvW8Geom._fields_]


def test_kernels(tmp_path):
    """the tiled kernel in 2 / 4 / 8 sub-tiles wide and split over K, the generic kernel and the pre-pass of the fused form per
    type of x: gfx950, no scratch, no atomics; the matrix-core kernels: v_mfma_i32_16x16x64_i8 only, fed by global_load_dwordx4
    and ds_read_b128, at most 128 VGPRs (two workgroups per compute unit fit)"""
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    tiles, levels, single = set(), set(), set()
    for sym, dm in names.items():
        m = re.match(r"^void lsq::qconv_w8_tiles_kernel<(?:\(int\))?([248]), (?:\(bool\))?(true|false|0|1)>\(", dm)
        if m:
            tiles.add((int(m.group(1)), m.group(2) in ("true", "1")))
            continue
        m = re.match(r"^void lsq::qconv_w8_levels_kernel<lsq::io_(bf16|f16|f32)>\(", dm)
        if m:
            levels.add(m.group(1))
            continue
        m = re.match(r"^lsq::qconv_w8_(generic)_kernel\(", dm)
        assert m, "not a kernel of this library: %s" % dm
        single.add(m.group(1))
    assert tiles == {(s, k) for s in (2, 4, 8) for k in (False, True)}
    assert levels == {"bf16", "f16", "f32"} and single == {"generic"}
    notes = ""
    for f in sorted(os.listdir(str(tmp_path))):
        if f.endswith(".co"):
            notes += subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(str(tmp_path), f)],
                                    capture_output=True, text=True, check=True).stdout
    vgprs = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        vgprs[re.search(r"\.name:\s+(\S+)", blk).group(1)] = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
    for sym, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0 and not [o for o in ops if o.startswith("scratch_")], "%s uses %d bytes of scratch" % (sym, scratch)
        assert not [o for o in ops if "atomic" in o], sym
        mfma = [o for o in ops if o.startswith("v_mfma")]
        if "tiles_kernel" in names[sym]:
            assert mfma and all(o == "v_mfma_i32_16x16x64_i8" for o in mfma), sym
            assert "global_load_dwordx4" in ops and "ds_read_b128" in ops, sym
            assert 0 < vgprs[sym] <= 128, (sym, vgprs[sym])
        else:
            assert not mfma, sym


def test_plan_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qconv_w8_library()
    out = (ctypes.c_int32 * 8)()
    g = E.LsqQconvW8Geom(2, 16, 5, 7, 17, 3, 3, 1, 1, 1, 1, 1, 1)
    assert lib.lsq_qconv_w8_plan(ctypes.byref(g), 1, None) == LSQ_EINVAL and b"NULL" in lib.lsq_qconv_w8_last_error()
    assert lib.lsq_qconv_w8_plan(None, 1, ctypes.byref(out)) == LSQ_EINVAL and b"NULL geometry" in lib.lsq_qconv_w8_last_error()
    plan = E.qconv_w8_plan
    # form by Cin % 16, K <= 65536 and alignment
    for Cin, k, aligned, form in ((16, 3, True, "mfma"), (32, 1, True, "mfma"), (48, (1, 3), True, "mfma"), (4096, 4, True, "mfma"),
                                  (65536, 1, True, "mfma"), (3, 7, True, "generic"), (24, 3, True, "generic"), (8, 2, True, "generic"),
                                  (65552, 1, True, "generic"), (4096, (4, 5), True, "generic"), (16, 3, False, "generic")):
        for B in (1, 40):
            pl = plan(B, Cin, 8, 8, 64, k, 1, 0, 1, aligned)
            assert pl["form"] == form and (pl["shape"] == "generic") == (form == "generic"), (Cin, k, aligned, pl)
    assert plan(1, 65536, 1, 2, 5, 1)["K"] == 65536 and plan(1, 65552, 1, 2, 5, 1)["K"] == 65552
    # SUBS by M (M <= 16 is a tile shape too), split-K exactly while row_tiles * ceil(N / 64) is below the 256 compute units
    # assumed without a device, the LDS formula
    for M in (1, 9, 16, 17, 32, 33, 64, 65, 128, 512, 2048, 40000):
        for N in (5, 64, 1000, 16321):
            subs = 2 if M <= 32 else 4 if M <= 64 else 8
            pl = plan(1, 16, 1, M, N, 1)
            assert (pl["M"], pl["N"], pl["K"]) == (M, N, 16)
            row_tiles = -(-M // (16 * subs))
            split = row_tiles * -(-N // 64) < 256
            assert pl["shape"] == ("tiles_split_k" if split else "tiles") and pl["rows_per_tile"] == 16 * subs and pl["block"] == 256
            assert pl["cols_per_tile"] == (16 if split else 64) and pl["k_split"] == (4 if split else 1)
            assert pl["grid"] == row_tiles * -(-N // pl["cols_per_tile"])
            assert pl["lds_bytes"] == 16 * subs * (256 + 16) + 16 * subs * 16 + 256 <= 64 * 1024
    assert V.plan_row_counts(lambda M: plan(1, 16, 1, M, 17, 3, 1, 1)) == [1, 15, 16, 17, 32, 33, 64, 65]
    pl = plan(2, 3, 9, 9, 5, 7, 2, 3)                                      # generic: (4 pixels, 1 channel) per wave, 4 waves
    assert pl["shape"] == "generic" and pl["block"] == 256 and pl["rows_per_tile"] == 4 and pl["cols_per_tile"] == 1
    assert pl["M"] == 2 * 5 * 5 and pl["grid"] == -(-(-(-50 // 4) * 5) // 4) and pl["lds_bytes"] == 0
    # the output's extent
    assert plan(1, 16, 9, 9, 16, 5, 1, 4, 2)["M"] == 81 and plan(3, 16, 4, 9, 67, 1, (2, 1), 0, 1)["M"] == 3 * 2 * 9


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qconv_w8_library()
    ok = 1 << 20
    base = dict(B=2, Cin=16, H=5, W=7, Cout=8, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)

    def geom(**kw):
        return E.LsqQconvW8Geom(**dict(base, **kw))

    def lv(ld=E.LSQ_W8_U8, x=ok, s=ok, z=ok, wd=E.LSQ_W8_I8, w=ok, ws=ok, wz=ok, bias=None, bd=E.LSQ_F32, y=ok, yd=E.LSQ_BF16, g=True,
           **kw):
        return lib.lsq_qconv_w8_forward_levels(ld, x, s, z, ctypes.byref(geom(**kw)) if g else None, wd, w, ws, wz, bias, bd, y, yd, None)

    def fu(code=E.LSQ_BF16, x=ok, s=ok, b=ok, r=(0, 255, 0, 255), wd=E.LSQ_W8_I8, w=ok, ws=ok, wz=ok, bias=None, bd=E.LSQ_F32, y=ok,
           lws=ok, g=True, **kw):
        return lib.lsq_qconv_w8_forward(code, x, s, b, r[0], r[1], r[2], r[3], ctypes.byref(geom(**kw)) if g else None, wd, w, ws, wz,
                                        bias, bd, y, lws, None)

    def err():
        return lib.lsq_qconv_w8_last_error()

    for f in (lv, fu):
        assert f(g=False) == LSQ_EINVAL and b"NULL geometry" in err()
        for name in ("B", "Cin", "H", "W"):
            assert f(**{name: 0}) == LSQ_EINVAL and b"at least 1" in err(), name
        assert f(Cout=-1) == LSQ_EINVAL and b"negative Cout" in err()
        for name in ("kh", "kw"):
            assert f(**{name: 0}) == LSQ_EINVAL and b"kernel" in err() and b"positive" in err(), name
        for name in ("sh", "sw"):
            assert f(**{name: 0}) == LSQ_EINVAL and b"stride" in err(), name
            assert f(**{name: -2}) == LSQ_EINVAL and b"stride" in err(), name
        for name in ("dh", "dw"):
            assert f(**{name: 0}) == LSQ_EINVAL and b"dilation" in err(), name
        for name in ("ph", "pw"):
            assert f(**{name: -1}) == LSQ_EINVAL and b"negative padding" in err(), name
        assert f(kh=8) == LSQ_EINVAL and b"empty output" in err()               # 8 > 5 + 2
        assert f(kw=4, dw=3) == LSQ_EINVAL and b"empty output" in err()         # 3 * 3 + 1 > 7 + 2
        assert f(H=1 << 31) == LSQ_EINVAL and b"31 bits" in err()
        assert f(ph=1 << 30, H=1 << 20) == LSQ_EINVAL and b"31 bits" in err()
        assert f(sw=1 << 31) == LSQ_EINVAL and b"31 bits" in err()
        assert f(B=1 << 62) == LSQ_EINVAL and b"64-bit offsets" in err()
        assert f(H=1 << 30, W=1 << 30, Cin=1 << 10) == LSQ_EINVAL and b"64-bit offsets" in err()
        assert f(B=1 << 20, H=1 << 10, W=1 << 10, Cout=1 << 20, kh=1, kw=1, ph=0, pw=0) == LSQ_EINVAL and b"31-bit grid" in err()
        assert f(wd=2) == LSQ_EINVAL and b"w_level_dtype" in err()
        for null in ("x", "w", "ws", "wz", "y", "s"):
            assert f(**{null: None}) == LSQ_EINVAL and b"NULL" in err(), null
        assert f(wz=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(ws=ok + 1) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(y=ok + 1) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(bias=ok, bd=E.LSQ_F16) == LSQ_EINVAL and b"bias" in err()
        assert f(bias=ok + 2, bd=E.LSQ_F32) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(Cout=0) == 0                                               # nothing to do, nothing launched
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
    from torchlsq.functional import lsq_conv2d_w8a8
    lw, s_w, zw = V.conv_weight(7, 16, (3, 3))
    lx = V.x_levels(2, 16, 5, 5, torch.uint8)
    s, z = W.act(0.05, 3)
    op = torch.ops.torchlsq.lsq_conv2d_w8_q8
    geo = ([1, 1], [1, 1], [1, 1], torch.float32)
    with pytest.raises(RuntimeError, match="uint8 .* or int8"):
        op(lx.to(torch.int32), s, z, lw, s_w, zw, None, *geo)
    with pytest.raises(RuntimeError, match=r"\[Cout, Cin, kh, kw\], got 2 dims"):
        op(lx, s, z, lw.reshape(7, -1), s_w, zw, None, *geo)                       # a wrong weight rank
    with pytest.raises(RuntimeError, match=r"\[B, Cin, H, W\], got 3 dims"):
        op(lx[0], s, z, lw, s_w, zw, None, *geo)
    with pytest.raises(RuntimeError, match="Cin = 16"):
        op(lx[:, :8], s, z, lw, s_w, zw, None, *geo)
    with pytest.raises(RuntimeError, match="w_scale must be 7 float32"):
        op(lx, s, z, lw, s_w.double(), zw, None, *geo)
    with pytest.raises(RuntimeError, match="w_zero must be 7 int32"):
        op(lx, s, z, lw, s_w, zw[:6], None, *geo)
    with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
        op(lx, s, z, lw, s_w, zw, None, [1, 1], [1, 1], [1, 1], torch.float64)
    with pytest.raises(RuntimeError, match="bias"):
        op(lx, s, z, lw, s_w, zw, torch.zeros(7, dtype=torch.float16), *geo)
    with pytest.raises(RuntimeError, match="stride must be positive"):
        op(lx, s, z, lw, s_w, zw, None, [0, 1], [1, 1], [1, 1], torch.float32)
    with pytest.raises(RuntimeError, match="padding must not be negative"):
        op(lx, s, z, lw, s_w, zw, None, [1, 1], [-1, 1], [1, 1], torch.float32)
    with pytest.raises(RuntimeError, match="empty output"):
        op(lx, s, z, lw, s_w, zw, None, [1, 1], [0, 0], [3, 3], torch.float32)
    fused = torch.ops.torchlsq.lsq_conv2d_w8_a8
    x = torch.randn(2, 16, 5, 5)
    sc, sh = torch.tensor([0.05]), torch.tensor([-3.0])
    with pytest.raises(RuntimeError, match="0..255 or within -128..127"):
        fused(x, sc, sh, -1, 255, 0, 255, lw, s_w, zw, None, [1, 1], [1, 1], [1, 1])
    with pytest.raises(RuntimeError, match="floating-point"):
        fused(lx, sc, sh, 0, 255, 0, 255, lw, s_w, zw, None, [1, 1], [1, 1], [1, 1])
    y = op(lx[:0], s, z, lw, s_w, zw, None, [2, 2], [1, 1], [1, 1], torch.float16)
    assert y.shape == (0, 7, 3, 3) and y.dtype == torch.float16
    # the functional's own checks
    wq = torch._make_per_channel_quantized_tensor(lw.contiguous(), s_w.double(), zw.long(), 0)
    xq = torch._make_per_tensor_quantized_tensor(lx.contiguous(), 0.05, 3)
    with pytest.raises(ValueError, match="groups == 1"):
        lsq_conv2d_w8a8(xq, wq, groups=2)
    with pytest.raises(AssertionError, match="4-D"):
        lsq_conv2d_w8a8(xq, torch._make_per_channel_quantized_tensor(lw.reshape(7, -1).contiguous(), s_w.double(), zw.long(), 0))
    w2 = torch._make_per_channel_quantized_tensor(lw[:, :, :2, :2].contiguous(), s_w.double(), zw.long(), 0)
    with pytest.raises(ValueError, match="asymmetric"):
        lsq_conv2d_w8a8(xq, w2, padding="same")                                 # a 2 x 2 kernel: one row more on one side
    with pytest.raises(ValueError, match="stride 1"):
        lsq_conv2d_w8a8(xq, wq, stride=2, padding="same")
    assert lsq_conv2d_w8a8(xq, wq, padding="same").shape == (2, 7, 5, 5)
    assert lsq_conv2d_w8a8(xq, wq, padding="same", dilation=2).shape == (2, 7, 5, 5)
    assert lsq_conv2d_w8a8(xq, wq, padding="valid").shape == (2, 7, 3, 3)
    assert torch.equal(lsq_conv2d_w8a8(xq, wq, padding=1), lsq_conv2d_w8a8(xq, wq, padding="same"))
    fake = torch.empty(2, 16, 5, 5, dtype=torch.uint8, device="meta")
    ym = op(fake, s.to("meta"), z.to("meta"), lw.to("meta"), s_w.to("meta"), zw.to("meta"), None, [2, 1], [1, 0], [1, 2], torch.bfloat16)
    assert ym.shape == (2, 7, 3, 1) and ym.dtype == torch.bfloat16 and ym.is_contiguous(memory_format=CL)


@pytest.mark.parametrize("geometry", V.GEOMETRIES + [(2, 3, 9, 9, 5, (7, 7), (2, 2), (3, 3), (1, 1)), (1, 24, 4, 4, 3, (3, 3), (1, 1), (1, 1), (1, 1))],
                         ids=V.geom_id)
def test_cpu_path_bound_restatement_and_layout(geometry):
    """the CPU path against the float64 reference within the derived bound; its integers against F.unfold + the linear's exact_I;
    a channels-last and an NCHW x (and weight) give the same bits; the output is channels-last and of the right shape"""
    B, Cin, H, Wd, N, k, s, p, d = geometry
    oh, ow = V.out_hw(H, Wd, k, s, p, d)
    for i, (x_dt, zx, w_dt, zeros, y_dt, bias_kind) in enumerate(V.VARIANTS):
        lw, s_w, zw = V.conv_weight(N, Cin, k, w_dt, B + Cin + i, zeros)
        bias = None if bias_kind is None else W.random_bias(N, torch.float32 if bias_kind == "f32" else y_dt, i)
        lx = V.x_levels(B, Cin, H, Wd, x_dt, seed=H + i)
        y = q8(lx, 0.0371, zx, lw, s_w, zw, bias, s, p, d, y_dt)
        assert y.shape == (B, N, oh, ow) and y.dtype == y_dt and y.is_contiguous(memory_format=CL)
        r, E = V.reference(lx, f32(0.0371), zx, lw, s_w, zw, bias, s, p, d)
        C.assert_within_bound(y, r, E, y_dt, "conv %s %s" % (V.geom_id(geometry), y_dt))
        I = V.exact_I(lx, zx, lw, zw, s, p, d)
        assert torch.equal(I, V.unfold_I(lx, zx, lw, zw, s, p, d))
        y2 = q8(lx.contiguous(), 0.0371, zx, lw.contiguous(), s_w, zw, bias, s, p, d, y_dt)          # NCHW operands
        assert not lx.contiguous().is_contiguous(memory_format=CL) or Cin == 1 or H * Wd == 1
        assert torch.equal(bits(y), bits(y2))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda v: str(v).replace("torch.", ""))
def test_cpu_levels_op_is_exact_for_power_of_two_scales_and_small_I(dtype):
    """levels within +-7 of the zero points over K = 9 * 16 = 144: |I| <= 144 * 49 < 2^13, scales 2^-6 and 2^-4, a bias that is a
    multiple of 2^-10 below 4: every fp32 step is exact, so y is the float64 result rounded once -- padding included"""
    N, Cin = 9, 16
    g = torch.Generator().manual_seed(1)
    lw = torch.randint(-7, 8, (N, Cin, 3, 3), generator=g).to(torch.int8)
    zw = torch.randint(-3, 4, (N,), generator=g).to(torch.int32)
    s_w = torch.full((N,), 2.0 ** -6)
    lx = torch.randint(112, 119, (2, Cin, 5, 4), generator=g).to(torch.uint8)
    bias = torch.randint(-4096, 4096, (N,), generator=g).float() * 2.0 ** -10
    for b in (None, bias):
        y = q8(lx, W.S_X_EXACT, 115, lw, s_w, zw, b, (1, 1), (2, 1), (1, 1), dtype)
        r, _ = V.reference(lx, W.S_X_EXACT, 115, lw, s_w, zw, b, (1, 1), (2, 1), (1, 1))
        C.assert_exact(y, r, dtype, "exact %s" % dtype)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("rng", [(0, 127, 0, 255), (0, 255, 0, 255), (-128, 127, -128, 127), (-64, 63, -128, 127)],
                         ids=lambda v: "x".join(map(str, v)))
def test_cpu_fused_op_equals_the_levels_op_on_the_levels_forward_bytes(rng, dtype):
    qmin, qmax, tmin, tmax = rng
    scale, shift = 0.05, -3.0 if tmin == 0 else 0.4
    B, Cin, H, Wd, N = 2, 16, 5, 3, 9
    lw, s_w, zw = V.conv_weight(N, Cin, (3, 3), torch.int8, 3, (-7, 127))
    bias = W.random_bias(N, dtype, 3)
    x = W.special_x(B * H * Wd, Cin, dtype, scale, shift, qmin, qmax).reshape(B, H, Wd, Cin).permute(0, 3, 1, 2)     # channels-last
    sc, sh = torch.tensor([scale]), torch.tensor([shift])
    geo = ([2, 1], [1, 2], [1, 1])
    y = torch.ops.torchlsq.lsq_conv2d_w8_a8(x, sc, sh, qmin, qmax, tmin, tmax, lw, s_w, zw, bias, *geo)
    lv = torch.ops.torchlsq.lsq_levels_per_tensor(x, sc, sh, qmin, qmax, tmin, tmax, 0)
    lv = lv.view(torch.uint8) if tmax > 127 else lv
    assert int(lv[0, 0, 0, 0]) == qmin                                          # the NaN went to quant_min
    s_x = sc.abs().clamp_min(torch.finfo(torch.float32).eps)
    zx = torch.fmin(torch.full_like(s_x, tmax), torch.fmax(torch.full_like(s_x, tmin), -sh * (1.0 / s_x))).round().to(torch.int32)
    want = torch.ops.torchlsq.lsq_conv2d_w8_q8(lv, s_x, zx, lw, s_w, zw, bias, *geo, dtype)
    assert y.dtype == dtype and y.shape == (B, N, 3, 5) and torch.equal(bits(y), bits(want))
    assert bool(torch.isfinite(y.float()).all()) and y.is_contiguous(memory_format=CL)
    y_nchw = torch.ops.torchlsq.lsq_conv2d_w8_a8(x.contiguous(), sc, sh, qmin, qmax, tmin, tmax, lw.contiguous(), s_w, zw, bias, *geo)
    assert torch.equal(bits(y), bits(y_nchw))


def _pow2_quantizers():
    """a per-tensor quint8 activation quantizer and a per-channel qint8 weight quantizer on a conv weight, run on one batch and
    then given power-of-two scales and shifts that are integer multiples of them: dequantize() of their tensors is exact"""
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver, MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    torch.manual_seed(5)
    m_x = LSQFakeQuantizer(observer=MovingAverageMinMaxObserver, otype="activation")
    m_w = LSQFakeQuantizer(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                           qscheme=torch.per_channel_symmetric)
    w = torch.randn(12, 16, 3, 3) * 0.1
    x = torch.randn(2, 16, 6, 5)
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


def test_through_torch_quantized_tensors_against_f_conv2d_on_the_dequantized_ones():
    """lsq_conv2d_w8a8(m_x.quantize(x), m_w.quantize(w), bias, ...) against float64 F.conv2d(xq.dequantize(), wq.dequantize(), bias)
    within the derived bound; power-of-two scales, so the dequantized tensors and every float64 product are exact"""
    from torchlsq.functional import lsq_conv2d_w8a8
    m_x, m_w, x, w = _pow2_quantizers()
    bias = torch.randn(12)
    xq, wq = m_x.quantize(x), m_w.quantize(w)
    assert xq.dtype == torch.quint8 and wq.dtype == torch.qint8 and wq.dim() == 4 and xq.q_zero_point() == 117
    assert len(wq.q_per_channel_zero_points().unique()) > 2
    for stride, padding, dilation in ((1, 1, 1), ((2, 1), (0, 2), (1, 2))):
        want = F.conv2d(xq.dequantize().double(), wq.dequantize().double(), bias.double(), stride, padding, dilation)
        s3, p3, d3 = ((v, v) if isinstance(v, int) else v for v in (stride, padding, dilation))
        I = V.exact_I(xq.int_repr(), 117, wq.int_repr(), wq.q_per_channel_zero_points(), s3, p3, d3)
        E = 9 * 2.0 ** -24 * (xq.q_scale() * wq.q_per_channel_scales().reshape(1, -1, 1, 1) * I.abs().double() + bias.double().abs().reshape(1, -1, 1, 1))
        for dtype in C.DTYPES:
            y = lsq_conv2d_w8a8(xq, wq, bias, stride, padding, dilation, out_dtype=dtype)
            C.assert_within_bound(y, want, E, dtype, "through quantized tensors, %s" % dtype)
        # the floating form with the quantizer's constants: the same bits as the quantized-tensor form
        y = lsq_conv2d_w8a8(x, wq, bias, stride, padding, dilation, scale=m_x.scale.detach(), shift=m_x.shift.detach(),
                            quant_min=m_x.quant_min, quant_max=m_x.quant_max, type_min=0, type_max=255)
        assert torch.equal(y, lsq_conv2d_w8a8(xq, wq, bias, stride, padding, dilation))
    wt = torch.quantize_per_tensor(w, 2.0 ** -9, 3, torch.qint8)                 # a per-tensor weight: its pair repeated
    want = F.conv2d(xq.dequantize().double(), wt.dequantize().double(), None, 1, 1)
    I = V.exact_I(xq.int_repr(), 117, wt.int_repr(), torch.full((12,), 3), (1, 1), (1, 1), (1, 1))
    C.assert_within_bound(lsq_conv2d_w8a8(xq, wt, padding=1), want, 9 * 2.0 ** -24 * xq.q_scale() * 2.0 ** -9 * I.abs().double(),
                          torch.float32, "per-tensor weight")
    with pytest.raises(AssertionError, match="axis 0"):
        lsq_conv2d_w8a8(xq, torch.quantize_per_channel(w, torch.ones(16), torch.zeros(16, dtype=torch.int64), 1, torch.qint8))


def test_an_x_that_requires_grad_raises():
    from torchlsq.functional import lsq_conv2d_w8a8
    m_x, m_w, x, w = _pow2_quantizers()
    wq = m_w.quantize(w)
    kw = dict(scale=m_x.scale.detach(), shift=m_x.shift.detach(), quant_min=0, quant_max=255)
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_conv2d_w8a8(x.clone().requires_grad_(True), wq, None, **kw)
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_conv2d_w8a8(x, wq, None, **dict(kw, scale=m_x.scale))
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_conv2d_w8a8(m_x.quantize(x), wq, torch.zeros(12, requires_grad=True))
    with torch.no_grad():
        assert lsq_conv2d_w8a8(x.clone().requires_grad_(True), wq, None, **dict(kw, scale=m_x.scale)).shape == (2, 12, 4, 3)


def test_conv2d_w8a8_from_quantized_from_float_and_state_dict():
    from torchlsq.functional import lsq_conv2d_w8a8
    from torchlsq.quantized import Conv2dW8A8
    model, in_q, _ = V.qat_conv_model()
    layer = model[0]
    wq = layer.weight_fake_quant.quantize(layer.weight.detach())
    x = torch.randn(3, 16, 7, 7)
    m = Conv2dW8A8.from_quantized(wq, layer.bias, in_q, padding=1)
    assert sorted(k for k, _ in m.named_buffers()) == ["input_scale", "input_shift", "weight_levels", "weight_scale", "weight_zero_point"]
    assert [k for k, _ in m.named_parameters()] == ["bias"]
    assert m.weight_levels.dtype == torch.int8 and m.weight_levels.shape == (8, 16, 3, 3) and m.weight_levels.is_contiguous(memory_format=CL)
    assert m.weight_scale.dtype == torch.float32 and m.weight_zero_point.dtype == torch.int32
    rng = (in_q.quant_min, in_q.quant_max, 0, 255)
    assert m.input_range == rng and (m.stride, m.padding, m.dilation, m.kernel_size) == ((1, 1), (1, 1), (1, 1), (3, 3))
    with torch.no_grad():
        want = lsq_conv2d_w8a8(x, wq, layer.bias, 1, 1, 1, scale=in_q.scale.detach(), shift=in_q.shift.detach(), quant_min=rng[0],
                               quant_max=rng[1], type_min=0, type_max=255)
        assert want.shape == (3, 8, 7, 7) and torch.equal(m(x), want) and torch.equal(m(in_q.quantize(x)), want)
        assert m(x).is_contiguous(memory_format=CL)
        other = Conv2dW8A8(16, 8, 3, stride=2, bias=True, weight_dtype=torch.uint8, input_range=(-128, 127, -128, 127))
        assert other(x).shape == (3, 8, 3, 3)
        other.load_state_dict(m.state_dict())
        assert other.input_range == rng and other.weight_levels.dtype == torch.int8 and other.stride == (1, 1) and other.padding == (1, 1)
        assert other.weight_levels.is_contiguous(memory_format=CL) and torch.equal(other(x), m(x))
        extra = m.state_dict()["_extra_state"]
        assert extra["stride"] == [1, 1] and extra["padding"] == [1, 1] and extra["dilation"] == [1, 1] and extra["weight_dtype"] == "int8"
        assert sorted(k for k in m.state_dict() if not k.endswith("_extra_state")) == [
            "bias", "input_scale", "input_shift", "weight_levels", "weight_scale", "weight_zero_point"]
        f = Conv2dW8A8.from_float(layer, in_q)
        assert torch.equal(f.weight_levels, wq.int_repr()) and torch.equal(f.bias, layer.bias) and torch.equal(f(x), want)
        assert torch.equal(f.weight_scale, wq.q_per_channel_scales().float()) and (f.in_channels, f.out_channels) == (16, 8)
    with pytest.raises(ValueError, match="per-tensor"):
        Conv2dW8A8.from_float(layer, layer.weight_fake_quant)                  # a per-channel input quantizer
    with pytest.raises(ValueError, match="LSQFakeQuantizer"):
        Conv2dW8A8.from_quantized(wq, None, None)
    with pytest.raises(ValueError, match="per-channel or per-tensor"):
        Conv2dW8A8.from_float(torch.nn.Conv2d(16, 4, 3), in_q)
    with pytest.raises(ValueError, match="groups == 1"):
        Conv2dW8A8.from_float(torch.nn.Conv2d(16, 4, 3, groups=2), in_q)


def test_convert_w8a8_on_convolutions_and_on_a_mixed_model():
    import torch.nn as nn
    from torch.ao.quantization import QConfig
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver, MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import Conv2dW8A8, LinearW8A8, LSQFakeQuantizer, convert_w8a8
    model, in_q, mid_q = V.qat_conv_model()
    conv = convert_w8a8(model, {"0": in_q, "2": mid_q})
    assert conv is not model and isinstance(model[0], nn.Conv2d)
    assert [type(m).__name__ for m in conv] == ["Conv2dW8A8", "ReLU", "Conv2dW8A8"]
    assert conv[2].stride == (2, 2) and conv[2].padding == (0, 0) and conv[2].bias is None
    only = convert_w8a8(model, {"2": mid_q})                                   # exactly the listed layers
    assert isinstance(only[0], nn.Conv2d) and isinstance(only[2], Conv2dW8A8)
    for m in (conv[0], conv[2]):                    # no float weight is left in a converted module
        assert [k for k, _ in m.named_parameters()] in (["bias"], [])
        assert not [k for k, v in m.state_dict().items() if torch.is_tensor(v) and v.is_floating_point() and v.dim() >= 2]
    x = torch.randn(5, 16, 7, 7)
    with torch.no_grad():
        h = x
        for i, q in ((0, in_q), (2, mid_q)):
            xq = q.quantize(h)
            wq = model[i].weight_fake_quant.quantize(model[i].weight.detach())
            r, E = V.reference(xq.int_repr(), f32(xq.q_scale()), xq.q_zero_point(), wq.int_repr(), wq.q_per_channel_scales().float(),
                               wq.q_per_channel_zero_points(), model[i].bias, model[i].stride, model[i].padding, model[i].dilation)
            y = conv[i](h)
            C.assert_within_bound(y, r, E, torch.float32, "converted layer %d" % i)
            h = torch.relu(y)
        assert h.shape == (5, 4, 3, 3)
    mixed, q0, q1, q2 = V.qat_conv_model(with_linear=True)
    both = convert_w8a8(mixed, {"0": q0, "2": q1, "4": q2})
    assert [type(m).__name__ for m in both] == ["Conv2dW8A8", "ReLU", "Conv2dW8A8", "Flatten", "LinearW8A8"]
    with torch.no_grad():
        y = both(x)
        lin = LinearW8A8.from_float(mixed[4], q2)
        assert y.shape == (5, 5) and torch.equal(y, lin(torch.flatten(both[2](both[1](both[0](x))), 1)))
    # refusals; the error for anything that is neither still says "not a linear layer"
    with pytest.raises(ValueError, match="not a linear layer"):
        convert_w8a8(model, {"1": in_q})                                       # a ReLU
    with pytest.raises(ValueError, match="per-tensor"):
        convert_w8a8(model, {"0": model[0].weight_fake_quant})                 # a per-channel input quantizer
    weight = LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                        qscheme=torch.per_channel_symmetric)
    grouped = nn.Conv2d(16, 8, 3, groups=2)
    grouped.weight_fake_quant = weight()
    grouped.weight_fake_quant(grouped.weight.detach())
    with pytest.raises(ValueError, match="not a linear layer or a 2-D convolution"):
        convert_w8a8(nn.Sequential(grouped), {"0": in_q})                      # groups = 2
    import torch.ao.nn.intrinsic.qat as nniqat
    fused = nniqat.ConvBn2d(16, 8, 3, qconfig=QConfig(activation=nn.Identity, weight=weight))
    fused.weight_fake_quant(fused.weight.detach())
    with pytest.raises(ValueError, match="fused ConvBn2d .* not a linear layer"):
        convert_w8a8(nn.Sequential(fused), {"0": in_q})
    with pytest.raises(ValueError, match="fused"):
        Conv2dW8A8.from_float(fused, in_q)
    fresh = nn.Conv2d(16, 8, 3)
    fresh.weight_fake_quant = weight()
    with pytest.raises(ValueError, match="not a linear layer"):
        convert_w8a8(nn.Sequential(fresh), {"0": in_q})                        # an untrained weight quantizer
    raw = LSQFakeQuantizer(observer=MovingAverageMinMaxObserver, otype="activation")
    with pytest.raises(ValueError, match="has not seen a batch"):
        convert_w8a8(model, {"0": raw})                                        # an untrained input quantizer
    same = convert_w8a8(model, {"0": in_q}, inplace=True)
    assert same is model and isinstance(model[0], Conv2dW8A8) and isinstance(model[2], nn.Conv2d)
