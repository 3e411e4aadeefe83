"""The W8A8 depthwise conv2d on 8-bit levels (include/lsq_hip_dwconv_w8.h), everything that needs no GPU: the library's exports
against its header and `_abi.py`, its kernel set and their resources, the plan on both sides of every threshold, every refusal, and
the CPU path of the ops -- the definition the GPU tests compare against -- held to the existing `lsq_conv2d_w8_q8` on the dense
embedding and to an independent numpy restatement, bit for bit, with the module and the converter on top.
"""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dwconv_w8_cases as D
import qlinear_w8_cases as W
import requant_w8_cases as R
from helpers import LLVM, demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_dwconv_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_dwconv_w8.so")
NAMES = sorted(["lsq_dwconv_w8_abi_version", "lsq_dwconv_w8_last_error", "lsq_dwconv_w8_forward_levels", "lsq_dwconv_w8_plan"])
LSQ_EINVAL = -1
CL = torch.channels_last
OPS = torch.ops.torchlsq


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    return [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(const void\*|int64_t)", "", decl.strip()).split(",") if f.strip()]


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_dwconv_w8_\w+)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_DWCONV_W8) == NAMES and len(NAMES) == 4
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_", "lsq_requant_", "lsq_resadd_",
                  "lsq_pool_", "lsq_dwconv_"):
        assert other not in und, other
    assert E.dwconv_w8_library().lsq_dwconv_w8_abi_version() == E.DWCONV_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_DWCONV_W8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    assert _fields(text, "lsq_dwconv_w8_out") == [f[0] for f in E.LsqDwconvW8Out._fields_] and ctypes.sizeof(E.LsqDwconvW8Out) == 8 * 8


def test_kernels(tmp_path):
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    short = {}
    for sym, dm in names.items():
        m = re.match(r"^(?:void )?lsq::dwconv_w8_(packets_dot|packets_loop|generic)_kernel(?:<([^>]*)>)?\(", dm)
        assert m, "not a kernel of this library: %s" % dm
        short[sym] = m.group(1) + "".join("_" + n for n in re.findall(r"\d+", re.sub(r"\(int\)", "", m.group(2) or "")))
    # packets_dot_<stride>: the unrolled 3 x 3 window through v_dot4_u32_u8, one pixel per lane
    assert sorted(short.values()) == ["generic", "packets_dot_1", "packets_dot_2", "packets_loop"]
    notes = ""
    for f in sorted(os.listdir(str(tmp_path))):
        if f.endswith(".co"):
            notes += subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(str(tmp_path), f)],
                                    capture_output=True, text=True, check=True).stdout
    vgprs, lds = {}, {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        sym = re.search(r"\.name:\s+(\S+)", blk).group(1)
        vgprs[sym] = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        lds[sym] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    for sym, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0, "%s uses %d bytes of scratch" % (sym, scratch)
        assert 0 < vgprs[sym] <= 128, (sym, vgprs[sym])
        assert lds[sym] == 0, (sym, lds[sym])
        if short[sym].startswith("packets"):
            assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops, sym
        if short[sym].startswith("packets_dot"):
            assert ops.count("v_dot4_u32_u8") >= 64 and "v_perm_b32" in ops, sym


def test_plan_without_a_gpu():
    from torchlsq import extension as E
    # packets if and only if C % 16 == 0 and x, w and y are aligned
    for C, aligned, y_aligned in itertools.product((3, 15, 16, 17, 20, 24, 32, 48), (True, False), (True, False)):
        pl = E.dwconv_w8_plan(2, C, 9, 7, 3, 1, 1, aligned=aligned, y_aligned=y_aligned)
        want = D.expected_plan(2, C, 9, 7, (3, 3), (1, 1), (1, 1), aligned, y_aligned)
        assert (pl["family"], pl["pixels_per_lane"], pl["grid"], pl["unrolled_window"], pl["unrolled_stride"]) == want, (C, aligned, y_aligned, pl)
        assert pl["family"] == ("packets" if aligned and y_aligned and C % 16 == 0 else "generic")
        assert (pl["OH"], pl["OW"], pl["block"]) == (9, 7, 256)
    assert E.dwconv_w8_plan(32, 144, 56, 56, 3, 1, 1) == dict(family="packets", grid=32 * 56 * 56 * 9 // 256, block=256, pixels_per_lane=1,
                                                              OH=56, OW=56, unrolled_window=3, unrolled_stride=1)
    # the unrolled windows: 3 x 3 without dilation at stride (1, 1) and (2, 2), nothing else (5 x 5 takes the loop)
    for k, s, d, want in ((3, 1, 1, (3, 1)), (3, 2, 1, (3, 2)), (3, 3, 1, (0, 0)), (3, (1, 2), 1, (0, 0)), (3, (2, 1), 1, (0, 0)),
                          (3, 1, 2, (0, 0)), (3, 1, (1, 2), (0, 0)), ((3, 2), 1, 1, (0, 0)), ((1, 3), 1, 1, (0, 0)), (5, 1, 1, (0, 0)),
                          (1, 1, 1, (0, 0)), (2, 1, 1, (0, 0)), (7, 2, 1, (0, 0))):
        pl = E.dwconv_w8_plan(2, 16, 20, 20, k, s, 0, d)
        assert (pl["unrolled_window"], pl["unrolled_stride"]) == want and pl["family"] == "packets" and pl["pixels_per_lane"] == 1, (k, s, d, pl)
    # output sizes: torch's rule
    for g in D.GEOMETRIES + [(1, 16, 12, 13, (3, 3), (2, 2), (1, 1), (1, 1)), (1, 16, 12, 13, (5, 5), (3, 2), (2, 1), (1, 2))]:
        B, C, H, Wd, k, s, p, d = g
        pl = E.dwconv_w8_plan(B, C, H, Wd, k, s, p, d)
        want = F.conv2d(torch.zeros(1, 1, H, Wd), torch.zeros(1, 1, *k), None, s, p, d).shape[2:]
        assert (pl["OH"], pl["OW"]) == tuple(want) == D.out_hw(g), g
        assert pl["grid"] == D.expected_plan(B, C, *want, k, s, d)[2]
    # pixels per lane: the library ships one pixel per lane at both strides, so the two-workgroups-per-compute-unit
    # rule never lowers it; the rule itself is the expected plan's, on both sides of 512 workgroups at 256 compute units
    for B in (1, 31, 32, 33, 512):
        pl = E.dwconv_w8_plan(B, 64, 34, 34, 3, 1, 1)
        assert (pl["family"], pl["pixels_per_lane"], pl["grid"], pl["unrolled_window"], pl["unrolled_stride"]) == \
            D.expected_plan(B, 64, 34, 34, (3, 3), (1, 1), (1, 1)), (B, pl)


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.dwconv_w8_library()
    err = lib.lsq_dwconv_w8_last_error
    G = E.LsqQconvW8Geom

    def geom(**kw):
        base = dict(B=2, Cin=16, H=9, W=7, Cout=16, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)
        base.update(kw)
        return G(*[base[f[0]] for f in G._fields_])
    out = (ctypes.c_int32 * 8)()
    plan = lib.lsq_dwconv_w8_plan
    assert plan(None, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"NULL geometry" in err()
    assert plan(ctypes.byref(geom()), 1, 1, None) == LSQ_EINVAL and b"NULL output" in err()
    for bad, msg in ((dict(B=0), b"at least 1"), (dict(Cin=0, Cout=0), b"at least 1"), (dict(H=0), b"at least 1"), (dict(W=-1), b"at least 1"),
                     (dict(Cout=32), b"channel multiplier"), (dict(Cout=8), b"channel multiplier"), (dict(Cout=0), b"channel multiplier"),
                     (dict(kh=0), b"kernel"), (dict(kw=-2), b"kernel"), (dict(sh=0), b"stride"), (dict(sw=0), b"stride"),
                     (dict(dh=0), b"dilation"), (dict(dw=-1), b"dilation"), (dict(ph=-1), b"negative padding"), (dict(pw=-1), b"negative padding"),
                     (dict(H=2, ph=0), b"empty output"), (dict(W=1, pw=0), b"empty output"), (dict(dh=6), b"empty output"),
                     (dict(H=1 << 31), b"beyond 31 bits"), (dict(sh=1 << 31), b"beyond 31 bits"), (dict(pw=1 << 31), b"beyond 31 bits"),
                     (dict(kh=65, kw=64, H=80, W=80), b"at most 4096"), (dict(kh=4097, kw=1, H=5000), b"at most 4096"),
                     (dict(B=1 << 40, H=1 << 20, W=1 << 20), b"64-bit")):
        assert plan(ctypes.byref(geom(**bad)), 1, 1, ctypes.byref(out)) == LSQ_EINVAL and msg in err(), (bad, err())
    assert plan(ctypes.byref(geom(kh=64, kw=64, H=80, W=80)), 1, 1, ctypes.byref(out)) == 0          # 4096 taps are served
    assert plan(ctypes.byref(geom(B=1 << 24, Cin=16, Cout=16, H=1 << 10, W=1 << 10)), 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"31-bit grid" in err()
    # the call: everything is refused before anything is enqueued (no GPU here: an accepted call would fail in the launch)
    x = torch.zeros(2 * 9 * 7 * 16 + 64, dtype=torch.uint8)
    y = torch.zeros(2 * 9 * 7 * 16 * 4 + 64, dtype=torch.uint8)
    w = torch.zeros(9 * 16, dtype=torch.int8)
    s_x, zx = torch.ones(3), torch.zeros(3, dtype=torch.int32)
    s_w, zw, bias = torch.ones(16), torch.zeros(16, dtype=torch.int32), torch.zeros(16)
    osc, osh = torch.ones(3), torch.zeros(3)

    def outq(**kw):
        base = dict(out_scale=osc.data_ptr(), out_shift=osh.data_ptr(), quant_min=0, quant_max=255, type_min=0, type_max=255, act=0,
                    mid_dtype=E.LSQ_F32)
        base.update(kw)
        return E.LsqDwconvW8Out(*[base[f[0]] for f in E.LsqDwconvW8Out._fields_])

    def call(o=None, **kw):
        a = dict(level_dtype=0, x=x.data_ptr(), s_x=s_x.data_ptr(), zx=zx.data_ptr(), g=geom(), w_level_dtype=1, w=w.data_ptr(),
                 s_w=s_w.data_ptr(), zw=zw.data_ptr(), bias=None, bias_dtype=0, o=outq() if o is None else o, y=y.data_ptr())
        a.update(kw)
        return lib.lsq_dwconv_w8_forward_levels(a["level_dtype"], a["x"], a["s_x"], a["zx"], None if a["g"] is None else ctypes.byref(a["g"]),
                                                a["w_level_dtype"], a["w"], a["s_w"], a["zw"], a["bias"], a["bias_dtype"],
                                                None if a["o"] == "null" else ctypes.byref(a["o"]), a["y"], None)
    assert call(o="null") == LSQ_EINVAL and b"NULL output description" in err()
    assert call(g=None) == LSQ_EINVAL and b"NULL geometry" in err()
    assert call(level_dtype=2) == LSQ_EINVAL and b"level_dtype" in err()
    assert call(w_level_dtype=-1) == LSQ_EINVAL and b"w_level_dtype" in err()
    for name in ("x", "s_x", "zx", "w", "s_w", "zw", "y"):
        assert call(**{name: None}) == LSQ_EINVAL and b"NULL buffer" in err(), name
    assert call(s_x=s_x.data_ptr() + 2) == LSQ_EINVAL and b"s_x and zx must be element-aligned" in err()
    assert call(zx=zx.data_ptr() + 1) == LSQ_EINVAL and b"s_x and zx must be element-aligned" in err()
    assert call(s_w=s_w.data_ptr() + 2) == LSQ_EINVAL and b"w_scale, w_zero and bias" in err()
    assert call(zw=zw.data_ptr() + 3) == LSQ_EINVAL and b"w_scale, w_zero and bias" in err()
    assert call(bias=bias.data_ptr() + 2, bias_dtype=E.LSQ_F32) == LSQ_EINVAL and b"w_scale, w_zero and bias" in err()
    assert call(bias=bias.data_ptr(), bias_dtype=E.LSQ_BF16) == LSQ_EINVAL and b"float32 or of mid_dtype" in err()
    assert call(bias=bias.data_ptr(), bias_dtype=E.LSQ_F64) == LSQ_EINVAL and b"float32 or of mid_dtype" in err()
    for bad, msg in ((dict(out_scale=None), b"come together"), (dict(out_shift=None), b"come together"),
                     (dict(out_scale=osc.data_ptr() + 2), b"element-aligned"), (dict(out_shift=osh.data_ptr() + 3), b"element-aligned"),
                     (dict(mid_dtype=E.LSQ_F64), b"mid_dtype"), (dict(mid_dtype=7), b"mid_dtype"), (dict(act=3), b"act must be"),
                     (dict(act=-1), b"act must be"), (dict(quant_min=5, quant_max=4), b"must lie within"),
                     (dict(quant_min=-1, quant_max=255), b"must lie within"), (dict(type_min=-129, type_max=0), b"must lie within"),
                     (dict(type_min=3, type_max=2), b"must lie within"), (dict(quant_min=0, quant_max=256), b"must lie within")):
        assert call(outq(**bad)) == LSQ_EINVAL and msg in err(), (bad, err())
    for bad, msg in ((dict(Cout=32), b"channel multiplier"), (dict(kh=65, kw=64, H=80, W=80), b"at most 4096"), (dict(ph=-1), b"negative padding")):
        assert call(g=geom(**bad)) == LSQ_EINVAL and msg in err(), (bad, err())
    # y overlapping x, in bytes of either; a floating y counts its element size and is element-aligned
    for off in (0, 100, 2 * 9 * 7 * 16 - 1):
        assert call(y=x.data_ptr() + off) == LSQ_EINVAL and b"overlap" in err()
    assert call(x=x.data_ptr() + 63, y=x.data_ptr()) == LSQ_EINVAL and b"overlap" in err()
    floats = outq(out_scale=None, out_shift=None)
    assert call(floats, x=y.data_ptr() + 2 * 9 * 7 * 16 * 4 - 1) == LSQ_EINVAL and b"overlap" in err()
    assert call(floats, y=y.data_ptr() + 2) == LSQ_EINVAL and b"element-aligned" in err()
    assert call(outq(out_scale=None, out_shift=None, mid_dtype=E.LSQ_BF16), y=y.data_ptr() + 1) == LSQ_EINVAL and b"element-aligned" in err()


def test_host_checks_of_the_ops():
    from torchlsq.functional import LevelsTensor, lsq_depthwise_conv2d_w8a8, lsq_depthwise_conv2d_w8a8_q
    for name in ("lsq_dwconv2d_w8_q8_q", "lsq_dwconv2d_w8_q8"):
        assert hasattr(OPS, name)
    c = D.case(D.GEOMETRIES[0], D.VARIANTS[0], (True, torch.float32, 1))
    lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, act, mid = c
    flt = (lx, s, z, lw, s_w, zw, bias, *geo)
    with pytest.raises(RuntimeError, match="uint8 .* or int8"):
        OPS.lsq_dwconv2d_w8_q8(lx.float(), *flt[1:], 0, torch.float32)
    with pytest.raises(RuntimeError, match="weight levels must be int8"):
        OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw.float(), *flt[4:], 0, torch.float32)
    with pytest.raises(RuntimeError, match=r"tap-major, \[kh, kw, C\]"):
        OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw.permute(2, 0, 1).unsqueeze(1), *flt[4:], 0, torch.float32)
    with pytest.raises(RuntimeError, match="one filter per channel"):
        OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw[:, :, :8].contiguous(), *flt[4:], 0, torch.float32)
    with pytest.raises(RuntimeError, match=r"\[B, C, H, W\]"):
        OPS.lsq_dwconv2d_w8_q8(lx[0], *flt[1:], 0, torch.float32)
    with pytest.raises(RuntimeError, match="one float32 value"):
        OPS.lsq_dwconv2d_w8_q8(lx, s.double(), *flt[2:], 0, torch.float32)
    with pytest.raises(RuntimeError, match="w_scale must be 16 float32"):
        OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_w[:8], *flt[5:], 0, torch.float32)
    with pytest.raises(RuntimeError, match="w_zero must be 16 int32"):
        OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_w, zw.long(), *flt[6:], 0, torch.float32)
    with pytest.raises(RuntimeError, match="the bias needs 16 values"):
        OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_w, zw, bias[:3], *geo, 0, torch.float32)
    with pytest.raises(RuntimeError, match="bias must be float32 or of out_dtype"):
        OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_w, zw, bias.half(), *geo, 0, torch.bfloat16)
    with pytest.raises(RuntimeError, match="out_dtype must be"):
        OPS.lsq_dwconv2d_w8_q8(*flt, 0, torch.float64)
    with pytest.raises(RuntimeError, match="mid_dtype must be"):
        OPS.lsq_dwconv2d_w8_q8_q(*flt, osc, osh, *rng, 0, torch.float64)
    with pytest.raises(RuntimeError, match="act must be 0"):
        OPS.lsq_dwconv2d_w8_q8(*flt, 3, torch.float32)
    with pytest.raises(RuntimeError, match="must lie within"):
        OPS.lsq_dwconv2d_w8_q8_q(*flt, osc, osh, -1, 255, 0, 255, 0, torch.float32)
    with pytest.raises(RuntimeError, match="empty output"):
        OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_w, zw, bias, [1, 1], [0, 0], [5, 5], 0, torch.float32)
    with pytest.raises(RuntimeError, match="negative padding"):
        OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_w, zw, bias, [1, 1], [-1, 0], [1, 1], 0, torch.float32)
    with pytest.raises(RuntimeError, match="inference-only"):
        OPS.lsq_dwconv2d_w8_q8_q(*flt, osc.clone().requires_grad_(True), osh, *rng, 0, torch.float32)
    with pytest.raises(RuntimeError, match="inference-only"):
        OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_w.clone().requires_grad_(True), zw, bias, *geo, 0, torch.float32)
    # the functional entry points: a [C, 1, kh, kw] quantized weight, permuted per call; a channel multiplier is refused
    wq = torch._make_per_channel_quantized_tensor(lw.permute(2, 0, 1).unsqueeze(1).contiguous(), s_w.double(), zw.long(), 0)
    x = LevelsTensor(lx, s, z, 0, 255)
    got = lsq_depthwise_conv2d_w8a8_q(x, wq, bias, 1, 1, 1, out_scale=osc, out_shift=osh, out_quant_min=0, out_quant_max=255, act="relu")
    assert isinstance(got, LevelsTensor) and torch.equal(got.levels, D.run(c)) and got.levels.is_contiguous(memory_format=CL)
    xq = torch._make_per_tensor_quantized_tensor(lx, float(s), int(z))
    assert torch.equal(lsq_depthwise_conv2d_w8a8_q(xq, wq, bias, 1, 1, 1, out_scale=osc, out_shift=osh, out_quant_min=0, out_quant_max=255,
                                                   act="relu").levels, got.levels)
    f = lsq_depthwise_conv2d_w8a8(x, wq, bias, 1, "same", 1, act="relu6", out_dtype=torch.bfloat16)
    assert f.dtype == torch.bfloat16 and torch.equal(f, OPS.lsq_dwconv2d_w8_q8(*flt, 2, torch.bfloat16))
    # a floating x goes through lsq_levels_per_tensor with the input quantizer's constants first
    xf = x.dequantize(torch.float32)
    in_s, in_b = s.clone(), -z.float() * s
    ff = lsq_depthwise_conv2d_w8a8(xf, wq, bias, 1, 1, 1, scale=in_s, shift=in_b, quant_min=0, quant_max=255, act="none")
    lv = OPS.lsq_levels_per_tensor(xf, in_s, in_b, 0, 255, 0, 255, 0).view(torch.uint8)
    assert ff.dtype == torch.float32 and torch.equal(ff, OPS.lsq_dwconv2d_w8_q8(lv, *flt[1:], 0, torch.float32))
    with pytest.raises(AssertionError, match="channel multiplier"):
        lsq_depthwise_conv2d_w8a8(x, torch._make_per_channel_quantized_tensor(torch.zeros(32, 2, 3, 3, dtype=torch.int8), torch.ones(32).double(),
                                                                              torch.zeros(32).long(), 0))
    with pytest.raises(AssertionError, match="act must be"):
        lsq_depthwise_conv2d_w8a8(x, wq, act="gelu")
    with pytest.raises(AssertionError, match="out_scale"):
        lsq_depthwise_conv2d_w8a8_q(x, wq)
    # an empty batch; an NCHW levels tensor (copied to channels-last first)
    assert OPS.lsq_dwconv2d_w8_q8(lx[:0], *flt[1:], 0, torch.bfloat16).shape == (0, 16, 9, 7)
    assert OPS.lsq_dwconv2d_w8_q8_q(lx[:0], *flt[1:], osc, osh, *rng, 0, torch.float32).dtype == torch.uint8
    assert not lx.contiguous().is_contiguous(memory_format=CL)
    assert torch.equal(OPS.lsq_dwconv2d_w8_q8_q(lx.contiguous(), *flt[1:], osc, osh, *rng, act, mid), D.run(c))
    # the fake kernels: shapes, dtypes and the memory format of the real ones
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        fa = [None if t is None else mode.from_tensor(t) for t in (lx, s, z, lw, s_w, zw, bias)]
        fo, fh = mode.from_tensor(osc), mode.from_tensor(osh)
        q = OPS.lsq_dwconv2d_w8_q8_q(*fa, [2, 2], [1, 1], [1, 1], fo, fh, -128, 127, -128, 127, 2, torch.float32)
        fl = OPS.lsq_dwconv2d_w8_q8(*fa, [1, 1], [2, 2], [2, 2], 0, torch.float16)
    assert (q.shape, q.dtype) == ((2, 16, 5, 4), torch.int8) and q.is_contiguous(memory_format=CL)
    assert (fl.shape, fl.dtype) == ((2, 16, 9, 7), torch.float16) and fl.is_contiguous(memory_format=CL)


@pytest.mark.parametrize("variant", D.VARIANTS, ids=range(len(D.VARIANTS)))
@pytest.mark.parametrize("geometry", D.GEOMETRIES, ids=D.geom_id)
def test_cpu_path_is_the_dense_embedding_through_the_existing_ops(geometry, variant):
    """every mid and act, levels out (both types) and floats out: torch.equal on the bits"""
    stats = []
    for out_variant in D.OUT_VARIANTS:
        c = D.case(geometry, variant, out_variant, 5)
        got, want = D.run(c), D.composed(c)
        assert got.dtype == want.dtype and got.shape == want.shape and got.is_contiguous(memory_format=CL)
        assert torch.equal(D.bits(got), D.bits(want)), (geometry, variant, out_variant)
        if out_variant[0] is not None and got.numel() >= 1000:
            stats.append(D.assert_conditions(got, c, (geometry, variant, out_variant)))
    if stats:
        print("non-vacuity %s variant %s: inside %.2f-%.2f, tap roll %.2f-%.2f, channel roll %.2f-%.2f" % (
            D.geom_id(geometry), variant[:4], min(s[0] for s in stats), max(s[0] for s in stats), min(s[1] for s in stats),
            max(s[1] for s in stats), min(s[2] for s in stats), max(s[2] for s in stats)))


@pytest.mark.parametrize("variant", D.VARIANTS, ids=range(len(D.VARIANTS)))
@pytest.mark.parametrize("geometry", D.GEOMETRIES, ids=D.geom_id)
def test_cpu_path_is_the_numpy_restatement_bit_for_bit(geometry, variant):
    for unsigned, mid, act in D.OUT_VARIANTS:
        c = D.case(geometry, variant, (unsigned, mid, act), 7)
        lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, _, _ = c
        v, I = D.numpy_value(lx, s, int(z), lw, s_w, zw, bias, geo)
        assert int(np.abs(I).max()) > 1000
        u = torch.from_numpy(v).to(mid).float().numpy()
        if act >= 1:
            u = np.where(u < 0, np.float32(0), u)
        if act == 2:
            u = np.where(u > 6, np.float32(6), u)
        got = D.run(c)
        if unsigned is None:
            assert got.dtype == mid and torch.equal(D.bits(got), D.bits(torch.from_numpy(u).to(mid)))
        else:
            assert got.dtype == (torch.uint8 if unsigned else torch.int8)
            assert torch.equal(got.to(torch.int64), torch.from_numpy(D.numpy_levels(u, osc, osh, rng))), (geometry, variant, unsigned, mid, act)


@pytest.mark.parametrize("mid", D.MIDS, ids=lambda v: str(v).replace("torch.", ""))
def test_act_2_is_relu6_on_the_mid_tensor(mid):
    c = D.case(D.GEOMETRIES[0], D.VARIANTS[0], (None, mid, 0), 9)
    u = D.run(c)
    assert bool((u.float() > 6).any()) and bool((u.float() < 0).any())
    for act, fn in ((1, F.relu), (2, F.relu6)):
        got = D.run(c[:11] + (act, mid))
        assert torch.equal(D.bits(got), D.bits(fn(u.float()).to(mid)))
    cq = D.case(D.GEOMETRIES[0], D.VARIANTS[0], (True, mid, 2), 9)
    assert torch.equal(D.run(cq), R.levels_of(F.relu6(D.run(cq[:8] + (None, None, None, 0, mid)).float()).to(mid), cq[8], cq[9], cq[10], False))


def test_rounding_at_ties_is_half_to_even_and_a_nan_stays_a_nan():
    # a 1 x 1 kernel of weight level 1, s_w = s_x = 1, zero points 0: v is the level itself; scale 2: levels l / 2 + 64, odd l are ties
    lx = torch.arange(0, 32, dtype=torch.uint8).reshape(1, 1, 4, 8).repeat(1, 16, 1, 1).contiguous(memory_format=CL)
    s, z = W.act(1.0, 0)
    lw, s_w, zw = torch.ones(1, 1, 16, dtype=torch.int8), torch.ones(16), torch.zeros(16, dtype=torch.int32)
    one = ([1, 1], [0, 0], [1, 1])
    got = OPS.lsq_dwconv2d_w8_q8_q(lx, s, z, lw, s_w, zw, None, *one, torch.tensor([2.0]), torch.tensor([-128.0]), 0, 255, 0, 255, 0, torch.float32)
    l = np.arange(32)
    want = np.where(l % 2 == 0, l // 2, np.where((l // 2) % 2 == 0, l // 2, l // 2 + 1)) + 64
    assert torch.equal(got[0, 0].flatten().to(torch.int64), torch.from_numpy(want))
    # ReLU6 on the levels 0..31: 7.. become 6 exactly, in every mid
    for mid in D.MIDS:
        f = OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_w, zw, None, *one, 2, mid)
        assert f[0, 3].flatten().tolist() == [float(min(v, 6)) for v in range(32)]
    # a NaN weight scale in channel 5: the selects keep the NaN (floats out), the level is quant_min (levels out), whatever act
    s_nan = s_w.clone()
    s_nan[5] = float("nan")
    for act in D.ACTS:
        f = OPS.lsq_dwconv2d_w8_q8(lx, s, z, lw, s_nan, zw, None, *one, act, torch.float32)
        assert bool(f[:, 5].isnan().all()) and not bool(f[:, 4].isnan().any())
        for rng in ((3, 200, 0, 255), (-100, 100, -128, 127)):
            q = OPS.lsq_dwconv2d_w8_q8_q(lx, s, z, lw, s_nan, zw, None, *one, torch.tensor([0.5]), torch.tensor([0.0]), *rng, act, torch.bfloat16)
            assert bool((q[:, 5].to(torch.int64) == rng[0]).all()) and not bool((q[:, 4].to(torch.int64) == rng[0]).all())


def test_state_dict_round_trips():
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import DepthwiseConv2dW8A8Q
    net, qs, x = D.inverted_residual()
    with torch.no_grad():
        h = net.expand(qs["in"](x))
    xl = LevelsTensor.from_quantized(qs["hidden"].quantize(h))
    m = DepthwiseConv2dW8A8Q.from_float(net.depthwise[0], qs["hidden"], qs["dw"], act="relu6", mid_dtype=torch.bfloat16)
    fresh = DepthwiseConv2dW8A8Q(48, 3, padding=1)
    fresh.load_state_dict(m.state_dict())
    assert {"weight_levels", "weight_scale", "weight_zero_point", "input_scale", "input_shift", "output_scale", "output_shift"} <= \
        set(dict(m.named_buffers()))
    assert m.weight_levels.shape == (3, 3, 48) and m.weight_levels.dtype == torch.int8 and m.weight_levels.is_contiguous()
    assert (fresh.act, fresh.mid_dtype, fresh.quantized, fresh.output_range) == ("relu6", torch.bfloat16, True, m.output_range)
    assert "output levels" in repr(fresh) and "act=relu6" in repr(fresh)
    want = m(xl)
    assert isinstance(want, LevelsTensor) and torch.equal(fresh(xl).levels, want.levels) and len(want.levels.unique()) > 16
    wq = net.depthwise[0].weight_fake_quant.quantize(net.depthwise[0].weight.detach())
    assert torch.equal(m.weight_levels, wq.int_repr()[:, 0].permute(1, 2, 0))
    assert torch.equal(want.levels, OPS.lsq_dwconv2d_w8_q8_q(xl.levels, xl.scale, xl.zero_point, m.weight_levels, m.weight_scale,
                                                             m.weight_zero_point, m.bias, [1, 1], [1, 1], [1, 1], m.output_scale,
                                                             m.output_shift, *m.output_range, 2, torch.bfloat16))
    # a floating x is quantized with the input quantizer first: the same levels
    assert torch.equal(m(h).levels, want.levels)
    # no output quantizer: floats out, and that travels in the state too
    f = DepthwiseConv2dW8A8Q.from_float(net.depthwise[0], qs["hidden"], None, act="relu", mid_dtype=torch.float16)
    fresh = DepthwiseConv2dW8A8Q(48, 3, padding=1)
    fresh.load_state_dict(f.state_dict())
    y = fresh(xl)
    assert not fresh.quantized and y.dtype == torch.float16 and y.shape == (2, 48, 9, 7) and "floating output" in repr(fresh)
    assert torch.equal(y, OPS.lsq_dwconv2d_w8_q8(xl.levels, xl.scale, xl.zero_point, m.weight_levels, m.weight_scale, m.weight_zero_point,
                                                 m.bias, [1, 1], [1, 1], [1, 1], 1, torch.float16))
    with pytest.raises(ValueError, match="groups == in_channels == out_channels"):
        DepthwiseConv2dW8A8Q.from_float(net.project, qs["dw"], None)
    with pytest.raises(ValueError, match="act must be"):
        DepthwiseConv2dW8A8Q.from_float(net.depthwise[0], qs["hidden"], None, act="gelu")
    with pytest.raises(ValueError, match="LSQFakeQuantizer"):
        DepthwiseConv2dW8A8Q.from_float(net.depthwise[0], None, None)


@pytest.mark.parametrize("mid", R.MIDS, ids=lambda v: str(v).replace("torch.", ""))
def test_convert_w8a8_depthwise_on_an_inverted_residual_block_equals_the_modules_written_out(mid):
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import AddW8A8Q, Conv2dW8A8AddQ, Conv2dW8A8Q, DepthwiseConv2dW8A8Q, convert_w8a8_depthwise
    net, qs, x = D.inverted_residual()
    new = D.convert_inverted_residual(net, qs, mid)
    assert isinstance(new.expand[0], Conv2dW8A8Q) and isinstance(new.expand[1], torch.nn.Identity)
    assert isinstance(new.depthwise[0], DepthwiseConv2dW8A8Q) and isinstance(new.depthwise[1], torch.nn.Identity)
    assert isinstance(new.project, Conv2dW8A8AddQ) and isinstance(new.add, AddW8A8Q)
    assert (new.depthwise[0].act, new.depthwise[0].mid_dtype, new.depthwise[0].quantized) == ("relu6", mid, True)
    assert isinstance(net.depthwise[1], torch.nn.ReLU6) and isinstance(net.depthwise[0], torch.nn.Conv2d)      # a deep copy
    xl = LevelsTensor.from_quantized(qs["in"].quantize(x))
    got = new(xl)                                                                            # the block's own forward
    want, h, d = D.inverted_residual_written_out(net, qs, xl, mid)
    assert isinstance(got, LevelsTensor) and got.levels.shape == (2, 16, 9, 7) and torch.equal(got.levels, want.levels)
    assert len(want.levels.unique()) > 16 and len(d.levels.unique()) > 16 and isinstance(d, LevelsTensor) and d.levels.shape == (2, 48, 9, 7)
    # ReLU6 is in the kernel: the depthwise layer's levels are those of the unfused float layer on the same input levels
    with torch.no_grad():
        ref = F.relu6(F.conv2d(h.dequantize(), net.depthwise[0].weight_fake_quant(net.depthwise[0].weight), net.depthwise[0].bias, 1, 1, 1, 48))
    close = (qs["dw"].quantize(ref).int_repr().to(torch.int64) - d.levels.to(torch.int64)).abs()
    assert int(close.max()) <= 1 and float((close == 0).double().mean()) > 0.9
    # refusals of the converter, by name
    with pytest.raises(ValueError, match="'project' is not a 2-D convolution with groups"):
        convert_w8a8_depthwise(net, {"project": qs["dw"]}, {})
    with pytest.raises(ValueError, match="listed in output_quantizers, relu or relu6 but not"):
        convert_w8a8_depthwise(net, {"depthwise.0": qs["hidden"]}, {}, relu6=("expand.0",))
    with pytest.raises(ValueError, match="listed in relu and in relu6"):
        convert_w8a8_depthwise(net, {"depthwise.0": qs["hidden"]}, {}, relu=("depthwise.0",), relu6=("depthwise.0",))
    # without an output quantizer the layer gives floats; relu on a layer followed by ReLU6 leaves that module alone
    fl = convert_w8a8_depthwise(net, {"depthwise.0": qs["hidden"]}, {}, relu=("depthwise.0",), mid_dtype=mid)
    assert not fl.depthwise[0].quantized and isinstance(fl.depthwise[1], torch.nn.ReLU6) and fl.depthwise[0](h).dtype == mid
    # the dense converters keep refusing the grouped layer
    from torchlsq.quantized import convert_w8a8_q
    with pytest.raises(ValueError, match="groups == 1"):
        convert_w8a8_q(net, {"depthwise.0": qs["hidden"]}, {"depthwise.0": qs["dw"]})
