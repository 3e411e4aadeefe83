"""Pooling on 8-bit levels (include/lsq_hip_pool_w8.h), everything that needs no GPU: the library's exports against its header
and `_abi.py`, its kernel set, the plans on both sides of every threshold, every refusal, and the CPU path of the ops -- the
definition the GPU tests compare against -- held to torch's own pooling, to an independent numpy restatement (bit for bit) and to
the float64 mean (two roundings), with the modules and the converter on top.
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

import pool_w8_cases as P
import requant_w8_cases as R
import resadd_w8_cases as A
from helpers import LLVM, demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_pool_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_pool_w8.so")
NAMES = sorted(["lsq_pool_w8_abi_version", "lsq_pool_w8_last_error", "lsq_pool_w8_max", "lsq_pool_w8_avg_forward", "lsq_pool_w8_adaptive",
                "lsq_pool_w8_plan_max", "lsq_pool_w8_plan_avg"])
LSQ_EINVAL = -1
CL = torch.channels_last
OPS = torch.ops.torchlsq


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    return [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(const void\*|int64_t)", "", decl.strip()).split(",") if f.strip()]


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_pool_w8_\w+)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_POOL_W8) == NAMES and len(NAMES) == 7
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_", "lsq_requant_", "lsq_resadd_",
                  "lsq_pool_"):
        assert other not in und, other
    assert E.pool_w8_library().lsq_pool_w8_abi_version() == E.POOL_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_POOL_W8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    assert _fields(text, "lsq_pool_w8_geom") == [f[0] for f in E.LsqPoolW8Geom._fields_] and ctypes.sizeof(E.LsqPoolW8Geom) == 13 * 8
    assert _fields(text, "lsq_pool_w8_avg") == [f[0] for f in E.LsqPoolW8Avg._fields_] and ctypes.sizeof(E.LsqPoolW8Avg) == 12 * 8


def test_kernels(tmp_path):
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    short = {}
    for sym, dm in names.items():
        m = re.match(r"^(?:void )?lsq::pool_w8_(max_packets|max_generic|avg_lane|avg_shared|avg_generic)_kernel(?:<([^>]*)>)?\(", dm)
        assert m, "not a kernel of this library: %s" % dm
        short[sym] = m.group(1) + "".join("_" + n for n in re.findall(r"\d+", re.sub(r"\(int\)", "", m.group(2) or "")))
    # max_packets_<pixels per lane>_<K>, avg_lane_<K>: K = 2, 3 the unrolled K x K window, 0 any window
    assert sorted(short.values()) == ["avg_generic", "avg_lane_0", "avg_lane_2", "avg_lane_3", "avg_shared", "max_generic", "max_packets_1_0",
                                      "max_packets_1_2", "max_packets_1_3"]
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
        assert 0 < vgprs[sym] <= 64, (sym, vgprs[sym])                    # 8 waves per SIMD: bandwidth kernels
        assert lds[sym] == (16384 if short[sym] == "avg_shared" else 0), (sym, lds[sym])
        if short[sym].startswith(("max_packets", "avg_lane", "avg_shared")):
            assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops, sym


def _plan_raw(fn, g, aligned=1):
    out = (ctypes.c_int32 * 8)()
    return fn(ctypes.byref(g), aligned, ctypes.byref(out)), list(out)


def test_plan_without_a_gpu():
    from torchlsq import extension as E
    # the max pool: packets if and only if C % 16 == 0 and the buffers are aligned
    for C, aligned in itertools.product((3, 15, 16, 17, 20, 24, 32, 48), (True, False)):
        pl = E.pool_w8_plan_max(2, C, 9, 7, 3, 2, 1, aligned=aligned)
        packets = aligned and C % 16 == 0
        assert pl["family"] == ("packets" if packets else "generic") and pl["block"] == 256 and pl["pixels_per_lane"] == 1, (C, pl)
        assert (pl["OH"], pl["OW"]) == (5, 4) and pl["unrolled_window"] == (3 if packets else 0)
        assert pl["grid"] == -(-(2 * 5 * 4 * (C // 16 if packets else C)) // 256), (C, pl)
    assert E.pool_w8_plan_max(32, 64, 112, 112, 3, 2, 1) == dict(family="packets", grid=32 * 56 * 56 * 4 // 256, block=256, pixels_per_lane=1,
                                                                 OH=56, OW=56, unrolled_window=3)
    # the unrolled windows: 2 x 2 and 3 x 3 without dilation, nothing else
    for k, d, want in ((2, 1, 2), (3, 1, 3), ((3, 2), 1, 0), ((2, 3), 1, 0), (3, (1, 2), 0), (3, 2, 0), (1, 1, 0), (4, 1, 0), (5, 1, 0)):
        assert E.pool_w8_plan_max(2, 16, 12, 12, k, 1, 0, d)["unrolled_window"] == want, (k, d)
        if d == 1:
            pl = E.pool_w8_plan_avg(2, 16, 12, 12, k, 1, 0)
            assert pl["unrolled_window"] == (want if pl["family"] == "packets" else 0) and pl["family"] != "generic", (k, pl)
    assert E.pool_w8_plan_avg(2, 16, 12, 12, 3, 1, 0)["unrolled_window"] == 3 and E.pool_w8_plan_avg(2, 16, 12, 12, (3, 2), 1, 0)["unrolled_window"] == 0
    # output sizes: torch's rule, ceil_mode's last window included
    for H, W, k, s, p, d, ceil_mode in P.MAX_GEOMS + [(7, 7, (3, 3), (2, 2), (1, 1), (1, 1), True), (5, 6, (2, 2), (2, 2), (1, 1), (1, 1), True),
                                                      (10, 4, (3, 3), (3, 3), (1, 1), (1, 1), True)]:
        pl = E.pool_w8_plan_max(1, 16, H, W, k, s, p, d, ceil_mode)
        want = F.max_pool2d(torch.zeros(1, 1, H, W), k, s, p, d, ceil_mode).shape[2:]
        assert (pl["OH"], pl["OW"]) == tuple(want) == P.out_hw(H, W, k, s, p, d, ceil_mode), (H, W, k, s, p, d, ceil_mode)
    # the average pool: the family, the lanes that share a window and the grid on both sides of every threshold
    seen = set()
    cases = [(1, 16, 6, 6, (3, 3)), (1, 16, 4, 10, (2, 5)),                          # 9 | 10 taps
             (1, 16, 3, 5, (3, 5)), (1, 16, 4, 4, (4, 4)), (1, 16, 5, 3, (5, 3)),    # 15 | 16 taps: 8 | 16 lanes at most
             (1, 16, 15, 17, (15, 17)), (1, 16, 16, 16, (16, 16)), (1, 16, 33, 31, (33, 31)), (1, 16, 260, 260, (260, 260)),
             (3, 32, 7, 7, (7, 7)), (1, 16, 8, 6, (4, 3)),
             (32, 512, 7, 7, (7, 7)), (32, 2048, 7, 7, (7, 7)), (256, 2048, 7, 7, (7, 7)), (32, 256, 56, 56, (2, 2)),
             (1022, 2048, 7, 7, (7, 7)), (1023, 2048, 7, 7, (7, 7)),                 # 511 | 512 workgroups with a window per lane
             (8, 16, 256, 635, (2, 5)), (8, 16, 256, 640, (2, 5)),
             (511, 2048, 7, 7, (7, 7)), (512, 2048, 7, 7, (7, 7)),                   # 2 | 4 lanes
             (2, 24, 7, 7, (7, 7)), (2, 3, 6, 6, (3, 3))]
    for (B, C, H, W, k), aligned in itertools.product(cases, (True, False)):
        pl = E.pool_w8_plan_avg(B, C, H, W, k, aligned=aligned)
        OH, OW = H // k[0], W // k[1]
        family, lanes, grid = P.expected_avg_plan(B, C, OH, OW, k[0] * k[1], aligned)
        assert (pl["family"], pl["lanes_per_window"], pl["grid"], pl["OH"], pl["OW"], pl["block"]) == (family, lanes, grid, OH, OW, 256), (B, C, H, W, k, pl)
        assert pl["lds_bytes"] == (16384 if family == "packets_shared" else 0)
        assert pl["packets_per_workgroup"] == (256 // lanes if family == "packets_shared" else 0)
        seen.add((family, lanes))
    assert seen >= {("generic", 1), ("packets", 1)} | {("packets_shared", n) for n in (2, 4, 8, 16, 32, 128, 256)}, seen
    assert E.pool_w8_plan_avg(32, 2048, 7, 7, 7)["lanes_per_window"] == 32 and E.pool_w8_plan_avg(256, 2048, 7, 7, 7)["lanes_per_window"] == 4
    assert E.pool_w8_plan_avg(32, 256, 56, 56, 2)["family"] == "packets"


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.pool_w8_library()
    err = lib.lsq_pool_w8_last_error
    G = E.LsqPoolW8Geom

    def geom(**kw):
        base = dict(B=2, C=16, H=9, W=7, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1, dh=1, dw=1, ceil_mode=0)
        base.update(kw)
        return G(*[base[f[0]] for f in G._fields_])
    out = (ctypes.c_int32 * 8)()
    for fn in (lib.lsq_pool_w8_plan_max, lib.lsq_pool_w8_plan_avg):
        assert fn(None, 1, ctypes.byref(out)) == LSQ_EINVAL and b"NULL geometry" in err()
        assert fn(ctypes.byref(geom()), 1, None) == LSQ_EINVAL and b"NULL output" in err()
        for bad, msg in ((dict(B=0), b"at least 1"), (dict(C=0), b"at least 1"), (dict(H=0), b"at least 1"), (dict(W=-1), b"at least 1"),
                         (dict(kh=0), b"kernel"), (dict(kw=-2), b"kernel"), (dict(sh=0), b"stride"), (dict(sw=0), b"stride"),
                         (dict(dh=0), b"dilation"), (dict(ph=2), b"half the kernel"), (dict(pw=-1), b"half the kernel"),
                         (dict(kh=2, ph=2), b"half the kernel"), (dict(H=2, ph=0), b"empty output"), (dict(W=1, pw=0), b"empty output"),
                         (dict(H=1 << 30), b"beyond 29 bits"), (dict(kh=1 << 12, kw=(1 << 11) + 1, H=1 << 13, W=1 << 13, ph=0, pw=0), b"2^23"),
                         (dict(B=1 << 40, H=1 << 20, W=1 << 20), b"64-bit")):
            assert fn(ctypes.byref(geom(**bad)), 1, ctypes.byref(out)) == LSQ_EINVAL and msg in err(), (bad, err())
    assert lib.lsq_pool_w8_plan_avg(ctypes.byref(geom(dw=2)), 1, ctypes.byref(out)) == LSQ_EINVAL and b"no dilation" in err()
    assert lib.lsq_pool_w8_plan_max(ctypes.byref(geom(dw=2)), 1, ctypes.byref(out)) == 0
    assert lib.lsq_pool_w8_plan_max(ctypes.byref(geom(H=2, dh=3)), 1, ctypes.byref(out)) == LSQ_EINVAL and b"may hold no tap" in err()
    assert lib.lsq_pool_w8_plan_max(ctypes.byref(geom(kh=1 << 12, kw=1 << 11, H=1 << 13, W=1 << 13, ph=0, pw=0)), 1, ctypes.byref(out)) == 0
    # the calls: everything is refused before anything is enqueued (no GPU here: an accepted call would fail in the launch)
    x = torch.zeros(2 * 9 * 7 * 16 + 64, dtype=torch.uint8)
    y = torch.zeros(2 * 5 * 4 * 16 * 4 + 64, dtype=torch.uint8)
    s_x, zx = torch.ones(3), torch.zeros(3, dtype=torch.int32)
    osc, osh = torch.ones(3), torch.zeros(3)
    g = geom()
    assert lib.lsq_pool_w8_max(2, x.data_ptr(), ctypes.byref(g), y.data_ptr(), None) == LSQ_EINVAL and b"level_dtype" in err()
    assert lib.lsq_pool_w8_max(0, None, ctypes.byref(g), y.data_ptr(), None) == LSQ_EINVAL and b"NULL buffer" in err()
    assert lib.lsq_pool_w8_max(0, x.data_ptr(), ctypes.byref(g), None, None) == LSQ_EINVAL and b"NULL buffer" in err()
    assert lib.lsq_pool_w8_max(0, x.data_ptr(), None, y.data_ptr(), None) == LSQ_EINVAL and b"NULL geometry" in err()
    assert lib.lsq_pool_w8_max(1, x.data_ptr(), ctypes.byref(geom(ph=2)), y.data_ptr(), None) == LSQ_EINVAL and b"half the kernel" in err()
    for off in (0, 100, 2 * 9 * 7 * 16 - 1):
        assert lib.lsq_pool_w8_max(0, x.data_ptr(), ctypes.byref(g), x.data_ptr() + off, None) == LSQ_EINVAL and b"overlap" in err()
    assert lib.lsq_pool_w8_max(0, x.data_ptr() + 639, ctypes.byref(g), x.data_ptr(), None) == LSQ_EINVAL and b"overlap" in err()

    def avg(**kw):
        base = dict(s_x=s_x.data_ptr(), zx=zx.data_ptr(), out_scale=osc.data_ptr(), out_shift=osh.data_ptr(), quant_min=0, quant_max=255,
                    type_min=0, type_max=255, mid_dtype=E.LSQ_F32, count_include_pad=1, has_divisor=0, divisor_override=0)
        base.update(kw)
        return E.LsqPoolW8Avg(*[base[f[0]] for f in E.LsqPoolW8Avg._fields_])

    def call(a, level_dtype=0, xp=x.data_ptr(), yp=y.data_ptr(), gg=g):
        return lib.lsq_pool_w8_avg_forward(level_dtype, xp, ctypes.byref(gg), None if a is None else ctypes.byref(a), yp, None)
    assert call(None) == LSQ_EINVAL and b"NULL constants" in err()
    assert call(avg(), level_dtype=-1) == LSQ_EINVAL and b"level_dtype" in err()
    for bad, msg in ((dict(s_x=None), b"NULL s_x or zx"), (dict(zx=None), b"NULL s_x or zx"), (dict(s_x=s_x.data_ptr() + 2), b"element-aligned"),
                     (dict(zx=zx.data_ptr() + 1), b"element-aligned"), (dict(out_scale=None), b"come together"),
                     (dict(out_shift=None), b"come together"), (dict(out_scale=osc.data_ptr() + 2), b"element-aligned"),
                     (dict(out_shift=osh.data_ptr() + 3), b"element-aligned"), (dict(mid_dtype=E.LSQ_F64), b"mid_dtype"),
                     (dict(mid_dtype=7), b"mid_dtype"), (dict(has_divisor=1, divisor_override=0), b"divisor_override"),
                     (dict(has_divisor=1, divisor_override=-3), b"divisor_override"), (dict(quant_min=5, quant_max=4), b"must lie within"),
                     (dict(quant_min=-1, quant_max=255), b"must lie within"), (dict(type_min=-129, type_max=0), b"must lie within"),
                     (dict(type_min=3, type_max=2), b"must lie within"), (dict(quant_min=0, quant_max=256), b"must lie within")):
        assert call(avg(**bad)) == LSQ_EINVAL and msg in err(), (bad, err())
    assert call(avg(), gg=geom(dh=2)) == LSQ_EINVAL and b"no dilation" in err()
    assert call(avg(), xp=None) == LSQ_EINVAL and b"NULL buffer" in err()
    assert call(avg(), yp=x.data_ptr() + 8) == LSQ_EINVAL and b"overlap" in err()
    # a floating y: its bytes count in the overlap, and it is element-aligned
    floats = avg(out_scale=None, out_shift=None)
    assert call(floats, xp=y.data_ptr() + 2 * 5 * 4 * 16 * 4 - 1) == LSQ_EINVAL and b"overlap" in err()
    assert call(floats, yp=y.data_ptr() + 2) == LSQ_EINVAL and b"element-aligned" in err()
    assert call(avg(out_scale=None, out_shift=None, mid_dtype=E.LSQ_BF16), yp=y.data_ptr() + 1) == LSQ_EINVAL and b"element-aligned" in err()
    # adaptive sizes
    ga = geom()
    assert lib.lsq_pool_w8_adaptive(3, 7, ctypes.byref(ga)) == 0 and (ga.kh, ga.kw, ga.sh, ga.sw, ga.ph, ga.pw, ga.dh, ga.dw) == (3, 1, 3, 1, 0, 0, 1, 1)
    assert lib.lsq_pool_w8_adaptive(2, 7, ctypes.byref(geom())) == LSQ_EINVAL and b"does not divide" in err()
    assert lib.lsq_pool_w8_adaptive(9, 2, ctypes.byref(geom())) == LSQ_EINVAL and b"does not divide" in err()
    assert lib.lsq_pool_w8_adaptive(0, 1, ctypes.byref(geom())) == LSQ_EINVAL and b"at least 1" in err()
    assert lib.lsq_pool_w8_adaptive(1, 1, None) == LSQ_EINVAL and b"NULL geometry" in err()


def test_host_checks_of_the_ops():
    from torchlsq.functional import (LevelsTensor, lsq_adaptive_avg_pool2d_w8, lsq_adaptive_avg_pool2d_w8_q, lsq_avg_pool2d_w8_q,
                                     lsq_max_pool2d_w8)
    for name in ("lsq_max_pool2d_q8", "lsq_avg_pool2d_q8_q", "lsq_avg_pool2d_q8"):
        assert hasattr(OPS, name)
    lx, s_x, zx = P.x_levels(2, 16, 9, 7, torch.uint8)
    args = ([3, 3], [2, 2], [1, 1], False, True, None)
    osc, osh = torch.tensor([0.1]), torch.tensor([0.0])
    with pytest.raises(RuntimeError, match="uint8 .* or int8"):
        OPS.lsq_max_pool2d_q8(lx.float(), [3, 3], [2, 2], [1, 1], [1, 1], False)
    with pytest.raises(RuntimeError, match="half the kernel"):
        OPS.lsq_max_pool2d_q8(lx, [3, 3], [2, 2], [2, 2], [1, 1], False)
    with pytest.raises(RuntimeError, match=r"\[B, C, H, W\]"):
        OPS.lsq_max_pool2d_q8(lx[0], [3, 3], [2, 2], [1, 1], [1, 1], False)
    with pytest.raises(RuntimeError, match="one float32 value"):
        OPS.lsq_avg_pool2d_q8(lx, s_x.double(), zx, *args, torch.float32)
    with pytest.raises(RuntimeError, match="out_dtype must be"):
        OPS.lsq_avg_pool2d_q8(lx, s_x, zx, *args, torch.float64)
    with pytest.raises(RuntimeError, match="mid_dtype must be"):
        OPS.lsq_avg_pool2d_q8_q(lx, s_x, zx, *args, osc, osh, 0, 255, 0, 255, torch.float64)
    with pytest.raises(RuntimeError, match="divisor_override must be at least 1"):
        OPS.lsq_avg_pool2d_q8(lx, s_x, zx, [3, 3], [2, 2], [1, 1], False, True, 0, torch.float32)
    with pytest.raises(RuntimeError, match="must lie within"):
        OPS.lsq_avg_pool2d_q8_q(lx, s_x, zx, *args, osc, osh, -1, 255, 0, 255, torch.float32)
    with pytest.raises(RuntimeError, match="inference-only"):
        OPS.lsq_avg_pool2d_q8_q(lx, s_x, zx, *args, osc.clone().requires_grad_(True), osh, 0, 255, 0, 255, torch.float32)
    with pytest.raises(RuntimeError, match="inference-only"):
        OPS.lsq_avg_pool2d_q8(lx, s_x.clone().requires_grad_(True), zx, *args, torch.float32)
    x = LevelsTensor(lx, s_x, zx, 0, 255)
    with pytest.raises(RuntimeError, match="does not divide"):
        lsq_adaptive_avg_pool2d_w8(x, 2)
    with pytest.raises(RuntimeError, match="does not divide"):
        lsq_adaptive_avg_pool2d_w8_q(x, (3, 2), out_scale=osc, out_shift=osh, out_quant_min=0, out_quant_max=255)
    with pytest.raises(AssertionError, match="out_scale"):
        lsq_avg_pool2d_w8_q(x, 3)
    with pytest.raises(AssertionError, match="LevelsTensor"):
        lsq_max_pool2d_w8(lx, 3)
    # an empty batch; an NCHW levels tensor (copied to channels-last first); the constants are handed on, not copied
    assert OPS.lsq_max_pool2d_q8(lx[:0], [3, 3], [2, 2], [1, 1], [1, 1], False).shape == (0, 16, 5, 4)
    assert OPS.lsq_avg_pool2d_q8(lx[:0], s_x, zx, *args, torch.bfloat16).shape == (0, 16, 5, 4)
    nchw = LevelsTensor(lx.contiguous(), s_x, zx, 0, 255)
    a, b = lsq_max_pool2d_w8(nchw, 3, 2, 1), lsq_max_pool2d_w8(x, 3, 2, 1)
    assert not nchw.levels.is_contiguous(memory_format=CL) and a.levels.is_contiguous(memory_format=CL) and torch.equal(a.levels, b.levels)
    assert b.scale.data_ptr() == x.scale.data_ptr() and b.zero_point.data_ptr() == x.zero_point.data_ptr() and (b.quant_min, b.quant_max) == (0, 255)
    # the fake kernels: shapes, dtypes and the memory format of the real ones
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        fl = mode.from_tensor(lx)
        fs, fz, fo, fh = (mode.from_tensor(t) for t in (s_x, zx, osc, osh))
        m = OPS.lsq_max_pool2d_q8(fl, [3, 3], [2, 2], [0, 0], [1, 1], True)
        q = OPS.lsq_avg_pool2d_q8_q(fl, fs, fz, *args, fo, fh, -128, 127, -128, 127, torch.float32)
        f = OPS.lsq_avg_pool2d_q8(fl, fs, fz, *args, torch.float16)
    assert (m.shape, m.dtype) == ((2, 16, 4, 3), torch.uint8) and m.is_contiguous(memory_format=CL)
    assert (q.shape, q.dtype, f.shape, f.dtype) == ((2, 16, 5, 4), torch.int8, (2, 16, 5, 4), torch.float16)


@pytest.mark.parametrize("dtype", P.LEVEL_DTYPES, ids=("u8", "i8"))
@pytest.mark.parametrize("geom", P.MAX_GEOMS, ids=P.geom_id)
def test_max_pool_is_torchs_on_the_integers_and_on_the_dequantized_values(geom, dtype):
    from torchlsq.functional import LevelsTensor, lsq_max_pool2d_w8
    H, W, k, s, p, d, ceil_mode = geom
    lx, s_x, zx = P.x_levels(2, 20, H, W, dtype, 3)
    lx = P.negative_corner(lx) if dtype == torch.int8 else lx
    x = LevelsTensor(lx, s_x, zx, *P.R.W.LEVEL_RANGE[dtype])
    got = lsq_max_pool2d_w8(x, k, s, p, d, ceil_mode)
    want = F.max_pool2d(lx.to(torch.int32).float(), k, s, p, d, ceil_mode)
    assert got.levels.dtype == dtype and got.levels.is_contiguous(memory_format=CL) and torch.equal(got.levels.float(), want)
    assert len(got.levels.unique()) > 32
    if dtype == torch.int8 and max(p) > 0:
        # a padded tap is -inf, not the byte 0: a window of negative levels at the border keeps its negative maximum
        assert bool((got.levels[:, :, 0, 0] < 0).all())
    for mid in P.MIDS:
        # dequantize is non-decreasing: pooling the dequantized values and going back to levels gives the same bytes
        pooled = F.max_pool2d(x.dequantize(mid).float(), k, s, p, d, ceil_mode).to(mid)
        back = OPS.lsq_levels_per_tensor(pooled.float(), s_x, -zx.float() * s_x, *x_range(dtype), 0)
        assert torch.equal(back.view(dtype) if dtype == torch.uint8 else back, got.levels), mid
        assert torch.equal(got.dequantize(mid), pooled), mid


def x_range(dtype):
    lo, hi = P.R.W.LEVEL_RANGE[dtype]
    return lo, hi, lo, hi


@pytest.mark.parametrize("variant", P.AVG_VARIANTS, ids=P.avg_id)
@pytest.mark.parametrize("case", P.AVG_LANE_CASES + [(7, 7, (7, 7), (7, 7), (0, 0), False, True, None),
                                                     (8, 6, (4, 3), (4, 3), (0, 0), False, True, None)], ids=P.geom_id)
def test_avg_pool_cpu_path_is_the_numpy_restatement_bit_for_bit(case, variant):
    unsigned, mid = variant
    for x_dtype in P.LEVEL_DTYPES:
        c = P.avg_case(3, 24, case, x_dtype, bool(unsigned), 7)
        lx, s_x, zx, args, osc, osh, rng = c
        v = P.numpy_avg(lx, s_x, zx, *case[2:])
        u = torch.from_numpy(v).to(mid)
        if unsigned is None:
            got = P.avg_float(lx, s_x, zx, args, mid)
            assert got.dtype == mid and got.is_contiguous(memory_format=CL)
            assert torch.equal(got.view(torch.int32 if mid == torch.float32 else torch.int16), u.view(torch.int32 if mid == torch.float32 else torch.int16))
            continue
        got = P.avg_q(*c, mid)
        want = torch.from_numpy(P.numpy_levels(u.float().numpy(), osc, osh, rng))
        assert got.dtype == (torch.uint8 if unsigned else torch.int8) and got.is_contiguous(memory_format=CL)
        assert torch.equal(got.to(torch.int64), want), (case, variant, x_dtype)
        if got.numel() >= 336:
            P.assert_conditions(got, c, mid, (case, variant, x_dtype))


@pytest.mark.parametrize("x_dtype", P.LEVEL_DTYPES, ids=("u8", "i8"))
def test_avg_pool_is_within_two_roundings_of_torchs_float64_mean(x_dtype):
    bound = 2.0 ** -22
    worst = 0.0
    for ceil_mode, cip, div, pad in itertools.product((False, True), (False, True), (None, 5), (0, 1)):
        for H, W, k, s in ((12, 11, (3, 3), (2, 2)), (9, 10, (2, 3), (2, 1)), (7, 7, (7, 7), (7, 7)) if pad == 0 else (7, 8, (4, 3), (3, 2))):
            lx, s_x, zx = P.x_levels(2, 5, H, W, x_dtype, 11)
            args = (list(k), list(s), [pad, pad], ceil_mode, cip, div)
            got = P.avg_float(lx, s_x, zx, args).double()
            want = P.exact_mean(lx, s_x, zx, args)
            assert got.shape == want.shape
            err = (got - want).abs()
            assert bool((err <= bound * want.abs()).all()), (ceil_mode, cip, div, pad, H, W, k, float((err / want.abs().clamp_min(1e-300)).max()))
            worst = max(worst, float((err / want.abs().clamp_min(1e-300))[want != 0].max()))
    assert 0 < worst < bound


def test_the_one_rounding_of_a_sum_beyond_24_bits():
    # 260 x 260 levels 255 with z_x = 0: S = 17 238 000 > 2^24; with three levels 254 S is odd and no float32: float(S) is rounded
    # once, then the two fp32 steps
    lx = torch.full((1, 16, 260, 260), 255, dtype=torch.uint8).contiguous(memory_format=CL)
    lx[0, 1::2, 7, 5:8] = 254
    s_x, zx = torch.tensor([0.0371]), torch.zeros(1, dtype=torch.int32)
    got = OPS.lsq_avg_pool2d_q8(lx, s_x, zx, [260, 260], [260, 260], [0, 0], False, True, None, torch.float32)
    S = 255 * 260 * 260
    assert S > 2 ** 24 and int(np.float32(S - 3)) == S - 4
    want = [(np.float32(S - 3 * (c % 2)) * np.float32(0.0371)) / np.float32(260 * 260) for c in range(16)]
    assert got.shape == (1, 16, 1, 1) and got.flatten().tolist() == [float(w) for w in want] and want[0] != want[1]


def test_rounding_at_ties_is_half_to_even_and_a_nan_goes_to_quant_min():
    # one tap per window, s_x = 1, z_x = 0: v is the level itself; scale 2: levels l / 2 + 64, the odd l are ties
    lx = torch.arange(0, 32, dtype=torch.uint8).reshape(1, 1, 4, 8).repeat(1, 16, 1, 1).contiguous(memory_format=CL)
    s_x, zx = torch.tensor([1.0]), torch.zeros(1, dtype=torch.int32)
    one = ([1, 1], [1, 1], [0, 0], False, True, None)
    got = OPS.lsq_avg_pool2d_q8_q(lx, s_x, zx, *one, torch.tensor([2.0]), torch.tensor([-128.0]), 0, 255, 0, 255, torch.float32)
    l = np.arange(32)
    want = np.where(l % 2 == 0, l // 2, np.where((l // 2) % 2 == 0, l // 2, l // 2 + 1)) + 64
    assert torch.equal(got[0, 0].flatten().to(torch.int64), torch.from_numpy(want))
    # a 2 x 2 window of (0, 1, 1, 1): v = 0.75, a division and not a multiple of a reciprocal; divisor 3: 1 exactly
    lx = torch.tensor([0, 1, 1, 1], dtype=torch.int8).reshape(1, 1, 2, 2).repeat(1, 16, 1, 1).contiguous(memory_format=CL)
    f = OPS.lsq_avg_pool2d_q8(lx, s_x, zx, [2, 2], [2, 2], [0, 0], False, True, 3, torch.float32)
    assert bool((f == 1.0).all())
    # a NaN scale of the input makes every v a NaN: quant_min, whatever the range
    for rng in ((3, 200, 0, 255), (-100, 100, -128, 127)):
        got = OPS.lsq_avg_pool2d_q8_q(lx, torch.tensor([float("nan")]), zx, [2, 2], [2, 2], [0, 0], False, True, None, torch.tensor([0.5]),
                                      torch.tensor([0.0]), *rng, torch.bfloat16)
        assert bool((got.to(torch.int64) == rng[0]).all())


def test_state_dict_round_trips():
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import AdaptiveAvgPool2dW8Q, AvgPool2dW8Q, MaxPool2dW8
    lx, s_x, zx = P.x_levels(2, 16, 12, 10, torch.uint8, 5)
    x = LevelsTensor(lx, s_x, zx, 0, 255)
    q = R.trained_quantizer(x.dequantize())
    m = AvgPool2dW8Q.from_float(torch.nn.AvgPool2d(3, 2, 1, ceil_mode=True, count_include_pad=False), q, torch.bfloat16)
    fresh = AvgPool2dW8Q(3, 2, 1, ceil_mode=True, count_include_pad=False)
    fresh.load_state_dict(m.state_dict())
    assert {"output_scale", "output_shift"} <= set(dict(m.named_buffers())) and fresh.mid_dtype == torch.bfloat16
    assert fresh.output_range == m.output_range and fresh.quantized and "output levels" in repr(fresh)
    want = m(x)
    assert isinstance(want, LevelsTensor) and torch.equal(fresh(x).levels, want.levels) and len(want.levels.unique()) > 16
    assert torch.equal(want.levels, OPS.lsq_avg_pool2d_q8_q(lx, s_x, zx, [3, 3], [2, 2], [1, 1], True, False, None, m.output_scale,
                                                            m.output_shift, *m.output_range, torch.bfloat16))
    a = AdaptiveAvgPool2dW8Q.from_float(torch.nn.AdaptiveAvgPool2d((3, 5)), None, torch.float16)
    fresh = AdaptiveAvgPool2dW8Q(1)
    fresh.output_size = (3, 5)
    fresh.load_state_dict(a.state_dict())
    assert not fresh.quantized and fresh.mid_dtype == torch.float16 and "floating output" in repr(fresh)
    y = fresh(x)
    assert y.dtype == torch.float16 and y.shape == (2, 16, 3, 5)
    assert torch.equal(y, OPS.lsq_avg_pool2d_q8(lx, s_x, zx, [4, 2], [4, 2], [0, 0], False, True, None, torch.float16))
    mp = MaxPool2dW8.from_float(torch.nn.MaxPool2d(3, 2, 1))
    assert mp.state_dict() == {} and torch.equal(mp(x).levels.float(), F.max_pool2d(lx.float(), 3, 2, 1)) and mp(x).scale.data_ptr() == x.scale.data_ptr()
    with pytest.raises(ValueError, match="output quantizer"):
        MaxPool2dW8.from_float(torch.nn.MaxPool2d(2), q)
    with pytest.raises(ValueError, match="needs an nn.AvgPool2d"):
        AvgPool2dW8Q.from_float(torch.nn.MaxPool2d(2), q)


@pytest.mark.parametrize("mid", R.MIDS, ids=lambda v: str(v).replace("torch.", ""))
def test_convert_w8a8_pool_on_a_small_network_equals_the_modules_and_ops_written_out(mid):
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import AdaptiveAvgPool2dW8Q, LinearW8A8Q, MaxPool2dW8, convert_w8a8_pool
    net, qs, x = P.small_net()
    new = P.convert_small_net(net, qs, mid)
    assert isinstance(new.maxpool, MaxPool2dW8) and isinstance(new.avgpool, AdaptiveAvgPool2dW8Q) and isinstance(new.fc, LinearW8A8Q)
    assert new.avgpool.quantized and new.avgpool.mid_dtype == mid
    assert isinstance(net.maxpool, torch.nn.MaxPool2d)                                         # a deep copy: the model is untouched
    xl = LevelsTensor.from_quantized(qs["x"].quantize(x))
    got = new(xl)                                                                             # the network's own forward
    want = P.small_net_written_out(net, qs, xl, mid)
    assert isinstance(got, LevelsTensor) and got.levels.shape == (4, 10) and torch.equal(got.levels, want) and len(want.unique()) > 16
    # the stretch between the stem and the classifier stays in levels
    h = new.maxpool(new.relu(new.stem(xl)))
    g = new.avgpool(new.block(h))
    assert isinstance(h, LevelsTensor) and h.levels.shape == (4, 16, 10, 10) and isinstance(g, LevelsTensor) and g.levels.shape == (4, 32, 1, 1)
    assert len(g.levels.unique()) > 16
    # None on the average pool: floats out; refusals of the converter
    fl = convert_w8a8_pool(net, {"avgpool": None}, mid_dtype=mid)
    assert not fl.avgpool.quantized and fl.avgpool(new.block(h)).dtype == mid
    with pytest.raises(ValueError, match="'maxpool' is a max pool"):
        convert_w8a8_pool(net, {"maxpool": qs["gap"]})
    with pytest.raises(ValueError, match="'relu' is not an nn.MaxPool2d"):
        convert_w8a8_pool(net, {"relu": None})
    with pytest.raises(ValueError, match="per-tensor"):
        convert_w8a8_pool(net, {"avgpool": net.stem.weight_fake_quant})
