"""The elementwise ops on 8-bit levels (include/lsq_hip_eltwise_w8.h), everything that needs no GPU: the library's exports against
its header and `_abi.py`, its kernel set and their resources, the plans on both sides of every threshold, every refusal, and the
CPU path of the ops -- the definition the GPU tests compare against -- held to the existing ops composed and to an independent
numpy restatement, bit for bit, with `lsq_act_table`, the modules and the converter on top.  No tolerance anywhere.
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

import eltwise_w8_cases as C
import requant_w8_cases as R
from helpers import LLVM, demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_eltwise_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_eltwise_w8.so")
NAMES = sorted(["lsq_eltwise_w8_abi_version", "lsq_eltwise_w8_last_error", "lsq_eltwise_w8_lut", "lsq_eltwise_w8_mul_gate",
                "lsq_eltwise_w8_plan_lut", "lsq_eltwise_w8_plan_mul"])
LSQ_EINVAL = -1
CL = torch.channels_last
OPS = torch.ops.torchlsq
one = C.one


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    return [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(const void\*|int64_t)", "", decl.strip()).split(",") if f.strip()]


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_eltwise_w8_\w+)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_ELTWISE_W8) == NAMES and len(NAMES) == 6
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_", "lsq_requant_", "lsq_resadd_",
                  "lsq_pool_", "lsq_dwconv_", "lsq_eltwise_"):
        assert other not in und, other
    assert E.eltwise_w8_library().lsq_eltwise_w8_abi_version() == E.ELTWISE_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_ELTWISE_W8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    assert _fields(text, "lsq_eltwise_w8_shape") == [f[0] for f in E.LsqEltwiseW8Shape._fields_] and ctypes.sizeof(E.LsqEltwiseW8Shape) == 4 * 8
    assert _fields(text, "lsq_eltwise_w8_mul") == [f[0] for f in E.LsqEltwiseW8Mul._fields_] and ctypes.sizeof(E.LsqEltwiseW8Mul) == 11 * 8


def test_kernels(tmp_path):
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    short = {}
    for sym, dm in names.items():
        m = re.match(r"^(?:void )?lsq::eltwise_w8_(lut_packets|lut_generic|mul_packets|mul_generic)_kernel(?:<([^>]*)>)?\(", dm)
        assert m, "not a kernel of this library: %s" % dm
        short[sym] = m.group(1) + "".join("_" + n for n in re.findall(r"\d+", re.sub(r"\(int\)", "", m.group(2) or "")))
    # lut_packets_<packets per lane>, mul_packets_<pixels per lane>
    assert sorted(short.values()) == ["lut_generic", "lut_packets_1", "lut_packets_2", "mul_generic", "mul_packets_1", "mul_packets_2",
                                      "mul_packets_4"]
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
        assert lds[sym] == (256 if short[sym].startswith("lut_packets") else 0), (sym, lds[sym])
        if "packets" in short[sym]:
            assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops, sym
        if short[sym].startswith("lut_packets"):
            # the table is looked up with byte reads of LDS, and every packet of the lane is loaded before the first lookup
            per = int(short[sym].rsplit("_", 1)[1])
            assert "ds_read_u8" in ops and ops.index("ds_read_u8") > [i for i, o in enumerate(ops) if o == "global_load_dwordx4"][per - 1], sym
        if short[sym].startswith("mul_packets"):
            # the gate packet and every pixel's packet are loaded before the first conversion of a byte
            pix = int(short[sym].rsplit("_", 1)[1])
            first = min(i for i, o in enumerate(ops) if o.startswith("v_cvt_f32_ubyte"))
            assert [i for i, o in enumerate(ops) if o == "global_load_dwordx4"][pix] < first, sym


def test_plans_without_a_gpu():
    from torchlsq import extension as E
    # the table op: packets if and only if the buffers are aligned and n >= 16; the n % 16 last bytes ride in the same launch
    for n, aligned in itertools.product((1, 15, 16, 17, 31, 32, 255, 256, 257, 4096, 4097, 4111), (True, False)):
        assert E.eltwise_w8_plan_lut(n, aligned) == C.expected_plan_lut(n, aligned), (n, aligned)
    assert E.eltwise_w8_plan_lut(15)["family"] == "generic" and E.eltwise_w8_plan_lut(16)["family"] == "packets"
    assert E.eltwise_w8_plan_lut(17) == dict(family="packets", grid=1, block=256, packets_per_lane=1, lds_bytes=256, packets=1, tail_bytes=1)
    # packets per lane: 2, halved while the grid holds fewer than 2 workgroups per compute unit (256 are assumed without a GPU):
    # 512 workgroups of 256 lanes of 2 packets of 16 bytes, on both sides
    edge = 512 * 256 * 2 * 16 - 2 * 256 * 16 + 16        # the smallest n with 512 workgroups at 2 packets per lane
    hi, lo = E.eltwise_w8_plan_lut(edge), E.eltwise_w8_plan_lut(edge - 16)
    assert (hi["packets_per_lane"], hi["grid"]) == (2, 512) and (lo["packets_per_lane"], lo["grid"]) == (1, 1022), (hi, lo)
    assert hi == C.expected_plan_lut(edge) and lo == C.expected_plan_lut(edge - 16)
    assert E.eltwise_w8_plan_lut(32 * 16 * 112 * 112) == dict(family="packets", grid=784, block=256, packets_per_lane=2, lds_bytes=256,
                                                               packets=401408, tail_bytes=0)
    assert E.eltwise_w8_plan_lut(1 << 30)["packets_per_lane"] == 2 and E.eltwise_w8_plan_lut((1 << 30) + 5)["tail_bytes"] == 5
    # the gate multiply: packets if and only if C % 16 == 0 and the buffers are aligned
    for Cn, aligned in itertools.product((3, 15, 16, 17, 20, 24, 32, 48), (True, False)):
        pl = E.eltwise_w8_plan_mul(2, Cn, 3, 5, aligned)
        assert pl == C.expected_plan_mul(2, Cn, 3, 5, aligned), (Cn, aligned, pl)
        assert pl["family"] == ("packets" if aligned and Cn % 16 == 0 else "generic")
    for g in C.GEOMETRIES:
        assert E.eltwise_w8_plan_mul(*g) == C.expected_plan_mul(*g), g
    # pixels per lane: never more than H W ...
    for hw, want in (((1, 1), 1), ((1, 2), 2), ((1, 3), 2), ((2, 2), 4), ((1, 5), 4)):
        assert E.eltwise_w8_plan_mul(1 << 16, 64, *hw)["pixels_per_lane"] == want, hw
    # ... and halved while the grid holds fewer than 512 workgroups: B images of 64 channels at 16 x 16 have 4 B / P workgroups
    for B, want in ((1, 1), (255, 1), (256, 2), (511, 2), (512, 4), (4096, 4)):
        pl = E.eltwise_w8_plan_mul(B, 64, 16, 16)
        assert pl["pixels_per_lane"] == want and pl == C.expected_plan_mul(B, 64, 16, 16), (B, pl)
    assert E.eltwise_w8_plan_mul(32, 96, 28, 28) == dict(family="packets", grid=588, block=256, pixels_per_lane=1, lds_bytes=0,
                                                         lanes_per_image=4704)
    assert E.eltwise_w8_plan_mul(4096, 64, 15, 15)["lanes_per_image"] == 4 * 57          # ceil(225 / 4) pixels steps


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.eltwise_w8_library()
    err = lib.lsq_eltwise_w8_last_error
    out = (ctypes.c_int32 * 8)()
    # the plans
    for n in (0, -1):
        assert lib.lsq_eltwise_w8_plan_lut(n, 1, ctypes.byref(out)) == LSQ_EINVAL and b"at least 1 byte" in err()
    assert lib.lsq_eltwise_w8_plan_lut(16, 1, None) == LSQ_EINVAL and b"NULL output" in err()
    assert lib.lsq_eltwise_w8_plan_lut((1 << 40) * 256, 0, ctypes.byref(out)) == LSQ_EINVAL and b"31-bit grid" in err()
    S = E.LsqEltwiseW8Shape
    assert lib.lsq_eltwise_w8_plan_mul(None, 1, ctypes.byref(out)) == LSQ_EINVAL and b"NULL shape" in err()
    assert lib.lsq_eltwise_w8_plan_mul(ctypes.byref(S(2, 16, 3, 5)), 1, None) == LSQ_EINVAL and b"NULL output" in err()
    for bad in ((0, 16, 3, 5), (2, 0, 3, 5), (2, 16, 0, 5), (2, 16, 3, -1)):
        assert lib.lsq_eltwise_w8_plan_mul(ctypes.byref(S(*bad)), 1, ctypes.byref(out)) == LSQ_EINVAL and b"at least 1" in err(), bad
    for bad in ((1 << 29, 16, 1, 1), (1, 1 << 29, 1, 1), (1, 16, 1 << 29, 1), (1, 16, 1, 1 << 29)):
        assert lib.lsq_eltwise_w8_plan_mul(ctypes.byref(S(*bad)), 1, ctypes.byref(out)) == LSQ_EINVAL and b"beyond 29 bits" in err(), bad
    assert lib.lsq_eltwise_w8_plan_mul(ctypes.byref(S((1 << 29) - 1, 16, 1, 1)), 1, ctypes.byref(out)) == 0
    big = (1 << 29) - 1
    assert lib.lsq_eltwise_w8_plan_mul(ctypes.byref(S(big, big, big, big)), 1, ctypes.byref(out)) == LSQ_EINVAL and b"64-bit offsets" in err()
    assert lib.lsq_eltwise_w8_plan_mul(ctypes.byref(S(1 << 20, 3, 1 << 10, 1 << 9)), 0, ctypes.byref(out)) == LSQ_EINVAL and b"31-bit grid" in err()
    # the table op: every refusal comes before anything is enqueued, so host memory will do for the pointers
    x = torch.zeros(1024, dtype=torch.uint8)
    y = torch.zeros(1024, dtype=torch.uint8)
    t = torch.zeros(256, dtype=torch.uint8)
    lut = lib.lsq_eltwise_w8_lut
    for args in ((None, t.data_ptr(), 16, y.data_ptr()), (x.data_ptr(), None, 16, y.data_ptr()), (x.data_ptr(), t.data_ptr(), 16, None)):
        assert lut(*args, None) == LSQ_EINVAL and b"NULL buffer" in err()
    for n in (0, -5):
        assert lut(x.data_ptr(), t.data_ptr(), n, y.data_ptr(), None) == LSQ_EINVAL and b"at least 1 byte" in err()
    for off in (0, 1, 511):
        assert lut(x.data_ptr(), t.data_ptr(), 512, x.data_ptr() + off, None) == LSQ_EINVAL and b"overlap x's" in err(), off
    assert lut(x.data_ptr() + 511, t.data_ptr(), 512, x.data_ptr(), None) == LSQ_EINVAL and b"overlap x's" in err()
    for off in (0, 15, -255):                            # the table's 256 bytes against y's 16
        assert lut(x.data_ptr(), y.data_ptr() + 16 + off, 16, y.data_ptr() + 16, None) == LSQ_EINVAL and b"overlap the table" in err(), off
    # the gate multiply
    lx, lg, yy = torch.zeros(2 * 16 * 15, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8), torch.zeros(2 * 16 * 15 * 4 + 16, dtype=torch.uint8)
    s, z = torch.ones(4), torch.zeros(4, dtype=torch.int32)

    def consts(**kw):
        base = dict(s_x=s.data_ptr(), zx=z.data_ptr(), s_g=s.data_ptr() + 4, zg=z.data_ptr() + 4, out_scale=s.data_ptr() + 8,
                    out_shift=s.data_ptr() + 12, quant_min=0, quant_max=255, type_min=0, type_max=255, mid_dtype=E.LSQ_F32)
        base.update(kw)
        return E.LsqEltwiseW8Mul(*[base[f[0]] for f in E.LsqEltwiseW8Mul._fields_])

    def call(c=None, xd=0, gd=0, xp=lx.data_ptr(), gp=lg.data_ptr(), yp=yy.data_ptr(), shape=(2, 16, 3, 5), no_consts=False, no_shape=False):
        c = consts() if c is None else c
        return lib.lsq_eltwise_w8_mul_gate(xd, xp, gd, gp, None if no_shape else ctypes.byref(S(*shape)),
                                           None if no_consts else ctypes.byref(c), yp, None)
    assert call(xd=2) == LSQ_EINVAL and b"x_dtype must be" in err()
    assert call(gd=-1) == LSQ_EINVAL and b"g_dtype must be" in err()
    assert call(no_shape=True) == LSQ_EINVAL and b"NULL shape" in err()
    assert call(no_consts=True) == LSQ_EINVAL and b"NULL constants" in err()
    assert call(shape=(2, 16, 0, 5)) == LSQ_EINVAL and b"at least 1" in err()
    assert call(shape=(2, 1 << 29, 1, 1)) == LSQ_EINVAL and b"beyond 29 bits" in err()
    for p in ("xp", "gp", "yp"):
        assert call(**{p: None}) == LSQ_EINVAL and b"NULL buffer" in err(), p
    assert call(consts(mid_dtype=E.LSQ_F64)) == LSQ_EINVAL and b"mid_dtype must be" in err()
    for f in ("s_x", "zx", "s_g", "zg"):
        assert call(consts(**{f: None})) == LSQ_EINVAL and b"NULL s_x, zx, s_g or zg" in err(), f
        assert call(consts(**{f: s.data_ptr() + 2})) == LSQ_EINVAL and b"element-aligned" in err(), f
    assert call(consts(out_scale=None)) == LSQ_EINVAL and b"come together" in err()
    assert call(consts(out_shift=None)) == LSQ_EINVAL and b"come together" in err()
    assert call(consts(out_shift=s.data_ptr() + 1)) == LSQ_EINVAL and b"element-aligned" in err()
    for rng in ((5, 4, 0, 255), (0, 255, 9, 8), (-1, 255, 0, 255), (0, 255, -128, 127), (-129, 0, -128, 127), (0, 256, 0, 255)):
        assert call(consts(quant_min=rng[0], quant_max=rng[1], type_min=rng[2], type_max=rng[3])) == LSQ_EINVAL and b"must lie within" in err(), rng
    for off in (0, 1, 479):
        assert call(yp=lx.data_ptr() + off) == LSQ_EINVAL and b"overlap x's" in err(), off
    assert call(xp=yy.data_ptr() + 479) == LSQ_EINVAL and b"overlap x's" in err()
    for off in (0, 31):
        assert call(gp=yy.data_ptr() + off) == LSQ_EINVAL and b"overlap the gate's" in err(), off
    floats = consts(out_scale=None, out_shift=None)
    assert call(floats, yp=yy.data_ptr() + 480 * 4 - 1, xp=yy.data_ptr() + 2000) == LSQ_EINVAL and b"overlap" in err()       # y is 4 bytes an element
    assert call(floats, yp=yy.data_ptr() + 2) == LSQ_EINVAL and b"element-aligned" in err()
    assert call(consts(out_scale=None, out_shift=None, mid_dtype=E.LSQ_BF16), yp=yy.data_ptr() + 1) == LSQ_EINVAL and b"element-aligned" in err()


def test_host_checks_of_the_ops():
    from torchlsq.functional import LevelsTensor, lsq_act_w8_q, lsq_lut_w8, lsq_mul_gate_w8, lsq_mul_gate_w8_q
    for name in ("lsq_lut_w8", "lsq_mul_gate_w8_q8_q", "lsq_mul_gate_w8_q8"):
        assert hasattr(OPS, name)
    x, t = C.lut_x(2 * 16 * 3 * 5).reshape(2, 16, 3, 5), C.perm_table()
    with pytest.raises(RuntimeError, match="uint8 .* or int8"):
        OPS.lsq_lut_w8(x.float(), t, torch.uint8)
    with pytest.raises(RuntimeError, match="256 entries"):
        OPS.lsq_lut_w8(x, t[:255], torch.uint8)
    with pytest.raises(RuntimeError, match="256 entries"):
        OPS.lsq_lut_w8(x, t.to(torch.int32), torch.uint8)
    with pytest.raises(RuntimeError, match="out_dtype must be"):
        OPS.lsq_lut_w8(x, t, torch.float32)
    # the table op keeps x's shape and memory layout, whatever it is; int8 in and out are the same bytes
    for xv in (x, x.contiguous(memory_format=CL), x[:, :, 1:], x.flatten(), x[:0]):
        for dt in C.LEVEL_DTYPES:
            y = OPS.lsq_lut_w8(xv.view(dt), t.view(torch.int8), dt)
            assert y.dtype == dt and y.shape == xv.shape and torch.equal(y.view(torch.uint8), t[xv.long()])
            assert y.is_contiguous() == xv.is_contiguous() or not (xv.is_contiguous() or xv.is_contiguous(memory_format=CL))
    c = C.mul_case((2, 16, 3, 5), C.VARIANTS[0], (True, torch.float32))
    lx, s_x, zx, lg, s_g, zg, osc, osh, rng, mid = c
    ops = (lx, s_x, zx, lg, s_g, zg)
    with pytest.raises(RuntimeError, match="x_levels must be uint8"):
        OPS.lsq_mul_gate_w8_q8(lx.float(), *ops[1:], torch.float32)
    with pytest.raises(RuntimeError, match="g_levels must be uint8"):
        OPS.lsq_mul_gate_w8_q8(lx, s_x, zx, lg.float(), s_g, zg, torch.float32)
    with pytest.raises(RuntimeError, match="one float32 value"):
        OPS.lsq_mul_gate_w8_q8(lx, s_x.double(), *ops[2:], torch.float32)
    with pytest.raises(RuntimeError, match="one float32 value"):
        OPS.lsq_mul_gate_w8_q8(lx, s_x, zx, lg, s_g, zg.long(), torch.float32)
    with pytest.raises(RuntimeError, match=r"\[B, C, H, W\] or a \[B, C\]"):
        OPS.lsq_mul_gate_w8_q8(lx[0], *ops[1:], torch.float32)
    with pytest.raises(RuntimeError, match="the gate must be"):
        OPS.lsq_mul_gate_w8_q8(lx, s_x, zx, lg[:1], s_g, zg, torch.float32)
    with pytest.raises(RuntimeError, match="the gate must be"):
        OPS.lsq_mul_gate_w8_q8(lx, s_x, zx, lg.expand(2, 16, 3, 5), s_g, zg, torch.float32)
    with pytest.raises(RuntimeError, match="out_dtype must be"):
        OPS.lsq_mul_gate_w8_q8(*ops, torch.float64)
    with pytest.raises(RuntimeError, match="mid_dtype must be"):
        OPS.lsq_mul_gate_w8_q8_q(*ops, osc, osh, *rng, torch.float64)
    with pytest.raises(RuntimeError, match="must lie within"):
        OPS.lsq_mul_gate_w8_q8_q(*ops, osc, osh, -1, 255, 0, 255, torch.float32)
    with pytest.raises(RuntimeError, match="float32 tensors of one value"):
        OPS.lsq_mul_gate_w8_q8_q(*ops, osc.repeat(2), osh, *rng, torch.float32)
    with pytest.raises(RuntimeError, match="inference-only"):
        OPS.lsq_mul_gate_w8_q8_q(*ops, osc.clone().requires_grad_(True), osh, *rng, torch.float32)
    with pytest.raises(RuntimeError, match="inference-only"):
        OPS.lsq_mul_gate_w8_q8(lx, s_x.clone().requires_grad_(True), *ops[2:], torch.float32)
    # the gate as [B, C] or [B, C, 1, 1]; an NCHW x is copied to channels-last first; an empty batch
    want = C.run(c)
    assert want.is_contiguous(memory_format=CL) and torch.equal(OPS.lsq_mul_gate_w8_q8_q(lx, s_x, zx, lg.reshape(2, 16), s_g, zg, osc, osh, *rng, mid), want)
    assert not lx.contiguous().is_contiguous(memory_format=CL)
    assert torch.equal(OPS.lsq_mul_gate_w8_q8_q(lx.contiguous(), *ops[1:], osc, osh, *rng, mid), want)
    assert OPS.lsq_mul_gate_w8_q8_q(lx[:0], s_x, zx, lg[:0], s_g, zg, osc, osh, *rng, mid).shape == (0, 16, 3, 5)
    assert OPS.lsq_mul_gate_w8_q8(lx[:0], s_x, zx, lg[:0], s_g, zg, torch.bfloat16).dtype == torch.bfloat16
    # the functional entry points
    X, G = LevelsTensor(lx, s_x, zx, 0, 255), LevelsTensor(lg, s_g, zg, 0, 255)
    got = lsq_mul_gate_w8_q(X, G, osc, osh, 0, 255, mid_dtype=mid)
    assert isinstance(got, LevelsTensor) and torch.equal(got.levels, want) and got.scale.dtype == torch.float32
    assert torch.equal(lsq_mul_gate_w8_q(X, LevelsTensor(lg.reshape(2, 16), s_g, zg, 0, 255), osc, osh, 0, 255, mid_dtype=mid).levels, want)
    xq = torch._make_per_tensor_quantized_tensor(lx, float(s_x), int(zx))
    assert torch.equal(lsq_mul_gate_w8_q(xq, G, osc, osh, 0, 255, mid_dtype=mid).levels, want)
    f = lsq_mul_gate_w8(X, G, torch.bfloat16)
    assert f.dtype == torch.bfloat16 and torch.equal(C.bits(f), C.bits(OPS.lsq_mul_gate_w8_q8(*ops, torch.bfloat16)))
    with pytest.raises(AssertionError, match="out_scale"):
        lsq_mul_gate_w8_q(X, G)
    with pytest.raises(AssertionError, match="a gate of"):
        lsq_mul_gate_w8_q(X, X, osc, osh, 0, 255)
    with pytest.raises(AssertionError, match="LevelsTensor"):
        lsq_mul_gate_w8(lx, G)
    # lsq_lut_w8 / lsq_act_w8_q: a LevelsTensor of the output quantizer; the unfused chain on the same device, bit for bit
    o_s, o_b = one(0.03), one(-0.4)
    r = lsq_act_w8_q(X, "hardswish", o_s, o_b, -128, 127, mid_dtype=torch.bfloat16)
    chain = OPS.lsq_levels_per_tensor(F.hardswish(X.dequantize(torch.bfloat16)), o_s, o_b, -128, 127, -128, 127, 0)
    assert isinstance(r, LevelsTensor) and r.levels.dtype == torch.int8 and torch.equal(r.levels, chain) and r.levels.is_contiguous(memory_format=CL)
    assert (r.quant_min, r.quant_max) == (-128, 127) and len(r.levels.unique()) > 32
    assert torch.equal(lsq_lut_w8(X, C.perm_table(), o_s, o_b, 0, 255).levels, C.perm_table()[lx.long()])
    with pytest.raises(AssertionError, match="unknown activation"):
        lsq_act_w8_q(X, "softmax", o_s, o_b, 0, 255)
    with pytest.raises(AssertionError, match="must return a bfloat16 tensor"):
        lsq_act_w8_q(X, lambda v: v.float(), o_s, o_b, 0, 255, mid_dtype=torch.bfloat16)
    # the fake kernels: shapes, dtypes and the memory format of the real ones
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        fa = [mode.from_tensor(v) for v in ops]
        q = OPS.lsq_mul_gate_w8_q8_q(*fa, mode.from_tensor(osc), mode.from_tensor(osh), -128, 127, -128, 127, torch.float32)
        fl = OPS.lsq_mul_gate_w8_q8(*fa, torch.float16)
        ft = OPS.lsq_lut_w8(fa[0], mode.from_tensor(t), torch.int8)
    assert (q.shape, q.dtype) == ((2, 16, 3, 5), torch.int8) and q.is_contiguous(memory_format=CL)
    assert (fl.shape, fl.dtype) == ((2, 16, 3, 5), torch.float16) and fl.is_contiguous(memory_format=CL)
    assert (ft.shape, ft.dtype, ft.stride()) == ((2, 16, 3, 5), torch.int8, lx.stride())


# ---------------------------------------------------------------------------------------------------
# lsq_act_table
# ---------------------------------------------------------------------------------------------------
TORCH_FNS = {"identity": lambda v: v, "relu": F.relu, "relu6": F.relu6, "hardtanh": F.hardtanh, "leaky_relu": F.leaky_relu,
             "hardswish": F.hardswish, "hardsigmoid": F.hardsigmoid, "silu": F.silu, "gelu": F.gelu,
             "gelu_tanh": lambda v: F.gelu(v, approximate="tanh"), "sigmoid": torch.sigmoid, "tanh": torch.tanh}


@pytest.mark.parametrize("mid", C.MIDS, ids=C.name)
@pytest.mark.parametrize("fn", C.NAMED)
def test_act_table_is_its_definition_written_out(fn, mid):
    """the 256 bytes as in_dtype -> (float32 subtract, float32 multiply, rounding to mid) -> the torch function in mid -> level()
    restated in np.float32 steps; u8 / i8 on both sides"""
    from torchlsq.functional import lsq_act_table
    assert sorted(TORCH_FNS) == sorted(C.NAMED)
    for in_dtype, unsigned in itertools.product(C.LEVEL_DTYPES, (True, False)):
        s, z = one(0.047), one(131 if in_dtype == torch.uint8 else 3, torch.int32)
        rng = (0, 255, 0, 255) if unsigned else (-128, 127, -128, 127)
        osc, osh = one(0.021), one(-2.0 if unsigned else 0.4)
        table = lsq_act_table(fn, s, z, in_dtype, osc, osh, *rng[:2], mid_dtype=mid)
        assert table.dtype == torch.uint8 and table.shape == (256,)
        b = np.arange(256, dtype=np.uint8).view(np.uint8 if in_dtype == torch.uint8 else np.int8)
        u = C.round_to((b.astype(np.float32) - np.float32(int(z))) * np.float32(float(s)), mid)
        v = TORCH_FNS[fn](torch.from_numpy(u).to(mid))
        assert v.dtype == mid
        want = C.numpy_levels(v.float().numpy(), osc, osh, rng)
        assert torch.equal(table.view(torch.uint8 if unsigned else torch.int8).to(torch.int64), torch.from_numpy(want)), (fn, in_dtype, unsigned)
        assert len(table.unique()) > (8 if fn in ("hardtanh", "tanh", "sigmoid", "hardsigmoid") else 32), (fn, len(table.unique()))
        # the nn module of the function gives the same table, and the table op the unfused chain on any levels
        mod = {"identity": torch.nn.Identity(), "relu": torch.nn.ReLU(), "relu6": torch.nn.ReLU6(), "hardtanh": torch.nn.Hardtanh(),
               "leaky_relu": torch.nn.LeakyReLU(), "hardswish": torch.nn.Hardswish(), "hardsigmoid": torch.nn.Hardsigmoid(),
               "silu": torch.nn.SiLU(), "gelu": torch.nn.GELU(), "gelu_tanh": torch.nn.GELU(approximate="tanh"),
               "sigmoid": torch.nn.Sigmoid(), "tanh": torch.nn.Tanh()}[fn]
        assert torch.equal(lsq_act_table(mod, s, z, in_dtype, osc, osh, *rng[:2], mid_dtype=mid), table)


def test_act_table_of_a_parametrised_module_and_of_a_callable():
    from torchlsq.functional import act_function, lsq_act_table
    s, z, osc, osh = one(0.05), one(128, torch.int32), one(0.01), one(-1.28)
    args = (s, z, torch.uint8, osc, osh, 0, 255)
    assert torch.equal(lsq_act_table(torch.nn.Hardtanh(-0.5, 0.75), *args), lsq_act_table(lambda v: v.clamp(-0.5, 0.75), *args))
    assert not torch.equal(lsq_act_table(torch.nn.Hardtanh(-0.5, 0.75), *args), lsq_act_table("hardtanh", *args))
    assert torch.equal(lsq_act_table(torch.nn.LeakyReLU(0.2), *args), lsq_act_table(lambda v: F.leaky_relu(v, 0.2), *args))
    assert not torch.equal(lsq_act_table(torch.nn.LeakyReLU(0.2), *args), lsq_act_table("leaky_relu", *args))
    assert act_function(torch.nn.Hardtanh(-0.5, 0.75))[1] == "hardtanh(-0.5, 0.75)" and act_function(torch.nn.ReLU6())[1] == "relu6"
    assert act_function(None) == (None, "identity") and act_function(torch.nn.GELU(approximate="tanh"))[1] == "gelu_tanh"
    assert torch.equal(lsq_act_table(None, *args), lsq_act_table("identity", *args))


@pytest.mark.parametrize("dtype", C.LEVEL_DTYPES, ids=C.name)
def test_identity_table_to_the_same_quantizer_is_the_identity_on_the_range(dtype):
    """requantizing to the quantizer the levels came from gives the levels back, for every mid that holds them exactly"""
    from torchlsq._qlinear_a8_host import _act_constants
    from torchlsq.functional import lsq_act_table
    lo, hi = (0, 255) if dtype == torch.uint8 else (-128, 127)
    for qmin, qmax in ((lo, hi), (lo + 3, hi - 55)):
        for scale, zp in ((0.0371, lo + 3), (0.5, lo + 128), (1.0 / 255, lo)):
            osc, osh = one(scale), one(-zp * scale)
            s, z = _act_constants(osc, osh, lo, hi)
            assert int(z) == zp
            for mid in (torch.float32,):
                table = lsq_act_table(None, s, z, dtype, osc, osh, qmin, qmax, lo, hi, mid_dtype=mid).view(dtype).to(torch.int64)
                levels = torch.arange(lo, hi + 1)
                got = table[levels & 0xff]
                assert torch.equal(got[qmin - lo:qmax - lo + 1], levels[qmin - lo:qmax - lo + 1]), (qmin, qmax, scale, zp)
                assert bool((got[:qmin - lo] == qmin).all()) and bool((got[qmax - lo + 1:] == qmax).all())        # never read: clamped


# ---------------------------------------------------------------------------------------------------
# the gate multiply
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", C.VARIANTS, ids=C.variant_id)
@pytest.mark.parametrize("geometry", C.GEOMETRIES, ids=C.geom_id)
def test_cpu_path_is_the_existing_ops_composed_and_the_numpy_restatement(geometry, variant):
    """every mid, levels out (both types) and floats out: torch.equal on the bits, against `dequantize`, `torch.mul` and
    `lsq_levels_per_tensor` composed and against np.float32 steps with explicit roundings to mid"""
    stats = []
    for out_variant in C.OUT_VARIANTS:
        c = C.mul_case(geometry, variant, out_variant, 5)
        lx, s_x, zx, lg, s_g, zg, osc, osh, rng, mid = c
        got, want = C.run(c), C.composed(c)
        assert got.dtype == want.dtype and got.shape == want.shape == lx.shape
        assert got.is_contiguous(memory_format=CL) if lx.dim() == 4 else got.is_contiguous()
        assert torch.equal(C.bits(got), C.bits(want)), (geometry, variant, out_variant)
        t = C.numpy_value(lx, s_x, zx, lg, s_g, zg, mid)
        if rng is None:
            assert got.dtype == mid and torch.equal(C.bits(got), C.bits(torch.from_numpy(t).to(mid)))
        else:
            assert got.dtype == (torch.uint8 if out_variant[0] else torch.int8)
            assert torch.equal(got.to(torch.int64), torch.from_numpy(C.numpy_levels(t, osc, osh, rng))), (geometry, variant, out_variant)
            if got.numel() >= 1000:
                stats.append(C.assert_conditions(got, c, (geometry, variant, out_variant)))
    if stats:
        print("non-vacuity %s %s: inside %.2f-%.2f, channel roll %.2f-%.2f, image roll %.2f-%.2f" % (
            C.geom_id(geometry), C.variant_id(variant), min(s[0] for s in stats), max(s[0] for s in stats), min(s[1] for s in stats),
            max(s[1] for s in stats), min(s[2] for s in stats), max(s[2] for s in stats)))


# Found by a search over all 256 x 256 pairs of levels on the CPU (s_x = 0.3, s_g = 0.01, both zero points 128, output scale 0.03
# and zero point 128, mid float32): pairs (lx, lg) whose level changes when (1) the product is formed in double precision from
# operands that were never rounded to float32, or (2) the exact product a g is carried into the output quantizer's multiply-add
# without its own rounding, as a contracted a * g * inv_s + zp would.  The definition rounds a, g and a g to float32 one by one.
NO_FMA = dict(s_x=0.3, s_g=0.01, zx=128, zg=128, out_scale=0.03, out_shift=-128 * 0.03)
DOUBLE_PRODUCT_DIFFERS = [(3, 137), (15, 133), (33, 117), (45, 113), (49, 143), (53, 139)]
CONTRACTED_DIFFERS = [(3, 137), (11, 133), (23, 119), (23, 133), (33, 121), (43, 115)]


def test_the_product_is_rounded_on_its_own_never_contracted():
    f, d = np.float32, np.float64
    k = NO_FMA
    lx = torch.arange(256, dtype=torch.uint8).reshape(256, 1).repeat(1, 256).contiguous()
    lg = torch.arange(256, dtype=torch.uint8).reshape(1, 256).repeat(256, 1).contiguous()
    osc, osh, rng = one(k["out_scale"]), one(k["out_shift"]), (0, 255, 0, 255)
    got = OPS.lsq_mul_gate_w8_q8_q(lx, one(k["s_x"]), one(k["zx"], torch.int32), lg, one(k["s_g"]), one(k["zg"], torch.int32), osc, osh,
                                   *rng, torch.float32).to(torch.int64).numpy()
    a = (lx.numpy().astype(f) - f(k["zx"])) * f(k["s_x"])
    g = (lg.numpy().astype(f) - f(k["zg"])) * f(k["s_g"])
    want = C.numpy_levels((a * g).astype(f), osc, osh, rng)
    assert np.array_equal(got, want)
    inv, zp = f(1.0) / f(k["out_scale"]), f(128)
    assert zp == np.rint(-f(k["out_shift"]) * inv)
    double_product = ((lx.numpy().astype(d) - k["zx"]) * d(f(k["s_x"]))) * ((lg.numpy().astype(d) - k["zg"]) * d(f(k["s_g"])))
    wrong1 = C.numpy_levels(double_product.astype(f), osc, osh, rng)
    contracted = (a.astype(d) * g.astype(d) * d(inv) + d(zp)).astype(f)
    wrong2 = np.rint(np.minimum(f(255), np.maximum(f(0), contracted))).astype(np.int64)
    inside = (want > 0) & (want < 255)
    assert int(((wrong1 != want) & inside).sum()) >= 50 and int(((wrong2 != want) & inside).sum()) >= 50
    for i, j in DOUBLE_PRODUCT_DIFFERS:
        assert wrong1[i, j] != want[i, j] == got[i, j] and abs(int(wrong1[i, j]) - int(want[i, j])) == 1, (i, j)
    for i, j in CONTRACTED_DIFFERS:
        assert wrong2[i, j] != want[i, j] == got[i, j] and abs(int(wrong2[i, j]) - int(want[i, j])) == 1, (i, j)


def test_a_nan_goes_to_quant_min_and_stays_a_nan_in_the_floats():
    c = C.mul_case((2, 16, 3, 5), C.VARIANTS[0], (True, torch.float32))
    lx, s_x, zx, lg, s_g, zg, osc, osh, _, _ = c
    nan, inf = one(float("nan")), one(float("inf"))
    for mid in C.MIDS:
        for sx, sg in ((nan, s_g), (s_x, nan)):
            f = OPS.lsq_mul_gate_w8_q8(lx, sx, zx, lg, sg, zg, mid)
            assert f.dtype == mid and bool(f.isnan().all())
            for rng in ((3, 200, 0, 255), (-100, 100, -128, 127)):
                q = OPS.lsq_mul_gate_w8_q8_q(lx, sx, zx, lg, sg, zg, one(0.5), one(0.0), *rng, mid)
                assert bool((q.to(torch.int64) == rng[0]).all())
        # inf * 0 is a NaN too: the gate level on its zero point
        g0 = torch.full_like(lg, 7)
        q = OPS.lsq_mul_gate_w8_q8_q(lx, inf, zx, g0, s_g, one(7, torch.int32), one(0.5), one(0.0), 3, 200, 0, 255, mid)
        live = lx != int(zx)
        assert bool((q[live] == 3).all())
    # a NaN output scale: the sanitised scale keeps it, every level is quant_min
    q = OPS.lsq_mul_gate_w8_q8_q(lx, s_x, zx, lg, s_g, zg, nan, osh, 5, 250, 0, 255, torch.float32)
    assert bool((q == 5).all())


# ---------------------------------------------------------------------------------------------------
# the modules and the converter
# ---------------------------------------------------------------------------------------------------
def test_state_dict_round_trips():
    from torchlsq.functional import LevelsTensor, lsq_act_table
    from torchlsq.quantized import ActivationW8Q, MulGateW8Q
    net, qs, x = C.v3_block()
    with torch.no_grad():
        e = net.expand[0](qs["in"](x))
    el = LevelsTensor.from_quantized(qs["e"].quantize(e))
    m = ActivationW8Q.from_float(net.expand[1], qs["e"], qs["h"], mid_dtype=torch.bfloat16)
    assert {"table", "output_scale", "output_shift"} == set(dict(m.named_buffers()))
    assert m.table.dtype == torch.uint8 and m.table.shape == (256,) and len(m.table.unique()) > 32
    fresh = ActivationW8Q()
    assert torch.equal(fresh.table, torch.arange(256, dtype=torch.uint8))
    fresh.load_state_dict(m.state_dict())
    assert (fresh.function, fresh.mid_dtype, fresh.output_range) == ("hardswish", torch.bfloat16, m.output_range) and torch.equal(fresh.table, m.table)
    assert "hardswish" in repr(fresh) and "output levels" in repr(fresh) and "mid_dtype=bfloat16" in repr(fresh)
    want = m(el)
    assert isinstance(want, LevelsTensor) and torch.equal(fresh(el).levels, want.levels) and len(want.levels.unique()) > 32
    assert want.levels.shape == el.shape and want.levels.stride() == el.levels.stride()
    # the module's output is the unfused chain's on the same levels, bit for bit
    with torch.no_grad():
        chain = qs["h"].quantize(F.hardswish(el.dequantize(torch.bfloat16))).int_repr()
    assert torch.equal(want.levels, chain)
    from torchlsq.quantized.modules.packed_linear_a8 import _per_tensor_constants
    osc, osh, *rng = _per_tensor_constants(qs["h"], "h")
    assert torch.equal(m.table, lsq_act_table("hardswish", el.scale, el.zero_point, torch.uint8, osc, osh, *rng, mid_dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="LSQFakeQuantizer"):
        ActivationW8Q.from_float("relu", None, qs["h"])
    with pytest.raises(ValueError, match="LSQFakeQuantizer"):
        ActivationW8Q.from_float("relu", qs["e"], None)
    # the gate multiply
    g = MulGateW8Q.from_float(net.se.skip_mul, mid_dtype=torch.float16)
    assert {"output_scale", "output_shift"} == set(dict(g.named_buffers()))
    fresh = MulGateW8Q()
    fresh.load_state_dict(g.state_dict())
    assert (fresh.mid_dtype, fresh.output_range) == (torch.float16, g.output_range) and torch.equal(fresh.output_scale, qs["mul"].scale.detach())
    c = C.mul_case((2, 48, 7, 7), C.VARIANTS[0], (None, torch.float16))
    X, G = LevelsTensor(c[0], c[1], c[2], 0, 255), LevelsTensor(c[3], c[4], c[5], 0, 255)
    want = g(X, G)
    assert isinstance(want, LevelsTensor) and want.levels.shape == (2, 48, 7, 7) and len(want.levels.unique()) > 16
    for got in (fresh(X, G), fresh.mul(X, G), fresh.mul(G, X), fresh.mul(LevelsTensor(c[3].reshape(2, 48), c[4], c[5], 0, 255), X)):
        assert torch.equal(got.levels, want.levels)
    assert torch.equal(want.levels, OPS.lsq_mul_gate_w8_q8_q(*c[:6], g.output_scale, g.output_shift, *g.output_range, torch.float16))
    with pytest.raises(ValueError, match="its gate of"):
        fresh.mul(X, X)
    with pytest.raises(TypeError, match="two LevelsTensors"):
        fresh.mul(X, c[3])
    with pytest.raises(ValueError, match="LSQFakeQuantizer"):
        MulGateW8Q.from_float(torch.ao.nn.quantized.FloatFunctional())


@pytest.mark.parametrize("mid", R.MIDS, ids=C.name)
def test_convert_w8a8_eltwise_on_a_mobilenet_v3_block_equals_the_modules_written_out(mid):
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import (ActivationW8Q, AdaptiveAvgPool2dW8Q, AddW8A8Q, Conv2dW8A8AddQ, Conv2dW8A8Q, DepthwiseConv2dW8A8Q,
                                    MulGateW8Q, convert_w8a8_eltwise)
    net, qs, x = C.v3_block()
    new = C.convert_v3_block(net, qs, mid)
    assert isinstance(new.expand[0], Conv2dW8A8Q) and isinstance(new.expand[1], ActivationW8Q) and new.expand[1].function == "hardswish"
    assert isinstance(new.depthwise[0], DepthwiseConv2dW8A8Q) and isinstance(new.depthwise[1], ActivationW8Q)
    assert isinstance(new.se.avgpool, AdaptiveAvgPool2dW8Q) and isinstance(new.se.fc1[0], Conv2dW8A8Q) and isinstance(new.se.fc1[1], torch.nn.Identity)
    assert isinstance(new.se.scale_activation, ActivationW8Q) and new.se.scale_activation.function == "hardsigmoid"
    assert isinstance(new.se.skip_mul, MulGateW8Q) and isinstance(new.project, Conv2dW8A8AddQ) and isinstance(new.add, AddW8A8Q)
    assert new.se.skip_mul.mid_dtype == new.expand[1].mid_dtype == mid
    assert isinstance(net.expand[1], torch.nn.Hardswish) and hasattr(net.se.skip_mul, "activation_post_process")      # a deep copy
    xl = LevelsTensor.from_quantized(qs["in"].quantize(x))
    got = new(xl)                                                                            # the block's and the SE block's own forward
    want, mids = C.v3_block_written_out(net, qs, xl, mid)
    assert isinstance(got, LevelsTensor) and got.levels.shape == (2, 16, 9, 7) and torch.equal(got.levels, want.levels)
    assert len(want.levels.unique()) > 64 and all(len(v.levels.unique()) > 16 for v in mids.values()), {k: len(v.levels.unique()) for k, v in mids.items()}
    assert mids["gate"].levels.shape == (2, 48, 1, 1) and mids["mul"].levels.shape == (2, 48, 9, 7)
    # each new step gives the levels of the unfused float composition on the same input levels, bit for bit
    with torch.no_grad():
        for src, dst, fn in (("e", "h", F.hardswish), ("d", "da", F.hardswish), ("f2", "gate", F.hardsigmoid)):
            chain = qs[dst].quantize(fn(mids[src].dequantize(mid))).int_repr()
            assert torch.equal(mids[dst].levels, chain), (src, dst)
        prod = qs["mul"].quantize(mids["gate"].dequantize(mid) * mids["da"].dequantize(mid)).int_repr()
        assert torch.equal(mids["mul"].levels, prod)
        # and the whole block is within one level of the QAT block in float
        ref = net.add.activation_post_process.quantize(net(qs["in"](x))).int_repr()
    close = (ref.to(torch.int64) - got.levels.to(torch.int64)).abs()
    assert int(close.max()) <= 1 and float((close == 0).double().mean()) > 0.9
    # refusals of the converter, by name
    with pytest.raises(ValueError, match="'expand.0' is not an activation module"):
        convert_w8a8_eltwise(net, {"expand.0": (qs["in"], qs["e"])})
    with pytest.raises(ValueError, match="'nowhere' is not an activation module"):
        convert_w8a8_eltwise(net, {"nowhere": (qs["in"], qs["e"])})
    with pytest.raises(ValueError, match="'expand.1' needs the pair"):
        convert_w8a8_eltwise(net, {"expand.1": qs["e"]})
    with pytest.raises(ValueError, match="'project' is not a FloatFunctional"):
        convert_w8a8_eltwise(net, muls={"project": qs["mul"]})
    with pytest.raises(ValueError, match="LSQFakeQuantizer"):
        convert_w8a8_eltwise(net, muls={"add": torch.nn.Identity()})
    only = convert_w8a8_eltwise(net, {"depthwise.1": (qs["d"], qs["da"])}, mid_dtype=mid)
    assert isinstance(only.depthwise[1], ActivationW8Q) and isinstance(only.expand[1], torch.nn.Hardswish) and \
        isinstance(only.se.skip_mul, torch.ao.nn.quantized.FloatFunctional)
