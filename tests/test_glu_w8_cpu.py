"""The gated product act(gate) * up on 8-bit levels (include/lsq_hip_glu_w8.h), everything that needs no GPU: the library's exports
against its header and `_abi.py`, its kernel set and their resources, the plan on both sides of every threshold, every refusal, and
the CPU path of the ops -- the definition the GPU tests compare against -- held to the two compositions of existing ops and to an
independent numpy restatement, bit for bit, with `lsq_glu_table`, the modules and the converter on top.  No tolerance anywhere.
"""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import glu_w8_cases as C
from helpers import LLVM, demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_glu_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_glu_w8.so")
NAMES = sorted(["lsq_glu_w8_abi_version", "lsq_glu_w8_last_error", "lsq_glu_w8", "lsq_glu_w8_plan"])
LSQ_EINVAL = -1
OPS = torch.ops.torchlsq
one = C.one


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    return [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(const void\*|int64_t)", "", decl.strip()).split(",") if f.strip()]


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_glu_w8\w*)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_GLU_W8) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    # it imports no symbol of the other libraries and reads no environment variable
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und and not re.search(r"\blsq_", und), und
    assert E.glu_w8_library().lsq_glu_w8_abi_version() == E.GLU_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_GLU_W8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    assert _fields(text, "lsq_glu_w8_shape") == [f[0] for f in E.LsqGluW8Shape._fields_] and ctypes.sizeof(E.LsqGluW8Shape) == 4 * 8
    assert _fields(text, "lsq_glu_w8_consts") == [f[0] for f in E.LsqGluW8Consts._fields_] and ctypes.sizeof(E.LsqGluW8Consts) == 9 * 8


def test_kernels(tmp_path):
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    short = {}
    for sym, dm in names.items():
        m = re.match(r"^(?:void )?lsq::glu_w8_(packets|generic)_kernel(?:<([^>]*)>)?\(", dm)
        assert m, "not a kernel of this library: %s" % dm
        short[sym] = m.group(1) + "".join("_" + n for n in re.findall(r"\d+", re.sub(r"\(int\)", "", m.group(2) or "")))
    assert sorted(short.values()) == ["generic", "packets_1", "packets_2"]          # packets_<packet positions per lane>
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
        assert lds[sym] == (1024 if short[sym].startswith("packets") else 0), (sym, lds[sym])
        assert not any(o.startswith(("global_atomic", "flat_atomic", "ds_add", "ds_cmpst")) for o in ops), sym      # no atomics
        if short[sym].startswith("packets"):
            # a gate and an up packet per position, every one of them loaded before the first lookup; the table is read from LDS in
            # 4-byte reads; one 16-byte store per position (levels out)
            per = int(short[sym].rsplit("_", 1)[1])
            loads = [i for i, o in enumerate(ops) if o == "global_load_dwordx4"]
            assert len(loads) == 2 * per and "global_store_dwordx4" in ops, sym
            assert "ds_read_b32" in ops and ops.index("ds_read_b32") > loads[-1], sym
            assert ops.count("ds_read_b32") == 16 * per, sym


def test_plan_without_a_gpu():
    from torchlsq import extension as E
    # packets if and only if C % 16 == 0, both row strides % 16 == 0 and the buffers are aligned (256 CUs are assumed without a GPU)
    for Cn, aligned in itertools.product((1, 15, 16, 17, 32, 48, 272), (True, False)):
        for gs, us in ((Cn, Cn), (2 * Cn, 2 * Cn), (2 * Cn + 16, 2 * Cn + 16), (Cn + 8, Cn), (Cn, Cn + 1)):
            pl = E.glu_w8_plan(3, Cn, gs, us, aligned)
            assert pl == C.expected_plan(3, Cn, gs, us, aligned), (Cn, gs, us, aligned, pl)
            assert pl["family"] == ("packets" if aligned and Cn % 16 == 0 and gs % 16 == 0 and us % 16 == 0 else "generic")
    assert E.glu_w8_plan(1, 16) == dict(family="packets", grid=1, block=256, packets_per_lane=1, lds_bytes=1024, packets=1)
    assert E.glu_w8_plan(1, 15) == dict(family="generic", grid=1, block=256, packets_per_lane=1, lds_bytes=0, packets=0)
    assert E.glu_w8_plan(17, 15)["grid"] == 1 and E.glu_w8_plan(18, 15)["grid"] == 2          # 255 and 270 elements
    # packets per lane: 2, halved while the grid holds fewer than 2 workgroups per compute unit: 512 workgroups of 256 lanes of 2
    # packets, on both sides
    edge = 512 * 256 * 2 - 2 * 256 + 1               # the fewest packets with 512 workgroups at 2 packets per lane
    hi, lo = E.glu_w8_plan(edge, 16), E.glu_w8_plan(edge - 1, 16)
    assert (hi["packets_per_lane"], hi["grid"]) == (2, 512) and (lo["packets_per_lane"], lo["grid"]) == (1, 1022), (hi, lo)
    assert hi == C.expected_plan(edge, 16) and lo == C.expected_plan(edge - 1, 16)
    assert E.glu_w8_plan(2048, 14336, 28672, 28672) == dict(family="packets", grid=3584, block=256, packets_per_lane=2, lds_bytes=1024,
                                                           packets=2048 * 896)
    assert E.glu_w8_plan(16, 11008, 22016, 22016) == C.expected_plan(16, 11008, 22016, 22016)
    assert E.glu_w8_plan(16, 11008, 22016, 22016)["packets_per_lane"] == 1


def test_argument_validation_without_a_gpu():
    """every refusal of the C ABI; they all come before anything is enqueued, so host memory will do for the pointers"""
    from torchlsq import extension as E
    lib = E.glu_w8_library()
    err = lib.lsq_glu_w8_last_error
    out = (ctypes.c_int32 * 8)()
    S = E.LsqGluW8Shape
    plan = lib.lsq_glu_w8_plan
    assert plan(None, 1, ctypes.byref(out)) == LSQ_EINVAL and b"NULL shape" in err()
    assert plan(ctypes.byref(S(3, 16, 16, 16)), 1, None) == LSQ_EINVAL and b"NULL output" in err()
    for bad in ((0, 16, 16, 16), (3, 0, 16, 16), (-1, 16, 16, 16), (3, -4, 16, 16)):
        assert plan(ctypes.byref(S(*bad)), 1, ctypes.byref(out)) == LSQ_EINVAL and b"at least 1" in err(), bad
    for bad in ((3, 16, 15, 16), (3, 16, 16, 15), (3, 16, 0, 16), (1, 16, 16, -16)):
        assert plan(ctypes.byref(S(*bad)), 1, ctypes.byref(out)) == LSQ_EINVAL and b"must be at least C" in err(), bad
    for bad in ((1 << 40, 16, 1 << 40, 16), (1 << 40, 16, 16, 1 << 40), (1, 1 << 32, 1 << 32, 1 << 32), (1 << 30, 1 << 30, 1 << 30, 1 << 30)):
        assert plan(ctypes.byref(S(*bad)), 1, ctypes.byref(out)) == LSQ_EINVAL and b"64-bit offsets" in err(), bad
    assert plan(ctypes.byref(S(1 << 30, 1 << 10, 1 << 10, 1 << 10)), 0, ctypes.byref(out)) == LSQ_EINVAL and b"31-bit grid" in err()
    assert plan(ctypes.byref(S(1 << 20, 16, 1 << 30, 1 << 30)), 1, ctypes.byref(out)) == 0            # strides far apart are served
    rows, Cn = 6, 16
    gu = torch.zeros(rows * 2 * Cn + 64, dtype=torch.uint8)
    yy = torch.zeros(rows * Cn * 4 + 64, dtype=torch.uint8)
    tab = torch.zeros(256 + 4)
    s, z = torch.ones(4), torch.zeros(4, dtype=torch.int32)

    def consts(**kw):
        base = dict(s_u=s.data_ptr(), z_u=z.data_ptr(), out_scale=s.data_ptr() + 8, out_shift=s.data_ptr() + 12, quant_min=0, quant_max=255,
                    type_min=0, type_max=255, mid_dtype=E.LSQ_F32)
        base.update(kw)
        return E.LsqGluW8Consts(*[base[f[0]] for f in E.LsqGluW8Consts._fields_])

    def call(c=None, gd=0, ud=0, gp=gu.data_ptr(), up=gu.data_ptr() + Cn, tp=tab.data_ptr(), yp=yy.data_ptr(), shape=(rows, Cn, 2 * Cn, 2 * Cn),
             no_consts=False, no_shape=False):
        c = consts() if c is None else c
        return lib.lsq_glu_w8(gd, gp, ud, up, tp, None if no_shape else ctypes.byref(S(*shape)), None if no_consts else ctypes.byref(c), yp, None)
    assert call(gd=2) == LSQ_EINVAL and b"gate_dtype must be" in err()
    assert call(ud=-1) == LSQ_EINVAL and b"up_dtype must be" in err()
    assert call(no_shape=True) == LSQ_EINVAL and b"NULL shape" in err()
    assert call(no_consts=True) == LSQ_EINVAL and b"NULL constants" in err()
    assert call(shape=(0, Cn, Cn, Cn)) == LSQ_EINVAL and b"at least 1" in err()
    assert call(shape=(rows, Cn, Cn - 1, 2 * Cn)) == LSQ_EINVAL and b"must be at least C" in err()
    assert call(shape=(1 << 40, Cn, 1 << 40, Cn)) == LSQ_EINVAL and b"64-bit offsets" in err()
    for p in ("gp", "up", "tp", "yp"):
        assert call(**{p: None}) == LSQ_EINVAL and b"NULL buffer" in err(), p
    assert call(tp=tab.data_ptr() + 2) == LSQ_EINVAL and b"4-byte aligned" in err()
    assert call(consts(mid_dtype=E.LSQ_F64)) == LSQ_EINVAL and b"mid_dtype must be" in err()
    for f in ("s_u", "z_u"):
        assert call(consts(**{f: None})) == LSQ_EINVAL and b"NULL s_u or z_u" in err(), f
        assert call(consts(**{f: s.data_ptr() + 2})) == LSQ_EINVAL and b"element-aligned" in err(), f
    assert call(consts(out_scale=None)) == LSQ_EINVAL and b"come together" in err()
    assert call(consts(out_shift=None)) == LSQ_EINVAL and b"come together" in err()
    assert call(consts(out_shift=s.data_ptr() + 1)) == LSQ_EINVAL and b"element-aligned" in err()
    for rng in ((5, 4, 0, 255), (0, 255, 9, 8), (-1, 255, 0, 255), (0, 255, -128, 127), (-129, 0, -128, 127), (0, 256, 0, 255)):
        assert call(consts(quant_min=rng[0], quant_max=rng[1], type_min=rng[2], type_max=rng[3])) == LSQ_EINVAL and b"must lie within" in err(), rng
    # y against the SPAN of gate ((rows - 1) * stride + C bytes from its base), of up, and the table's 1024 bytes
    span = (rows - 1) * 2 * Cn + Cn
    for off in (0, 1, span - 1):
        assert call(yp=gu.data_ptr() + off) == LSQ_EINVAL and b"overlap the gate's span" in err(), off
    assert call(yp=gu.data_ptr() + span) == LSQ_EINVAL and b"overlap up's span" in err()      # y starts behind gate's span, in up's last row
    assert call(gp=yy.data_ptr() + rows * Cn - 1) == LSQ_EINVAL and b"overlap the gate's span" in err()
    assert call(up=yy.data_ptr() + rows * Cn - 1) == LSQ_EINVAL and b"overlap up's span" in err()
    for off in (0, 1020, -(rows * Cn - 1)):
        assert call(yp=tab.data_ptr() + off) == LSQ_EINVAL and b"overlap the table's 1024" in err(), off
    floats = consts(out_scale=None, out_shift=None)
    assert call(floats, gp=yy.data_ptr() + rows * Cn * 4 - 1) == LSQ_EINVAL and b"overlap the gate's span" in err()      # y is 4 bytes an element
    assert call(floats, yp=yy.data_ptr() + 2) == LSQ_EINVAL and b"element-aligned" in err()
    assert call(consts(out_scale=None, out_shift=None, mid_dtype=E.LSQ_BF16), yp=yy.data_ptr() + 1) == LSQ_EINVAL and b"element-aligned" in err()


def test_host_checks_of_the_ops():
    from torchlsq.functional import LevelsTensor, lsq_glu_act_w8_q, lsq_glu_table, lsq_glu_w8, lsq_glu_w8_q
    for name in ("lsq_glu_w8_q8_q", "lsq_glu_w8_q8"):
        assert hasattr(OPS, name)
    c = C.glu_case(5, 48, layout="halves")
    gate, up = C.operands(c)
    args = (gate.levels, up.levels, up.scale, up.zero_point, c["table"])
    q = (c["osc"], c["osh"], *c["rng"])
    with pytest.raises(RuntimeError, match="gate_levels must be uint8"):
        OPS.lsq_glu_w8_q8(gate.levels.float(), *args[1:], torch.float32)
    with pytest.raises(RuntimeError, match="up_levels must be uint8"):
        OPS.lsq_glu_w8_q8(args[0], up.levels.float(), *args[2:], torch.float32)
    with pytest.raises(RuntimeError, match="of one shape"):
        OPS.lsq_glu_w8_q8(args[0], up.levels[:, :32], *args[2:], torch.float32)
    with pytest.raises(RuntimeError, match="one float32 value"):
        OPS.lsq_glu_w8_q8(args[0], args[1], up.scale.double(), *args[3:], torch.float32)
    with pytest.raises(RuntimeError, match="one float32 value"):
        OPS.lsq_glu_w8_q8(*args[:3], up.zero_point.long(), args[4], torch.float32)
    for bad in (c["table"][:255], c["table"].double(), c["table"].to(torch.uint8), c["table"].repeat(2)[::2]):
        with pytest.raises(RuntimeError, match="256 entries"):
            OPS.lsq_glu_w8_q8(*args[:4], bad, torch.float32)
    with pytest.raises(RuntimeError, match="out_dtype must be"):
        OPS.lsq_glu_w8_q8(*args, torch.float64)
    with pytest.raises(RuntimeError, match="mid_dtype must be"):
        OPS.lsq_glu_w8_q8_q(*args, *q, torch.float64)
    with pytest.raises(RuntimeError, match="must lie within"):
        OPS.lsq_glu_w8_q8_q(*args, c["osc"], c["osh"], -1, 255, 0, 255, torch.float32)
    with pytest.raises(RuntimeError, match="float32 tensors of one value"):
        OPS.lsq_glu_w8_q8_q(*args, c["osc"].repeat(2), c["osh"], *c["rng"], torch.float32)
    with pytest.raises(RuntimeError, match="inference-only"):
        OPS.lsq_glu_w8_q8_q(*args, c["osc"].clone().requires_grad_(True), c["osh"], *c["rng"], torch.float32)
    with pytest.raises(RuntimeError, match="inference-only"):
        OPS.lsq_glu_w8_q8(*args[:4], c["table"].clone().requires_grad_(True), torch.float32)
    # any leading axes; an operand that is no row-strided view is made dense first; an empty tensor; a new dense result
    want = C.run(c)
    assert want.is_contiguous() and want.shape == (5, 48) and want.dtype == torch.uint8
    g3, u3 = gate.levels.contiguous().reshape(5, 3, 16), up.levels.contiguous().reshape(5, 3, 16)
    assert torch.equal(OPS.lsq_glu_w8_q8_q(g3, u3, *args[2:], *q, c["mid"]), want.reshape(5, 3, 16))
    gt = gate.levels.t().contiguous().t()            # column-major: innermost stride 5
    assert gt.stride() == (1, 5) and torch.equal(OPS.lsq_glu_w8_q8_q(gt, *args[1:], *q, c["mid"]), want)
    ge = gate.levels[:1].expand(5, 48)               # row stride 0
    assert ge.stride() == (0, 1) and torch.equal(OPS.lsq_glu_w8_q8_q(ge, *args[1:], *q, c["mid"]), OPS.lsq_glu_w8_q8_q(ge.contiguous(), *args[1:], *q, c["mid"]))
    assert OPS.lsq_glu_w8_q8_q(gate.levels[:0], up.levels[:0], *args[2:], *q, c["mid"]).shape == (0, 48)
    assert OPS.lsq_glu_w8_q8(gate.levels[:0], up.levels[:0], *args[2:], torch.bfloat16).dtype == torch.bfloat16
    # the functional entry points
    got = lsq_glu_w8_q(gate, up, c["table"], c["osc"], c["osh"], 0, 255, mid_dtype=c["mid"])
    assert isinstance(got, LevelsTensor) and torch.equal(got.levels, want) and got.scale.dtype == torch.float32
    assert (got.quant_min, got.quant_max) == (0, 255)
    assert torch.equal(lsq_glu_act_w8_q(gate, up, "silu", c["osc"], c["osh"], 0, 255, mid_dtype=c["mid"]).levels, want)
    f = lsq_glu_w8(gate, up, c["table"], torch.bfloat16)
    assert f.dtype == torch.bfloat16 and f.shape == (5, 48)
    with pytest.raises(AssertionError, match="out_scale"):
        lsq_glu_w8_q(gate, up, c["table"])
    with pytest.raises(AssertionError, match="one shape"):
        lsq_glu_w8_q(gate, LevelsTensor(up.levels[:, :16], up.scale, up.zero_point, 0, 255), c["table"], c["osc"], c["osh"], 0, 255)
    with pytest.raises(AssertionError, match="LevelsTensor"):
        lsq_glu_w8(gate.levels, up, c["table"])
    with pytest.raises(AssertionError, match="unknown activation"):
        lsq_glu_table("softmax", gate.scale, gate.zero_point, torch.uint8)
    with pytest.raises(AssertionError, match="gate_dtype must be"):
        lsq_glu_table("silu", gate.scale, gate.zero_point, torch.int16)
    with pytest.raises(AssertionError, match="must return a bfloat16 tensor"):
        lsq_glu_table(lambda v: v.float(), gate.scale, gate.zero_point, torch.uint8, None, torch.bfloat16)
    with pytest.raises(AssertionError, match="act_out is"):
        lsq_glu_table("silu", gate.scale, gate.zero_point, torch.uint8, (one(0.1), one(0.0)))
    # the fake kernels: shapes and dtypes of the real ones
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        fa = [mode.from_tensor(v) for v in args]
        fq = OPS.lsq_glu_w8_q8_q(*fa, mode.from_tensor(c["osc"]), mode.from_tensor(c["osh"]), -128, 127, -128, 127, torch.float32)
        fl = OPS.lsq_glu_w8_q8(*fa, torch.float16)
    assert (fq.shape, fq.dtype, fq.is_contiguous()) == ((5, 48), torch.int8, True)
    assert (fl.shape, fl.dtype, fl.is_contiguous()) == ((5, 48), torch.float16, True)


# ---------------------------------------------------------------------------------------------------
# lsq_glu_table
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", C.MIDS, ids=C.name)
@pytest.mark.parametrize("gd", C.LEVEL_DTYPES, ids=C.name)
def test_glu_table_is_its_definition_written_out(gd, mid):
    from torchlsq.functional import LevelsTensor, act_function, lsq_act_table, lsq_glu_table
    s, z = one(0.05), one(128 if gd == torch.uint8 else 0, torch.int32)
    b = torch.arange(256, dtype=torch.uint8).view(gd)
    lo = (0, 255) if gd == torch.uint8 else (-128, 127)
    u = LevelsTensor(b, s, z, *lo).dequantize(mid)
    for fn in C.CLAMP_TYPE + C.TRANSCENDENTAL:
        call, _ = act_function(fn)
        A = lsq_glu_table(fn, s, z, gd, None, mid)
        assert A.dtype == torch.float32 and A.shape == (256,)
        assert torch.equal(C.bits(A), C.bits((u if call is None else call(u)).float())), fn
        assert torch.equal(C.bits(A.to(mid).float()), C.bits(A)), fn                   # values of mid
        for act in ((one(0.03), one(-0.4), 0, 255), (one(0.02), one(0.1), -128, 127, -128, 127)):
            A2 = lsq_glu_table(fn, s, z, gd, act, mid)
            lv = lsq_act_table(fn, s, z, gd, *act, mid_dtype=mid)
            lv = lv if act[3] > 127 else lv.view(torch.int8)
            zp = torch.clamp(-act[1] / act[0], act[2], act[3]).round().to(torch.int32)
            want = LevelsTensor(lv, act[0], zp, act[2], act[3]).dequantize(mid).float()
            assert torch.equal(C.bits(A2), C.bits(want)), (fn, act[2])
    # a module and a callable go through act_function as they do for lsq_act_table
    A = lsq_glu_table(torch.nn.GELU(approximate="tanh"), s, z, gd, None, mid)
    assert torch.equal(C.bits(A), C.bits(lsq_glu_table("gelu_tanh", s, z, gd, None, mid)))
    assert torch.equal(C.bits(lsq_glu_table(lambda v: v * 2, s, z, gd, None, mid)), C.bits((u * 2).float()))


# ---------------------------------------------------------------------------------------------------
# the CPU path against the two compositions and numpy
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", C.MIDS, ids=C.name)
@pytest.mark.parametrize("pair", C.DTYPE_PAIRS, ids=C.pair_id)
def test_cpu_path_is_both_compositions_and_the_numpy_restatement(pair, mid):
    checked = 0
    for fn, act_q, unsigned, layout in itertools.product(("relu", "silu", "gelu", "sigmoid"), (False, True), (True, False, None),
                                                         ("halves",)):
        for zu in (128, 3):
            c = C.glu_case(24, 48, pair, (unsigned, mid), fn, act_q, layout, zu, seed=checked)
            got = C.run(c)
            note = (fn, act_q, unsigned, zu)
            want = C.composed_with_act_quantizer(c) if act_q else C.composed_without(c)
            assert C.same(got, want), note
            assert C.matches_numpy(got, c), note
            if unsigned is not None:
                assert got.dtype == (torch.uint8 if unsigned else torch.int8)
                C.assert_conditions(got, c, note)
            else:
                assert got.dtype == mid and len(got.float().unique()) > 100
            checked += 1
    assert checked == 48


@pytest.mark.parametrize("mid", C.MIDS, ids=C.name)
@pytest.mark.parametrize("pair", C.DTYPE_PAIRS, ids=C.pair_id)
def test_all_65536_byte_pairs(pair, mid):
    """C = 256, 256 rows, gate byte = row index, up byte = column index, with and without an activation quantizer"""
    for act_q in (False, True):
        c = C.glu_case(256, 256, pair, (True, mid), "silu", act_q, "dense", exhaustive=True)
        gate, up = C.operands(c)
        assert torch.equal(gate.levels.view(torch.uint8)[:, 0], torch.arange(256, dtype=torch.uint8))
        assert torch.equal(up.levels.view(torch.uint8)[0], torch.arange(256, dtype=torch.uint8))
        got = C.run(c)
        assert C.same(got, C.composed_with_act_quantizer(c) if act_q else C.composed_without(c)), act_q
        assert C.matches_numpy(got, c), act_q
        assert len(got.unique()) > 64


def test_special_values_of_the_table():
    """a NaN entry goes to quant_min (and stays a NaN in the floats), +-inf clamp to the borders; an inf times a zero of up is a NaN"""
    for mid in C.MIDS:
        for unsigned in (True, False):
            c = C.glu_case(16, 16, (torch.uint8, torch.uint8), (unsigned, mid), "silu", zu=128)
            c["table"] = c["table"].clone()
            c["table"][7], c["table"][8], c["table"][9] = float("nan"), float("inf"), float("-inf")
            gate, up = C.operands(c)
            gate.levels[0, :] = 7
            gate.levels[1, :] = 8
            gate.levels[2, :] = 9
            up.levels[:3, 0:4] = torch.tensor([130, 120, 128, 255], dtype=torch.uint8)       # +, -, the zero point, the largest
            got = C.run(c).to(torch.int64)
            lo, hi = c["rng"][0], c["rng"][1]
            assert got[0].tolist() == [lo] * 16
            assert got[1, :4].tolist() == [hi, lo, lo, hi] and got[2, :4].tolist() == [lo, hi, lo, lo]
            assert C.matches_numpy(C.run(c), c)
            f = C.run(dict(c, rng=None)).float()
            assert bool(f[0].isnan().all()) and f[1, 0] == float("inf") and f[1, 1] == float("-inf") and bool(f[1, 2].isnan())
            assert f[2, 0] == float("-inf") and f[2, 3] == float("-inf")
    # a table that does not hold values of mid_dtype is rounded to it first
    c = C.glu_case(24, 48, out_variant=(True, torch.float32))
    for mid in (torch.bfloat16, torch.float16):
        assert not torch.equal(c["table"].to(mid).float(), c["table"])
        assert C.same(C.run(dict(c, mid=mid)), C.run(dict(c, mid=mid, table=c["table"].to(mid).float()))) and C.matches_numpy(C.run(dict(c, mid=mid)), dict(c, mid=mid))


@pytest.mark.parametrize("layout", ("halves", "padded", "off_by_one", "odd_stride"))
def test_views_give_the_bytes_of_their_dense_copies(layout):
    from torchlsq.functional import LevelsTensor
    for pair, mid, unsigned in ((C.DTYPE_PAIRS[0], torch.float32, True), (C.DTYPE_PAIRS[1], torch.bfloat16, False),
                                (C.DTYPE_PAIRS[2], torch.float16, None)):
        c = C.glu_case(17, 48, pair, (unsigned, mid), "silu", False, layout, seed=3)
        gate, up = C.operands(c)
        assert not gate.levels.is_contiguous() or layout == "off_by_one"
        before = [b.clone() for b in c["bufs"]]
        got = C.run(c)
        d = C.run(c, ops=(C.dense(gate), C.dense(up)))
        assert C.same(got, d) and got.is_contiguous(), (layout, pair)
        assert all(torch.equal(a, b) for a, b in zip(before, c["bufs"]))                  # the operands are only read
        if layout in ("halves", "padded"):
            assert gate.levels.data_ptr() + 48 == up.levels.data_ptr()                    # ONE buffer, cut in place
            # the bytes between the rows never influence the result
            other = dict(c, bufs=[b.clone() for b in c["bufs"]])
            keep = torch.zeros_like(other["bufs"][0], dtype=torch.bool)
            for side in ("gate", "up"):
                C.view(keep, c[side], 17, 48, torch.bool).fill_(True)
            other["bufs"][0][~keep] ^= 0xff
            assert layout == "halves" or int((~keep).sum()) == 17 * 16
            assert C.same(C.run(other), got)
    # a [B, T, 2 C] fused output: the leading axes collapse to one row stride
    c = C.glu_case(12, 32, layout="halves", seed=5)
    gate, up = C.operands(c)
    g3, u3 = (LevelsTensor(t.levels.unflatten(0, (3, 4)), t.scale, t.zero_point, 0, 255) for t in (gate, up))
    assert g3.levels.stride() == (256, 64, 1)
    assert torch.equal(OPS.lsq_glu_w8_q8_q(g3.levels, u3.levels, up.scale, up.zero_point, c["table"], c["osc"], c["osh"], *c["rng"], c["mid"]),
                       C.run(c).unflatten(0, (3, 4)))


def test_the_product_is_rounded_on_its_own_never_contracted():
    """a * d is ONE rounded float32 multiply before level()'s multiply-add: with a table entry and an up value whose exact product is
    not a float32, level(t) with t the rounded product is what the definition asks for"""
    c = C.glu_case(256, 256, (torch.uint8, torch.uint8), (True, torch.float32), "gelu", exhaustive=True)
    got = C.run(c)
    t = C.numpy_value(c)
    gate, up = C.operands(c)
    a = c["table"].numpy()[gate.levels.numpy().astype(np.int64)].astype(np.float64)
    d = ((up.levels.numpy().astype(np.float32) - np.float32(128)) * np.float32(C.S_U)).astype(np.float64)
    inexact = (a * d) != t.astype(np.float64)
    assert inexact.mean() > 0.5                              # the float32 product is rounded nearly everywhere
    assert C.matches_numpy(got, c)


# ---------------------------------------------------------------------------------------------------
# the modules and the converter
# ---------------------------------------------------------------------------------------------------
def test_state_dict_round_trips():
    from torchlsq.quantized import GLUW8Q, GatedMLPW8Q, convert_w8a8_glu
    net, qs, x = C.mlp_block(shared=True, act_q=True)
    m = GLUW8Q.from_float(net.mlp.act_fn, qs["gate"], qs["hidden"], qs["act"], torch.bfloat16)
    assert m.table.dtype == torch.float32 and m.table.shape == (256,) and m.function == "silu" and m.mid_dtype == torch.bfloat16
    sd = m.state_dict()
    assert sorted(k for k in sd if not k.endswith("_extra_state")) == ["output_scale", "output_shift", "table"]
    assert sd["_extra_state"] == dict(output_range=list(m.output_range), mid_dtype="bfloat16", function="silu") and len(m.output_range) == 4
    fresh = GLUW8Q()
    fresh.load_state_dict(sd)
    assert fresh.mid_dtype == torch.bfloat16 and fresh.function == "silu" and fresh.output_range == m.output_range
    assert torch.equal(C.bits(fresh.table), C.bits(m.table)) and torch.equal(fresh.output_scale, m.output_scale)
    assert "silu(gate) * up" in repr(m)
    # the whole MLP: fused and unfused, through their state dicts
    for shared in (True, False):
        net, qs, x = C.mlp_block(shared=shared)
        conv = convert_w8a8_glu(net, {"mlp": C.mlp_quantizers(qs)})
        assert isinstance(conv.mlp, GatedMLPW8Q) and conv.mlp.fused == shared
        keys = set(k.split(".")[1] for k in conv.state_dict())
        assert keys == ({"gate_up", "glu", "down"} if shared else {"gate_proj", "up_proj", "glu", "down"})
        again = convert_w8a8_glu(net, {"mlp": C.mlp_quantizers(qs)})
        for p in again.state_dict().values():
            if isinstance(p, torch.Tensor):
                p.zero_()
        again.load_state_dict(conv.state_dict())
        xl = C_levels(qs["in"], x)
        assert torch.equal(again.mlp(xl, xl).levels, conv.mlp(xl, xl).levels)


def C_levels(q, x):
    from torchlsq.functional import LevelsTensor
    return LevelsTensor.from_quantized(q.quantize(x))


@pytest.mark.parametrize("mid", C.MIDS, ids=C.name)
def test_gated_mlp_fused_and_unfused_give_the_same_bytes_and_equal_the_modules_written_out(mid):
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import GLUW8Q, GatedMLPW8Q, LinearW8A8AddQ, LinearW8A8Q
    for act_q in (False, True):
        net, qs, x = C.mlp_block(shared=True, act_q=act_q)
        mlp = net.mlp
        xl = C_levels(qs["in"], x)
        down = LinearW8A8AddQ.from_float(mlp.down_proj, qs["hidden"], qs["add"], pre_quantizer=qs["down"], mid_dtype=mid)
        args = (mlp.act_fn, qs["in"], qs["gate"], qs["up"], qs["hidden"], qs.get("act"), mid)
        fused = GatedMLPW8Q.from_float(mlp.gate_proj, mlp.up_proj, down, *args)
        assert fused.fused and fused.gate_up.out_features == 96 and fused.gate_up.weight_levels.shape == (96, 32)
        # a second quantizer OBJECT with the same constants: two linears
        import copy
        two = GatedMLPW8Q.from_float(mlp.gate_proj, mlp.up_proj, down, mlp.act_fn, qs["in"], qs["gate"], copy.deepcopy(qs["up"]), qs["hidden"],
                                     qs.get("act"), mid)
        assert not two.fused
        a, b = fused(xl, xl), two(xl, xl)
        assert isinstance(a, LevelsTensor) and a.levels.shape == (24, 32) and torch.equal(a.levels, b.levels)
        # the fused linear's output is ONE [rows, 2 C] tensor whose halves are the two linears' outputs, and the product read them in place
        gu = fused.gate_up(xl)
        assert gu.levels.shape == (24, 96) and torch.equal(gu.levels[:, :48], two.gate_proj(xl).levels) and \
            torch.equal(gu.levels[:, 48:], two.up_proj(xl).levels)
        h = fused.glu(gu)
        assert torch.equal(h.levels, two.glu(two.gate_proj(xl), two.up_proj(xl)).levels) and len(h.levels.unique()) > 32
        # written out with the existing ops: the byte table + the gate multiply, or dequantize -> SiLU -> multiply -> levels
        g, u = two.gate_proj(xl), two.up_proj(xl)
        if act_q:
            from torchlsq.quantized import ActivationW8Q, MulGateW8Q
            want = MulGateW8Q.from_float(None, qs["hidden"], mid_dtype=mid)(ActivationW8Q.from_float("silu", qs["gate"], qs["act"], mid_dtype=mid)(g), u)
            assert torch.equal(h.levels, want.levels)
        else:
            t = torch.nn.functional.silu(g.dequantize(mid)) * u.dequantize(mid)
            m = fused.glu
            assert torch.equal(h.levels, OPS.lsq_levels_per_tensor(t, m.output_scale, m.output_shift, *m.output_range, 0).view(torch.uint8))
        assert torch.equal(a.levels, down(h, xl).levels)
        # without a residual: a LinearW8A8Q down; a residual is then refused
        plain = GatedMLPW8Q.from_float(mlp.gate_proj, mlp.up_proj, LinearW8A8Q.from_float(mlp.down_proj, qs["hidden"], qs["down"], mid_dtype=mid), *args)
        assert plain(xl).levels.shape == (24, 32)
        with pytest.raises(TypeError, match="needs a LinearW8A8AddQ"):
            plain(xl, xl)


def test_converter_and_its_refusals():
    from torchlsq.quantized import GatedMLPW8Q, GLUW8Q, LinearW8A8AddQ, LinearW8A8Q, convert_w8a8_glu
    net, qs, x = C.mlp_block(shared=True)
    conv = convert_w8a8_glu(net, {"mlp": C.mlp_quantizers(qs)})
    assert isinstance(conv.mlp, GatedMLPW8Q) and isinstance(conv.mlp.down, LinearW8A8AddQ) and isinstance(conv.mlp.glu, GLUW8Q)
    assert isinstance(net.mlp, C.GatedMLP)                                           # a deep copy
    assert isinstance(convert_w8a8_glu(net, {"mlp": C.mlp_quantizers(qs, add=False)}).mlp.down, LinearW8A8Q)
    # `act` in the place of `act_fn`
    net2, qs2, _ = C.mlp_block(shared=True)
    net2.mlp.act = net2.mlp.act_fn
    del net2.mlp.act_fn
    assert convert_w8a8_glu(net2, {"mlp": C.mlp_quantizers(qs2)}).mlp.glu.function == "silu"
    with pytest.raises(ValueError, match="'nope' is not a gated MLP"):
        convert_w8a8_glu(net, {"nope": C.mlp_quantizers(qs)})
    with pytest.raises(ValueError, match="'mlp.gate_proj' is not a gated MLP"):
        convert_w8a8_glu(net, {"mlp.gate_proj": C.mlp_quantizers(qs)})
    with pytest.raises(ValueError, match="'' is not a gated MLP"):
        convert_w8a8_glu(net, {"": C.mlp_quantizers(qs)})
    with pytest.raises(ValueError, match="needs a dict with"):
        convert_w8a8_glu(net, {"mlp": {k: v for k, v in C.mlp_quantizers(qs).items() if k != "hidden_quantizer"}})
    with pytest.raises(ValueError, match="needs a dict with"):
        convert_w8a8_glu(net, {"mlp": dict(C.mlp_quantizers(qs), other=None)})
    with pytest.raises(ValueError, match="needs a dict with"):
        convert_w8a8_glu(net, {"mlp": qs["in"]})
    with pytest.raises(ValueError, match="must be a converted"):
        GatedMLPW8Q.from_float(net.mlp.gate_proj, net.mlp.up_proj, net.mlp.down_proj, "silu", qs["in"], qs["gate"], qs["up"], qs["hidden"])
    with pytest.raises(TypeError, match="needs two LevelsTensors"):
        conv.mlp.glu(C_levels(qs["in"], x), x)
    with pytest.raises(AssertionError, match="an even number of columns"):
        conv.mlp.glu(C_levels(qs["in"], x[:, :31]))
