"""LayerNorm and RMSNorm on 8-bit levels (include/lsq_hip_norm_w8.h), everything that needs no GPU: the library's exports against
its header and `_abi.py`, its kernel set and their resources, the plan on both sides of every threshold, every refusal, and the CPU
path of the ops -- the definition the GPU tests compare against -- held to an independent numpy restatement bit for bit and to
float64 within the derived bound, with the modules and the converter on top.
"""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import norm_w8_cases as N
import requant_w8_cases as R
from helpers import LLVM, demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_norm_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_norm_w8.so")
NAMES = sorted(["lsq_norm_w8_abi_version", "lsq_norm_w8_last_error", "lsq_norm_w8", "lsq_norm_w8_plan"])
LSQ_EINVAL = -1
CL = torch.channels_last
OPS = torch.ops.torchlsq
one = N.one


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    return [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(const void\*|int64_t|float)", "", decl.strip()).split(",") if f.strip()]


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_norm_w8\w*)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_NORM_W8) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_", "lsq_requant_", "lsq_resadd_",
                  "lsq_pool_", "lsq_dwconv_", "lsq_eltwise_", "lsq_norm_"):
        assert other not in und, other
    assert E.norm_w8_library().lsq_norm_w8_abi_version() == E.NORM_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_NORM_W8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    assert _fields(text, "lsq_norm_w8_geom") == [f[0] for f in E.LsqNormW8Geom._fields_] and ctypes.sizeof(E.LsqNormW8Geom) == 4 * 8
    assert _fields(text, "lsq_norm_w8_consts") == [f[0] for f in E.LsqNormW8Consts._fields_] and ctypes.sizeof(E.LsqNormW8Consts) == 13 * 8


def test_kernels(tmp_path):
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    short = {}
    for sym, dm in names.items():
        m = re.match(r"^(?:void )?lsq::norm_w8_(packets|generic)_kernel(?:<([^>]*)>)?\(", dm)
        assert m, "not a kernel of this library: %s" % dm
        short[sym] = m.group(1) + "".join("_" + n for n in re.findall(r"\d+", re.sub(r"\(int\)", "", m.group(2) or "")))
    # packets_<lanes per row>_<packets per lane>
    assert sorted(short.values()) == sorted(["generic"] + ["packets_%d_%d" % (L, P) for L in (4, 8, 16, 32, 64) for P in range(1, 9)])
    assert set("packets_%d_%d" % lp for lp in N.every_lp()) <= set(short.values())
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
        # w and bias are staged in DYNAMIC LDS, sized by the plan (lds_bytes) at the launch: no kernel has a fixed segment
        assert lds[sym] == 0, (sym, lds[sym])
        # the correctly rounded square root: v_sqrt_f32 and its correction by two fmas on the neighbouring floats, and the divisions
        assert ops.count("v_sqrt_f32_e32") == 1 and "v_div_fixup_f32" in ops and "v_rsq_f32_e32" not in ops, sym
        at = ops.index("v_sqrt_f32_e32")
        assert ops[at:at + 14].count("v_fma_f32") >= 2, (sym, ops[at:at + 14])
        if short[sym].startswith("packets"):
            L, P = (int(v) for v in short[sym].split("_")[1:])
            assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops, sym
            # the row sums come from the dot instruction on the words as loaded, eight a packet, after the last load of the row
            dots = [i for i, o in enumerate(ops) if o.startswith("v_dot4_u32_u8")]
            assert len(dots) == 8 * P, (sym, len(dots))
            loop = ops[:dots[0]]
            loads = [i for i, o in enumerate(loop) if o == "global_load_dwordx4"]
            assert len(loads) >= P and "s_barrier" not in ops[dots[0]:], sym
            # parameters: registers for one packet a lane, LDS reads above
            assert ("ds_read_b128" in ops or "ds_read2_b64" in ops or "ds_read_b32" in ops or "ds_read2_b32" in ops) == (P > 1), sym


def test_plans_without_a_gpu():
    from torchlsq import extension as E
    for C, aligned in itertools.product((1, 3, 15, 16, 17, 20, 24, 32, 48, 96, 768, 1024, 1040, 4096, 8192, 8208, 65536), (True, False)):
        for R_ in (1, 2, 1000):
            assert E.norm_w8_plan(R_, C, aligned) == N.expected_plan(R_, C, aligned), (R_, C, aligned)
    # the family: packets if and only if C % 16 == 0, C <= 8192 and the buffers are aligned
    assert E.norm_w8_plan(5, 8192)["family"] == "packets" and E.norm_w8_plan(5, 8208)["family"] == "generic"
    assert E.norm_w8_plan(5, 16)["family"] == "packets" and E.norm_w8_plan(5, 16, aligned=False)["family"] == "generic"
    # (L, P): the fewest masked lanes, then the fewest packets.  768 elements are 48 packets: 16 lanes of 3, not 64 lanes of one
    want = {16: (4, 1), 64: (4, 1), 96: (4, 2), 128: (8, 1), 768: (16, 3), 1024: (64, 1), 1040: (16, 5), 2048: (64, 2), 4096: (64, 4),
            8192: (64, 8), 8176: (64, 8)}
    for C, lp in want.items():
        pl = E.norm_w8_plan(9, C)
        assert (pl["lanes_per_row"], pl["packets_per_lane"]) == lp == N.choose_lp(C), (C, pl)
    for C in range(16, 8193, 16):
        L, P = N.choose_lp(C)
        assert L * P >= C // 16 and L in (4, 8, 16, 32, 64) and 1 <= P <= 8
    # where w and bias live: nowhere without them, registers for one packet a lane, LDS (4 C bytes each, dynamic) above
    assert E.norm_w8_plan(9, 1024)["params"] == "registers" and E.norm_w8_plan(9, 1024)["lds_bytes"] == 0
    assert E.norm_w8_plan(9, 1024, has_weight=False, has_bias=False)["params"] == "none"
    assert E.norm_w8_plan(9, 768) == dict(family="packets", grid=1, block=256, lanes_per_row=16, packets_per_lane=3, rows_per_workgroup=16,
                                          params="lds", lds_bytes=6144)
    assert E.norm_w8_plan(9, 768, has_bias=False)["lds_bytes"] == 3072 and E.norm_w8_plan(9, 768, has_weight=False, has_bias=False)["lds_bytes"] == 0
    assert E.norm_w8_plan(9, 8192)["lds_bytes"] == 65536
    # rows per workgroup: (256 / L) groups of K = 8 rows, K halved while the grid holds fewer than 2 * 256 workgroups
    for C, G in ((16, 64), (768, 16), (1024, 4)):
        for K in (8, 4, 2):
            edge = 511 * G * K + 1
            hi, lo = E.norm_w8_plan(edge, C), E.norm_w8_plan(edge - 1, C)
            assert hi["rows_per_workgroup"] == G * K and hi["grid"] == 512 and lo["rows_per_workgroup"] == G * K // 2, (C, K, hi, lo)
            assert hi == N.expected_plan(edge, C) and lo == N.expected_plan(edge - 1, C)
    assert E.norm_w8_plan(64 * 197, 768)["rows_per_workgroup"] == 16 and E.norm_w8_plan(32 * 56 * 56, 96)["rows_per_workgroup"] == 128
    assert E.norm_w8_plan(5, 20) == dict(family="generic", grid=2, block=256, lanes_per_row=64, packets_per_lane=0, rows_per_workgroup=4,
                                         params="none", lds_bytes=0)


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.norm_w8_library()
    err = lib.lsq_norm_w8_last_error
    out = (ctypes.c_int32 * 8)()
    G = E.LsqNormW8Geom
    assert lib.lsq_norm_w8_plan(None, 1, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"NULL geometry" in err()
    assert lib.lsq_norm_w8_plan(ctypes.byref(G(4, 16, 0, 0)), 1, 1, 1, None) == LSQ_EINVAL and b"NULL output" in err()
    for bad in ((0, 16), (4, 0), (-1, 16)):
        assert lib.lsq_norm_w8_plan(ctypes.byref(G(*bad, 0, 0)), 1, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"at least 1" in err(), bad
    assert lib.lsq_norm_w8_plan(ctypes.byref(G(4, 65537, 0, 0)), 1, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"at most 65536" in err()
    assert lib.lsq_norm_w8_plan(ctypes.byref(G(4, 65536, 0, 0)), 1, 1, 1, ctypes.byref(out)) == 0
    assert lib.lsq_norm_w8_plan(ctypes.byref(G(1 << 29, 16, 0, 0)), 1, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"beyond 29 bits" in err()
    assert lib.lsq_norm_w8_plan(ctypes.byref(G((1 << 29) - 1, 16, 0, 0)), 1, 1, 1, ctypes.byref(out)) == 0
    assert lib.lsq_norm_w8_plan(ctypes.byref(G(4, 16, 2, 0)), 1, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"kind must be" in err()
    assert lib.lsq_norm_w8_plan(ctypes.byref(G(4, 16, 0, 2)), 1, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"x_dtype must be" in err()
    # the call: every refusal comes before anything is enqueued, so host memory will do for the pointers
    x, yy = torch.zeros(4 * 16, dtype=torch.uint8), torch.zeros(4 * 16 * 4 + 16, dtype=torch.uint8)
    s, z, p = torch.ones(4), torch.zeros(4, dtype=torch.int32), torch.zeros(64)

    def consts(**kw):
        base = dict(s_x=s.data_ptr(), zx=z.data_ptr(), weight=p.data_ptr(), bias=p.data_ptr() + 64, out_scale=s.data_ptr() + 8,
                    out_shift=s.data_ptr() + 12, param_dtype=E.LSQ_F32, quant_min=0, quant_max=255, type_min=0, type_max=255,
                    mid_dtype=E.LSQ_F32, eps=1e-5)
        base.update(kw)
        return E.LsqNormW8Consts(*[base[f[0]] for f in E.LsqNormW8Consts._fields_])

    def call(c=None, geom=(4, 16, 0, 0), xp=x.data_ptr(), yp=yy.data_ptr(), no_consts=False, no_geom=False):
        c = consts() if c is None else c
        return lib.lsq_norm_w8(None if no_geom else ctypes.byref(G(*geom)), None if no_consts else ctypes.byref(c), xp, yp, None)
    assert call(no_geom=True) == LSQ_EINVAL and b"NULL geometry" in err()
    assert call(no_consts=True) == LSQ_EINVAL and b"NULL constants" in err()
    assert call(geom=(4, 0, 0, 0)) == LSQ_EINVAL and b"at least 1" in err()
    assert call(geom=(4, 65537, 0, 0)) == LSQ_EINVAL and b"at most 65536" in err()
    assert call(geom=(4, 16, 3, 0)) == LSQ_EINVAL and b"kind must be" in err()
    assert call(geom=(4, 16, 0, -1)) == LSQ_EINVAL and b"x_dtype must be" in err()
    for ptr in ("xp", "yp"):
        assert call(**{ptr: None}) == LSQ_EINVAL and b"NULL buffer" in err(), ptr
    assert call(consts(mid_dtype=E.LSQ_F64)) == LSQ_EINVAL and b"mid_dtype must be" in err()
    assert call(consts(param_dtype=E.LSQ_F64)) == LSQ_EINVAL and b"param_dtype must be" in err()
    assert call(consts(param_dtype=E.LSQ_F64, weight=None, bias=None), geom=(4, 16, 0, 0), yp=None) == LSQ_EINVAL and b"NULL buffer" in err()
    for f in ("s_x", "zx"):
        assert call(consts(**{f: None})) == LSQ_EINVAL and b"NULL s_x or zx" in err(), f
        assert call(consts(**{f: s.data_ptr() + 2})) == LSQ_EINVAL and b"element-aligned" in err(), f
    for f in ("weight", "bias"):
        assert call(consts(**{f: p.data_ptr() + 2})) == LSQ_EINVAL and b"weight and bias must be element-aligned" in err(), f
    assert call(consts(weight=p.data_ptr() + 1, param_dtype=E.LSQ_BF16)) == LSQ_EINVAL and b"element-aligned" in err()
    assert call(consts(out_scale=None)) == LSQ_EINVAL and b"come together" in err()
    assert call(consts(out_shift=None)) == LSQ_EINVAL and b"come together" in err()
    assert call(consts(out_shift=s.data_ptr() + 1)) == LSQ_EINVAL and b"element-aligned" in err()
    for eps in (-1e-9, float("nan"), -float("inf")):
        assert call(consts(eps=eps)) == LSQ_EINVAL and b"eps" in err(), eps
    for rng in ((5, 4, 0, 255), (0, 255, 9, 8), (-1, 255, 0, 255), (0, 255, -128, 127), (-129, 0, -128, 127), (0, 256, 0, 255)):
        assert call(consts(quant_min=rng[0], quant_max=rng[1], type_min=rng[2], type_max=rng[3])) == LSQ_EINVAL and b"must lie within" in err(), rng
    for off in (0, 1, 63):
        assert call(yp=x.data_ptr() + off) == LSQ_EINVAL and b"overlap x's" in err(), off
    assert call(xp=yy.data_ptr() + 63) == LSQ_EINVAL and b"overlap x's" in err()
    assert call(consts(weight=yy.data_ptr() + 60)) == LSQ_EINVAL and b"overlap the weight's or the bias's" in err()
    assert call(consts(bias=yy.data_ptr())) == LSQ_EINVAL and b"overlap the weight's or the bias's" in err()
    floats = consts(out_scale=None, out_shift=None)
    assert call(floats, yp=yy.data_ptr() + 2) == LSQ_EINVAL and b"a floating y must be element-aligned" in err()
    assert call(floats, yp=yy.data_ptr(), xp=yy.data_ptr() + 64 * 4 - 1) == LSQ_EINVAL and b"overlap x's" in err()                 # y is 4 bytes an element
    assert call(consts(out_scale=None, out_shift=None, mid_dtype=E.LSQ_BF16), yp=yy.data_ptr() + 1) == LSQ_EINVAL and b"element-aligned" in err()


def test_host_checks_of_the_ops():
    from torchlsq.functional import LevelsTensor, lsq_layer_norm_w8, lsq_layer_norm_w8_q, lsq_rms_norm_w8_q
    for name in ("lsq_layer_norm_w8_q8_q", "lsq_layer_norm_w8_q8", "lsq_rms_norm_w8_q8_q", "lsq_rms_norm_w8_q8"):
        assert hasattr(OPS, name)
    x, s, z = N.rows(6, 32), one(N.S_X), one(128, torch.int32)
    w, b = N.params(32)
    q = (one(0.02), one(-2.56), (0, 255, 0, 255))
    X = LevelsTensor(x, s, z, 0, 255)
    with pytest.raises(RuntimeError, match="uint8 .* or int8"):
        N.run("layer", x.to(torch.int16), s, z, w, b, 1e-5, q, torch.float32)
    with pytest.raises(RuntimeError, match="mid_dtype must be"):
        N.run("layer", x, s, z, w, b, 1e-5, q, torch.float64)
    with pytest.raises(RuntimeError, match="out_dtype must be"):
        N.run("rms", x, s, z, w, b, 1e-5, None, torch.float64)
    with pytest.raises(RuntimeError, match="one float32 value"):
        N.run("layer", x, torch.ones(2), z, w, b, 1e-5, q, torch.float32)
    with pytest.raises(RuntimeError, match="one float32 value"):
        N.run("layer", x, s, z.to(torch.int64), w, b, 1e-5, q, torch.float32)
    with pytest.raises(RuntimeError, match="eps = .* not negative"):
        N.run("layer", x, s, z, w, b, -1.0, q, torch.float32)
    with pytest.raises(RuntimeError, match=r"weight must be .* of \[32\]"):
        N.run("layer", x, s, z, w[:31], b, 1e-5, q, torch.float32)
    with pytest.raises(RuntimeError, match="bias must be"):
        N.run("layer", x, s, z, w, b.double(), 1e-5, q, torch.float32)
    with pytest.raises(RuntimeError, match="one dtype"):
        N.run("layer", x, s, z, w, b.half(), 1e-5, q, torch.float32)
    with pytest.raises(RuntimeError, match="must lie within"):
        N.run("layer", x, s, z, w, b, 1e-5, (q[0], q[1], (0, 300, 0, 255)), torch.float32)
    with pytest.raises(RuntimeError, match="per-tensor quantizer"):
        N.run("layer", x, s, z, w, b, 1e-5, (torch.ones(2), q[1], q[2]), torch.float32)
    with pytest.raises(RuntimeError, match="at most 65536"):
        N.run("layer", torch.zeros(1, 65537, dtype=torch.uint8), s, z, None, None, 1e-5, q, torch.float32)
    with pytest.raises(RuntimeError, match="inference-only"):
        N.run("layer", x, s, z, w.clone().requires_grad_(True), b, 1e-5, q, torch.float32)
    # the functional forms: dims, normalized_shape, the output quantizer
    with pytest.raises(AssertionError, match="dim must be -1"):
        lsq_layer_norm_w8(X, w, b, dim=0)
    with pytest.raises(AssertionError, match="dim must be -1"):
        lsq_layer_norm_w8(LevelsTensor(x.reshape(2, 3, 32), s, z, 0, 255), None, None, dim=1)
    with pytest.raises(AssertionError, match="not the trailing shape"):
        lsq_layer_norm_w8(X, w, b, normalized_shape=(16,))
    with pytest.raises(AssertionError, match="needs the output quantizer"):
        lsq_layer_norm_w8_q(X, w, b)
    with pytest.raises(AssertionError, match="needs a LevelsTensor"):
        lsq_rms_norm_w8_q(x, w, None, out_scale=q[0], out_shift=q[1], out_quant_min=0, out_quant_max=255)
    # an empty batch, `out=`, the fake kernels, several trailing axes flattened
    assert N.run("layer", x[:0], s, z, w, b, 1e-5, q, torch.float32).shape == (0, 32)
    from torchlsq import extension as E
    buf = torch.zeros(6 * 32 + 1, dtype=torch.uint8)
    got = E.norm_w8_layer_q(x, s, z, w, b, 1e-5, q[0], q[1], *q[2], torch.float32, out=buf[1:].view(6, 32))
    assert got.data_ptr() == buf.data_ptr() + 1 and torch.equal(got, N.run("layer", x, s, z, w, b, 1e-5, q, torch.float32))
    with pytest.raises(RuntimeError, match="`out` must be"):
        E.norm_w8_layer_q(x, s, z, w, b, 1e-5, q[0], q[1], *q[2], torch.float32, out=buf[1:].view(6, 32).to(torch.int8))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        fx = mode.from_tensor(x)
        assert OPS.lsq_layer_norm_w8_q8_q(fx, s, z, w, b, 1e-5, q[0], q[1], -128, 127, -128, 127, torch.float32).dtype == torch.int8
        assert OPS.lsq_rms_norm_w8_q8(fx, s, z, w, None, 1e-5, torch.bfloat16).dtype == torch.bfloat16
    x3 = LevelsTensor(x.reshape(3, 2, 4, 8), s, z, 0, 255)
    v = lsq_layer_norm_w8(x3, w.reshape(4, 8), b.reshape(4, 8), normalized_shape=(4, 8))
    assert v.shape == (3, 2, 4, 8) and torch.equal(v.reshape(6, 32), lsq_layer_norm_w8(X, w, b))


# ---------------------------------------------------------------------------------------------------
# the CPU path against the numpy restatement, the bound against float64
# ---------------------------------------------------------------------------------------------------
GRID = [(kind, xd, out, mid) for kind in N.KINDS for xd in N.LEVEL_DTYPES for out in (True, False, None) for mid in N.MIDS]


@pytest.mark.parametrize("kind,x_dtype,unsigned,mid", GRID, ids=lambda v: N.name(v) if isinstance(v, torch.dtype) else str(v))
def test_cpu_path_is_the_numpy_restatement(kind, x_dtype, unsigned, mid):
    eps = N.EPS[kind]
    for C, wb, pdt, z_u8 in ((96, (True, True), torch.float32, 128), (20, (True, False), torch.bfloat16, 3), (48, (False, True), torch.float16, 0),
                             (1040, (False, False), torch.float32, 128)):
        R_ = N.rows_for(C)
        x, s, z = N.rows(R_, C, 3, x_dtype), one(N.S_X), N.zero_for(x_dtype, z_u8)
        w, b = N.params(C, 3, pdt)
        w, b = (w if wb[0] else None), (b if wb[1] else None)
        want_u = N.np_norm(kind, x, s, int(z), w, b, eps, mid)
        if unsigned is None:
            got = N.run(kind, x, s, z, w, b, eps, None, mid)
            assert got.dtype == mid and np.array_equal(got.float().numpy().view(np.int32), want_u.view(np.int32)), (C, wb)
            continue
        has_w = w is not None
        q = N.quantizer_for(kind, x, s, z, w, b, eps, unsigned, N.one_sided(kind, z_u8)) if has_w or kind == "layer" else \
            (one(0.02), one(0.0 if unsigned else 0.0), ((0, 255, 0, 255) if unsigned else (-128, 127, -128, 127)))
        got = N.run(kind, x, s, z, w, b, eps, q, mid)
        assert got.dtype == (torch.uint8 if unsigned else torch.int8)
        assert np.array_equal(got.numpy(), N.np_levels(want_u, float(q[0]), float(q[1]), q[2])), (C, wb)
        if has_w or kind == "layer":
            N.assert_conditions(kind, x, s, z, w, b, eps, q, mid, got, (kind, C))


@pytest.mark.parametrize("kind", N.KINDS)
def test_the_bound_against_float64(kind):
    """|a - a_exact| <= 2^-20 (|t w| + |bias|), and the level is the float64 composition's level except where the float64 value
    lies within that bound of a rounding boundary.  Measured: the worst error over these cases is 2^-21.9 of the
    bound's scale."""
    worst = 0.0
    eps = N.EPS[kind]
    for C, s_x, seed in ((16, 1e-3, 0), (96, 0.02, 1), (768, 0.3, 2), (1024, 0.02, 3), (8192, 1e-3, 4), (65536, 0.02, 5)):
        x, at = N.planted(C, torch.uint8, seed)
        x = torch.cat([x, N.rows(24, C, seed)])
        s, z = one(s_x), one(128 if kind == "layer" else 117, torch.int32)
        w, b = N.params(C, seed)
        a = N.run(kind, x, s, z, w, b, eps, None, torch.float32).numpy().astype(np.float64)
        exact, tw, bias = N.f64_norm(kind, x, s, int(z), w, b, eps)
        scale = np.abs(tw) + np.abs(bias)
        err = np.abs(a - exact)
        assert (err <= 2.0 ** -20 * scale).all(), (C, float((err / scale).max()))
        worst = max(worst, float((err / np.maximum(scale, 1e-300)).max()))
        q = R.out_quantizer(torch.from_numpy(exact[8:]), True, relu=False)
        lv = N.run(kind, x, s, z, w, b, eps, q, torch.float32).numpy().astype(np.int64)
        sc = np.float64(np.float32(float(q[0])))
        c = exact / sc + 128.0
        want = np.clip(np.rint(c), 0, 255).astype(np.int64)
        near = np.abs(c - np.floor(c) - 0.5) <= (2.0 ** -20 * scale) / sc + 2.0 ** -20 * np.abs(c) + 2.0 ** -18
        assert ((lv == want) | (near & (np.abs(lv - want) <= 1))).all(), C
        assert (lv != want).mean() < 1e-3
    print("worst |a - a_exact| / (|t w| + |bias|): 2^%.1f" % np.log2(worst))
    assert worst <= 2.0 ** -20


# ---------------------------------------------------------------------------------------------------
# exact integer statistics
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1024, 8192, 65536])
def test_integer_statistics_rows(C):
    eps = 1e-5
    q = (one(0.01), one(-1.28), (0, 255, 0, 255))
    for x_dtype in N.LEVEL_DTYPES:
        x, at = N.planted(C, x_dtype)
        s, z = one(N.S_X), N.zero_for(x_dtype, 128)
        w, b = N.params(C)
        t = N.run("layer", x, s, z, None, None, eps, None, torch.float32).numpy().astype(np.float64)
        exact, _, _ = N.f64_norm("layer", x, s, int(z), None, None, eps)
        assert (np.abs(t - exact) <= 2.0 ** -20 * np.abs(exact)).all()
        # the single outlier of a row of equal values sits sqrt(C - 1) deviations out, the others 1 / sqrt(C - 1) the other way (eps is
        # small beside a variance of (C - 1) / C^2 level^2 only up to a point: the float64 reference carries it)
        for row, sign in (("one_zero_in_255s", -1), ("one_8_in_7s", 1)):
            r = t[at[row]]
            k = int(np.argmax(np.abs(r)))
            assert np.sign(r[k]) == sign and abs(r[k]) > 0.5 * np.sqrt(C - 1) * (0.02 / np.sqrt(0.02 ** 2 + eps * C)) and len(np.unique(r)) == 2
        alt = t[at["alternating_0_255"]]
        assert np.allclose(np.abs(alt), 1.0, atol=1e-6) and alt[0] < 0 < alt[1]
        # a constant row: V = 0, t = 0 exactly, y = level(bias); with eps = 0 it is 0 * inf = NaN, which goes to quant_min
        assert (t[at["constant"]] == 0).all()
        lv = N.run("layer", x, s, z, w, b, eps, q, torch.float32)
        bias_levels = OPS.lsq_levels_per_tensor(b, q[0], q[1], *q[2], 0).view(torch.uint8)
        assert torch.equal(lv[at["constant"]], bias_levels) and len(bias_levels.unique()) > 16
        lv0 = N.run("layer", x, s, z, w, b, 0.0, (q[0], q[1], (3, 250, 0, 255)), torch.float32)
        assert bool((lv0[at["constant"]] == 3).all()) and len(lv0[at["alternating_0_255"]].unique()) > 8
        # the numpy restatement agrees on every row, for LayerNorm and for RMSNorm at three zero points
        assert np.array_equal(lv.numpy(), N.np_levels(N.np_norm("layer", x, s, int(z), w, b, eps, torch.float32), 0.01, -1.28, q[2]))
        for z_u8 in (0, 3, 128):
            zz = N.zero_for(x_dtype, z_u8)
            got = N.run("rms", x, s, zz, w, b, 1e-6, q, torch.float32)
            assert np.array_equal(got.numpy(), N.np_levels(N.np_norm("rms", x, s, int(zz), w, b, 1e-6, torch.float32), 0.01, -1.28, q[2]))
            e64, tw, bias = N.f64_norm("rms", x, s, int(zz), w, b, 1e-6)
            a = N.run("rms", x, s, zz, w, b, 1e-6, None, torch.float32).numpy().astype(np.float64)
            assert (np.abs(a - e64) <= 2.0 ** -20 * (np.abs(tw) + np.abs(bias))).all()


def test_a_float32_variance_shortcut_changes_levels():
    """mean = sum v / C, var = sum v^2 / C - mean^2 in float32 on the dequantized values: on the row of 7s with a single 8 (levels 121
    below the zero point, C = 1024) the variance, 3.9e-7, comes out of a cancellation at 5.86 whose float32 ulp is 4.8e-7.  The
    shortcut's levels differ from the definition's on nearly the whole row; on a random row they agree"""
    C = 1024
    x, at = N.planted(C)
    s, z = one(N.S_X), one(128, torch.int32)
    w, b = N.params(C)
    q = (one(0.01), one(-1.28), (0, 255, 0, 255))
    good = N.np_levels(N.np_norm("layer", x, s, 128, w, b, 1e-9, torch.float32), 0.01, -1.28, q[2])
    short = N.np_levels(N.np_norm("layer", x, s, 128, w, b, 1e-9, torch.float32, stats="float32"), 0.01, -1.28, q[2])
    got = N.run("layer", x, s, z, w, b, 1e-9, q, torch.float32).numpy()
    assert np.array_equal(got, good)
    row = at["one_8_in_7s"]
    assert (short[row] != good[row]).mean() > 0.9 and (short[0] != good[0]).mean() < 0.01, (short[row] != good[row]).mean()
    # and the definition is right there: float64 agrees with it
    exact, _, _ = N.f64_norm("layer", x, s, 128, w, b, 1e-9)
    want = np.clip(np.rint(exact / np.float64(np.float32(0.01)) + 128.0), 0, 255).astype(np.uint8)
    assert (want[row] != good[row]).mean() < 0.01


def test_product_and_add_are_rounded_apart():
    """six fixed inputs where one fma for t w + bias gives another level than the definition's multiply, then add"""
    q = (one(N.NO_FMA_SCALE), one(0.0), (0, 255, 0, 255))
    total = 0
    for seed in N.NO_FMA_SEEDS:
        x, w, b, at, fused = N.no_fma_case(seed)
        lv = N.run("layer", x, one(N.S_X), one(128, torch.int32), w, b, 1e-5, q, torch.float32)[0].numpy()
        assert len(at) >= 8 and set(lv[at]) <= {0, 2} and (fused == 1).all() and (lv[at] != fused).all(), seed
        assert np.array_equal(lv, N.np_levels(N.np_norm("layer", x, one(N.S_X), 128, w, b, 1e-5, torch.float32), N.NO_FMA_SCALE, 0.0, q[2])[0])
        total += len(at)
    assert total >= 90


def test_a_nan_goes_to_quant_min_and_stays_a_nan_in_the_floats():
    for kind, mid in itertools.product(N.KINDS, N.MIDS):
        x, s, z = N.rows(30, 48), one(N.S_X), one(128, torch.int32)
        w, b = N.params(48)
        w[5] = float("nan")
        for rng in ((3, 200, 0, 255), (-100, 100, -128, 127)):
            lv = N.run(kind, x, s, z, w, b, N.EPS[kind], (one(0.02), one(0.0), rng), mid).to(torch.int64)
            assert bool((lv[:, 5] == rng[0]).all()) and len(lv[:, 4].unique()) > 4
        v = N.run(kind, x, s, z, w, b, N.EPS[kind], None, mid)
        assert bool(v[:, 5].isnan().all()) and not bool(v[:, 4].isnan().any())
    # a NaN output scale: the sanitised scale keeps it, every level is quant_min
    lv = N.run("layer", x, s, z, None, None, 1e-5, (one(float("nan")), one(0.0), (5, 250, 0, 255)), torch.float32)
    assert bool((lv == 5).all())


def test_dim_1_is_dim_minus_1_on_the_permuted_tensor():
    from torchlsq.functional import LevelsTensor, lsq_layer_norm_w8, lsq_layer_norm_w8_q, lsq_rms_norm_w8, lsq_rms_norm_w8_q
    rows = N.rows(2 * 5 * 7, 48).reshape(2, 5, 7, 48)
    x = rows.permute(0, 3, 1, 2)
    assert x.is_contiguous(memory_format=CL)
    s, z = one(N.S_X), one(128, torch.int32)
    w, b = N.params(48)
    q = N.quantizer_for("layer", rows, s, z, w, b, 1e-6, False)
    X, Xr = LevelsTensor(x, s, z, 0, 255), LevelsTensor(rows, s, z, 0, 255)
    for fq, ff in ((lsq_layer_norm_w8_q, lsq_layer_norm_w8), (lsq_rms_norm_w8_q, lsq_rms_norm_w8)):
        a = fq(X, w, b, 1e-6, q[0], q[1], -128, 127, mid_dtype=torch.bfloat16, dim=1)
        c = fq(Xr, w, b, 1e-6, q[0], q[1], -128, 127, mid_dtype=torch.bfloat16)
        assert a.levels.shape == (2, 48, 5, 7) and a.levels.is_contiguous(memory_format=CL) and a.levels.dtype == torch.int8
        assert torch.equal(a.levels.permute(0, 2, 3, 1), c.levels) and len(c.levels.unique()) > 64
        assert (a.quant_min, a.quant_max) == (-128, 127) and torch.equal(a.scale, c.scale) and torch.equal(a.zero_point, c.zero_point)
        v = ff(X, w, b, 1e-6, torch.float16, dim=1)
        assert v.is_contiguous(memory_format=CL) and torch.equal(v.permute(0, 2, 3, 1), ff(Xr, w, b, 1e-6, torch.float16))
    # a levels tensor that is NOT in channels-last memory is read as if it were: the same values
    a = lsq_layer_norm_w8(LevelsTensor(x.contiguous(), s, z, 0, 255), w, b, 1e-6, dim=1)
    assert torch.equal(a, lsq_layer_norm_w8(X, w, b, 1e-6, dim=1))


# ---------------------------------------------------------------------------------------------------
# the modules and the converter
# ---------------------------------------------------------------------------------------------------
def test_state_dict_round_trips():
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import LayerNormW8Q, RMSNormW8Q
    net, qs, x = N.cn_block()
    m = LayerNormW8Q.from_float(net.norm, qs["n"], mid_dtype=torch.bfloat16, channels_first=True)
    assert {"weight", "bias", "output_scale", "output_shift"} == set(dict(m.named_buffers()))
    assert (m.eps, m.dim, m.levels_out, m.normalized_shape) == (1e-6, 1, True, (16,)) and torch.equal(m.weight, net.norm.weight.detach())
    fresh = LayerNormW8Q(16)
    fresh.load_state_dict(m.state_dict())
    assert (fresh.eps, fresh.dim, fresh.mid_dtype, fresh.output_range, fresh.levels_out) == (1e-6, 1, torch.bfloat16, m.output_range, True)
    assert torch.equal(fresh.weight, m.weight) and torch.equal(fresh.output_scale, qs["n"].scale.detach().reshape(1))
    assert "dim=1" in repr(fresh) and "output levels" in repr(fresh) and "mid_dtype=bfloat16" in repr(fresh)
    with torch.no_grad():
        d = net.dw(qs["in"](x))
    dl = LevelsTensor.from_quantized(qs["d"].quantize(d).contiguous(memory_format=CL))       # as the depthwise layer hands it on
    want = m(dl)
    assert isinstance(want, LevelsTensor) and torch.equal(fresh(dl).levels, want.levels) and len(want.levels.unique()) > 32
    assert want.levels.shape == dl.shape and want.levels.stride() == dl.levels.stride()
    # no output quantizer: floats of mid_dtype; an RMSNorm without bias; a norm without parameters
    f = LayerNormW8Q.from_float(net.norm, None, mid_dtype=torch.float16, channels_first=True)
    v = f(dl)
    assert v.dtype == torch.float16 and v.shape == dl.shape and not f.levels_out and "floats out" in repr(f)
    rms = torch.nn.RMSNorm(16, eps=None)
    with torch.no_grad():
        rms.weight.copy_(N.params(16)[0])
    r = RMSNormW8Q.from_float(rms, qs["n"], channels_first=True)
    assert r.bias.numel() == 0 and r.eps == torch.finfo(torch.float32).eps and isinstance(r(dl), LevelsTensor)
    fresh = RMSNormW8Q(16, bias=False)
    fresh.load_state_dict(r.state_dict())
    assert torch.equal(fresh(dl).levels, r(dl).levels) and fresh.eps == r.eps
    plain = LayerNormW8Q.from_float(torch.nn.LayerNorm(16, elementwise_affine=False), qs["n"], channels_first=True)
    assert plain.weight.numel() == 0 and plain.bias.numel() == 0 and isinstance(plain(dl), LevelsTensor)
    with pytest.raises(ValueError, match="LSQFakeQuantizer"):
        LayerNormW8Q.from_float(net.norm, torch.nn.Identity())
    with pytest.raises(AssertionError, match="reads levels"):
        m(d)


def _share(a, b):
    d = (a.to(torch.int64) - b.to(torch.int64)).abs()
    return int(d.max()), float((d > 0).double().mean())


@pytest.mark.parametrize("mid", N.MIDS, ids=N.name)
def test_convert_w8a8_norm_on_a_convnext_block_equals_the_modules_written_out(mid):
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import (ActivationW8Q, AddW8A8Q, Conv2dW8A8AddQ, Conv2dW8A8Q, DepthwiseConv2dW8A8Q, LayerNormW8Q,
                                    convert_w8a8_norm)
    net, qs, x = N.cn_block()
    new = N.convert_cn_block(net, qs, mid)
    assert isinstance(new.dw, DepthwiseConv2dW8A8Q) and isinstance(new.norm, LayerNormW8Q) and isinstance(new.pw1, Conv2dW8A8Q)
    assert isinstance(new.act, ActivationW8Q) and isinstance(new.pw2, Conv2dW8A8AddQ) and isinstance(new.add, AddW8A8Q)
    assert (new.norm.dim, new.norm.mid_dtype, new.norm.eps) == (1, mid, 1e-6) and isinstance(net.norm, N.LayerNorm2d)        # a deep copy
    xl = LevelsTensor.from_quantized(qs["in"].quantize(x))
    got = new(xl)
    want, mids = N.cn_block_written_out(net, qs, xl, mid)
    assert isinstance(got, LevelsTensor) and got.levels.shape == (2, 16, 9, 7) and torch.equal(got.levels, want.levels)
    assert len(want.levels.unique()) > 64 and all(len(v.levels.unique()) > 32 for v in mids.values())
    # the norm step against F.layer_norm of the dequantized values taken to levels: at most one level apart
    with torch.no_grad():
        chain = qs["n"].quantize(net.norm(mids["d"].dequantize(torch.float32)).to(mid)).int_repr()
    worst, share = _share(chain, mids["n"].levels)
    print("convnext block, %s: %.3f %% of the norm's levels differ from F.layer_norm's, by at most %d" % (N.name(mid), 100 * share, worst))
    assert worst <= 1
    # refusals of the converter, by name
    with pytest.raises(ValueError, match="'dw' is not an nn.LayerNorm or nn.RMSNorm"):
        convert_w8a8_norm(net, {"dw": qs["d"]})
    with pytest.raises(ValueError, match="'nowhere' is not an nn.LayerNorm"):
        convert_w8a8_norm(net, {"nowhere": qs["d"]})
    with pytest.raises(ValueError, match="channels_first names .'pw1'. are not among"):
        convert_w8a8_norm(net, {"norm": qs["n"]}, channels_first=("pw1",))
    with pytest.raises(ValueError, match="LSQFakeQuantizer"):
        convert_w8a8_norm(net, {"norm": torch.nn.Identity()})
    big = torch.nn.Sequential(torch.nn.LayerNorm(65537))
    with pytest.raises(ValueError, match="'0' cannot be served: .*at most 65536"):
        convert_w8a8_norm(big, {"0": qs["n"]})
    gn = torch.nn.Sequential(torch.nn.GroupNorm(2, 16))
    with pytest.raises(ValueError, match="GroupNorm and BatchNorm are not served"):
        convert_w8a8_norm(gn, {"0": qs["n"]})
    only = convert_w8a8_norm(net, {"norm": None}, channels_first=("norm",), mid_dtype=mid)
    assert isinstance(only.norm, LayerNormW8Q) and not only.norm.levels_out and isinstance(only.pw1, type(net.pw1))


@pytest.mark.parametrize("mid", N.MIDS, ids=N.name)
def test_convert_w8a8_norm_on_a_token_block_equals_the_modules_written_out(mid):
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import AddW8A8Q, LayerNormW8Q, LinearW8A8AddQ, LinearW8A8Q
    net, qs, x = N.token_block()
    new = N.convert_token_block(net, qs, mid)
    assert isinstance(new.proj, LinearW8A8AddQ) and isinstance(new.add, AddW8A8Q) and isinstance(new.norm, LayerNormW8Q)
    assert isinstance(new.fc1, LinearW8A8Q) and new.norm.dim == -1
    xl = LevelsTensor.from_quantized(qs["in"].quantize(x))
    got = new(xl)
    want, mids = N.token_block_written_out(net, qs, xl, mid)
    assert isinstance(got, LevelsTensor) and got.levels.shape == (2, 10, 96) and torch.equal(got.levels, want.levels)
    assert len(want.levels.unique()) > 64 and all(len(v.levels.unique()) > 32 for v in mids.values())
    with torch.no_grad():
        chain = qs["n"].quantize(net.norm(mids["a"].dequantize(torch.float32)).to(mid)).int_repr()
    worst, share = _share(chain, mids["n"].levels)
    print("token block, %s: %.3f %% of the norm's levels differ from F.layer_norm's, by at most %d" % (N.name(mid), 100 * share, worst))
    assert worst <= 1
