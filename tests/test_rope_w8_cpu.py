"""Rotary embedding and the KV-cache append on 8-bit levels (include/lsq_hip_rope_w8.h), everything that needs no GPU: the library's
exports against its header and `_abi.py`, its kernel set and their resources, every refusal, the plan on both sides of every
threshold, and the CPU path -- the definition the GPU tests compare against -- held to an independent numpy restatement, to the
composition of existing ops, to the derived bound against float64, with the placement, the decode that equals the prefill, the fake
kernels and the modules on top.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rope_w8_cases as C
from helpers import demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_rope_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_rope_w8.so")
NAMES = sorted(["lsq_rope_w8_abi_version", "lsq_rope_w8_last_error", "lsq_rope_w8", "lsq_rope_w8_plan"])
LSQ_EINVAL = -1
OPS = torch.ops.torchlsq
U8, I8, F32, BF16, F16 = C.U8, C.I8, C.F32, C.BF16, C.F16
one = C.one


# ---------------------------------------------------------------------------------------------------
# 1: the library
# ---------------------------------------------------------------------------------------------------
def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_rope_w8\w*)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_ROPE_W8) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_", "lsq_requant_", "lsq_resadd_",
                  "lsq_pool_", "lsq_dwconv_", "lsq_eltwise_", "lsq_norm_", "lsq_attn_", "lsq_bmm_", "lsq_softmax_", "lsq_rope_"):
        assert other not in und, other
    assert E.rope_w8_library().lsq_rope_w8_abi_version() == E.ROPE_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_ROPE_W8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    for name, cls, size in (("lsq_rope_w8_geom", E.LsqRopeW8Geom, 17 * 8), ("lsq_rope_w8_in", E.LsqRopeW8In, 16), ("lsq_rope_w8_out", E.LsqRopeW8Out, 56)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        fields = [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(?:int64_t|const void\*)", "", decl.strip()).split(",") if f.strip()]
        assert fields == [f[0] for f in cls._fields_] and ctypes.sizeof(cls) == size, name


def test_kernels(tmp_path):
    """the five kernels: no scratch, no LDS use, no atomics, packet loads and stores in the packets kernels, and no fused
    multiply-add outside the one correctly rounded division 1 / out_scale of the output side -- so none in the rotation, whatever mid"""
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    short = {}
    for sym, dm in names.items():
        m = re.match(r"^(?:void )?lsq::(rope_w8_\w+)_kernel(?:<([^>]*)>)?\(", dm)
        assert m, "not a kernel of this library: %s" % dm
        short[sym] = m.group(1) + ("" if m.group(2) is None else "_" + re.sub(r"\(bool\)", "", m.group(2)).replace("true", "1").replace("false", "0"))
    assert sorted(short.values()) == sorted(["rope_w8_generic", "rope_w8_copy_generic", "rope_w8_copy_packets", "rope_w8_packets_0", "rope_w8_packets_1"])
    for sym, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0, "%s uses %d bytes of scratch" % (sym, scratch)
        assert not any("atomic" in o or o.startswith("ds_") or o == "s_barrier" for o in ops), sym
        fused = [i for i, o in enumerate(ops) if re.match(r"v_(pk_)?(fma|fmac|mad|mac)_(f32|f16|legacy)", o) or o == "v_div_fmas_f32"]
        if short[sym].startswith("rope_w8_copy"):
            assert not fused and "v_div_fixup_f32" not in ops, sym        # (the 32-bit index divisions multiply floats; nothing else does)
        else:
            # one division: its fmas lie between the first v_div_scale_f32 and the v_div_fixup_f32, and there are no others
            assert ops.count("v_div_fixup_f32") == 1 and ops.count("v_rcp_f32_e32") == 1, sym
            lo, hi = ops.index("v_div_scale_f32"), ops.index("v_div_fixup_f32")
            assert fused and all(lo < i < hi for i in fused), (sym, [(i, ops[i]) for i in fused])
            assert any(o.startswith("v_mul_f32") for o in ops[hi:]) and any(o.startswith("v_sub_f32") for o in ops[hi:]), sym
        if "packets" in short[sym]:
            assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops, sym
        if short[sym] == "rope_w8_packets_0":
            assert ops.count("global_load_dwordx4") >= 10, sym        # 4 + 4 of the tables, the pair of packets


# ---------------------------------------------------------------------------------------------------
# 2: refusals
# ---------------------------------------------------------------------------------------------------
def _geom(E, **kw):
    base = dict(B=2, T=5, H=3, D=32, R=32, P=16, Tout=5, x_sb=480, x_st=96, x_sh=32, y_sb=480, y_st=96, y_sh=32, x_dtype=0, style=0, scatter=0, mode=0)
    base.update(kw)
    return E.LsqRopeW8Geom(*[base[f[0]] for f in E.LsqRopeW8Geom._fields_])


def test_library_refusals():
    from torchlsq import extension as E
    lib = E.rope_w8_library()
    out = (ctypes.c_int32 * 8)()

    def err():
        return lib.lsq_rope_w8_last_error()

    def plan(g, aligned=1, o=out):
        return lib.lsq_rope_w8_plan(ctypes.byref(g) if g is not None else None, aligned, ctypes.byref(o) if o is not None else None)
    assert plan(_geom(E)) == 0 and list(out) == [1, 1, 256, 1, 1, 1, 0, 1]
    assert plan(None) == LSQ_EINVAL and b"NULL geometry" in err()
    assert plan(_geom(E), o=None) == LSQ_EINVAL and b"NULL output" in err()
    assert plan(_geom(E), aligned=3) == LSQ_EINVAL and b"aligned must be 0 or the bytes" in err()
    assert plan(_geom(E, mode=1), aligned=2) == LSQ_EINVAL and b"aligned must be 0 or 1" in err()
    assert plan(_geom(E, x_dtype=2)) == LSQ_EINVAL and b"x_dtype must be" in err()
    assert plan(_geom(E, mode=2)) == LSQ_EINVAL and b"mode must be" in err()
    assert plan(_geom(E, style=2)) == LSQ_EINVAL and b"style must be" in err()
    assert plan(_geom(E, style=2, mode=1)) == 0                                     # COPY does not read style, R or P
    assert plan(_geom(E, scatter=2)) == LSQ_EINVAL and b"scatter must be 0 or 1" in err()
    for name in ("B", "T", "H", "D", "Tout"):
        for bad in (0, -1):
            assert plan(_geom(E, **{name: bad})) == LSQ_EINVAL and b"every extent must be at least 1" in err(), name
        assert plan(_geom(E, **{name: 1 << 29})) == LSQ_EINVAL and b"beyond 29 bits" in err(), name
    assert plan(_geom(E, P=0)) == LSQ_EINVAL and b"at least 1 is needed" in err()
    assert plan(_geom(E, P=1 << 29)) == LSQ_EINVAL and b"P = 536870912 is beyond 29 bits" in err()
    assert plan(_geom(E, B=1 << 20, T=1 << 20, Tout=1 << 20)) == LSQ_EINVAL and b"beyond 2^40 elements" in err()
    for R in (0, 1, 3, 31, 34, -2):
        assert plan(_geom(E, R=R)) == LSQ_EINVAL and b"must be even, at least 2 and at most D = 32" in err(), R
    assert plan(_geom(E, R=2)) == 0 and plan(_geom(E, R=30)) == 0
    assert plan(_geom(E, Tout=4)) == LSQ_EINVAL and b"Tout = 4 must be at least T = 5" in err()
    assert plan(_geom(E, Tout=4, scatter=1, y_sb=384)) == 0
    assert plan(_geom(E, x_st=-96)) == LSQ_EINVAL and b"must not be negative" in err()
    assert plan(_geom(E, y_sb=1 << 58)) == LSQ_EINVAL and b"within 2^58" in err()
    # overlapping output rows: a head stride below D, a token stride inside a head's rows, batches on top of each other
    for kw in (dict(y_sh=31), dict(y_st=64), dict(y_sb=479), dict(y_sb=0), dict(y_sh=16, y_st=48)):
        assert plan(_geom(E, **kw)) == LSQ_EINVAL and b"two rows of D = 32 elements overlap" in err(), kw
    assert plan(_geom(E, Tout=12, y_sb=1152, y_sh=384, y_st=32)) == 0               # the [B, H, Tmax, D] cache seen as [B, Tmax, H, D]
    big = dict(B=(1 << 16) + 1, T=1 << 16, Tout=1 << 16, H=1, D=16, x_sb=1 << 20, x_st=16, x_sh=16, y_sb=1 << 20, y_st=16, y_sh=16)
    assert plan(_geom(E, style=1, R=16, **big)) == LSQ_EINVAL and b"workgroups are beyond 2^24 - 1" in err()
    assert plan(_geom(E, style=1, R=16, **dict(big, B=1 << 15))) == 0 and out[1] == 1 << 23

    x, y = torch.zeros(2 * 5 * 96 + 64, dtype=U8), torch.zeros(4 * (2 * 5 * 96 + 64), dtype=U8)
    cos, sin, pos = torch.zeros(16 * 16 + 4), torch.zeros(16 * 16 + 4), torch.zeros(4, dtype=torch.int32)
    s, z = torch.ones(4), torch.zeros(4, dtype=torch.int32)

    def side(**kw):
        base = dict(s_x=s.data_ptr(), zx=z.data_ptr())
        base.update(kw)
        return E.LsqRopeW8In(base["s_x"], base["zx"])

    def outq(**kw):
        base = dict(out_scale=s.data_ptr(), out_shift=s.data_ptr() + 4, quant_min=0, quant_max=255, type_min=0, type_max=255, mid_dtype=E.LSQ_F32)
        base.update(kw)
        return E.LsqRopeW8Out(*[base[f[0]] for f in E.LsqRopeW8Out._fields_])

    def call(g=None, i=None, o=None, cp=cos.data_ptr(), sp=sin.data_ptr(), pp=pos.data_ptr(), xp=x.data_ptr(), yp=y.data_ptr(), no=()):
        g = _geom(E) if g is None else g
        i = side() if i is None else i
        o = outq() if o is None else o
        return lib.lsq_rope_w8(None if "g" in no else ctypes.byref(g), None if "i" in no else ctypes.byref(i), None if "o" in no else ctypes.byref(o),
                               cp, sp, pp, xp, yp, None)
    # NULL pointers where one is needed
    assert call(no="g") == LSQ_EINVAL and b"NULL geometry" in err()
    assert call(no="i") == LSQ_EINVAL and b"NULL input side" in err()
    assert call(i=side(s_x=None)) == LSQ_EINVAL and b"NULL input side, s_x or zx" in err()
    assert call(i=side(zx=None)) == LSQ_EINVAL and b"NULL input side, s_x or zx" in err()
    assert call(no="o") == LSQ_EINVAL and b"NULL output description" in err()
    assert call(cp=None) == LSQ_EINVAL and b"NULL cos or sin" in err()
    assert call(sp=None) == LSQ_EINVAL and b"NULL cos or sin" in err()
    assert call(xp=None) == LSQ_EINVAL and b"NULL buffer" in err()
    assert call(yp=None) == LSQ_EINVAL and b"NULL buffer" in err()
    assert call(o=outq(out_shift=None)) == LSQ_EINVAL and b"they come together" in err()
    # misaligned constants, tables, positions, a floating y
    assert call(i=side(s_x=s.data_ptr() + 2)) == LSQ_EINVAL and b"s_x and zx must be element-aligned" in err()
    assert call(i=side(zx=z.data_ptr() + 1)) == LSQ_EINVAL and b"s_x and zx must be element-aligned" in err()
    assert call(o=outq(out_scale=s.data_ptr() + 2)) == LSQ_EINVAL and b"out_scale and out_shift must be element-aligned" in err()
    assert call(cp=cos.data_ptr() + 2) == LSQ_EINVAL and b"cos and sin must be element-aligned" in err()
    assert call(sp=sin.data_ptr() + 1) == LSQ_EINVAL and b"cos and sin must be element-aligned" in err()
    assert call(pp=pos.data_ptr() + 2) == LSQ_EINVAL and b"positions must be 4-byte aligned" in err()
    assert call(o=outq(out_scale=None, out_shift=None), yp=y.data_ptr() + 2) == LSQ_EINVAL and b"a floating y must be element-aligned" in err()
    # the geometry again, through the launching entry point
    assert call(g=_geom(E, R=3)) == LSQ_EINVAL and b"must be even" in err()
    assert call(g=_geom(E, Tout=4)) == LSQ_EINVAL and b"must be at least T" in err()
    assert call(g=_geom(E, y_sh=31)) == LSQ_EINVAL and b"overlap" in err()
    # y on x, the tables, positions
    assert call(yp=x.data_ptr() + 959) == LSQ_EINVAL and b"the op in place is not served" in err()
    assert call(yp=cos.data_ptr()) == LSQ_EINVAL and b"bytes of cos or sin" in err()
    assert call(yp=sin.data_ptr() + 1020) == LSQ_EINVAL and b"bytes of cos or sin" in err()
    big = torch.zeros(600, dtype=torch.int32)
    assert call(pp=big.data_ptr() + 4 * 250, yp=big.data_ptr() + 48) == LSQ_EINVAL and b"overlap the 2 entries of positions" in err()
    # a bad mid, a bad range
    assert call(o=outq(mid_dtype=7)) == LSQ_EINVAL and b"mid_dtype must be" in err()
    assert call(o=outq(mid_dtype=E.LSQ_F64)) == LSQ_EINVAL and b"mid_dtype must be" in err()
    for kw in (dict(quant_min=-1), dict(quant_max=256), dict(quant_min=9, quant_max=3), dict(type_min=-129, type_max=0, quant_min=-5, quant_max=5)):
        assert call(o=outq(**kw)) == LSQ_EINVAL and b"must lie within" in err(), kw
    # COPY with anything given
    cg = _geom(E, mode=1)
    for cp_, sp_ in ((cos.data_ptr(), None), (None, sin.data_ptr())):
        assert lib.lsq_rope_w8(ctypes.byref(cg), None, None, cp_, sp_, None, x.data_ptr(), y.data_ptr(), None) == LSQ_EINVAL
        assert b"the input side, the output side, cos and sin must be NULL" in err()
    assert lib.lsq_rope_w8(ctypes.byref(cg), ctypes.byref(side()), None, None, None, None, x.data_ptr(), y.data_ptr(), None) == LSQ_EINVAL
    assert b"must be NULL" in err()
    assert lib.lsq_rope_w8(ctypes.byref(cg), None, ctypes.byref(outq()), None, None, None, x.data_ptr(), y.data_ptr(), None) == LSQ_EINVAL
    assert b"must be NULL" in err()
    assert lib.lsq_rope_w8(ctypes.byref(cg), None, None, None, None, None, x.data_ptr(), x.data_ptr() + 100, None) == LSQ_EINVAL and b"in place" in err()


def test_op_and_functional_refusals():
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, lsq_kv_append_w8, lsq_rope_tables, lsq_rope_w8, lsq_rope_w8_q
    x, consts = C.levels((2, 5, 3, 32), 0), C.constants(U8)
    cos, sin = C.tables(32, 16, F32)
    pos = torch.tensor([0, 3], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="levels must be uint8"):
        OPS.lsq_rope_w8_q8(x.float(), *consts, cos, sin, F32)
    with pytest.raises(RuntimeError, match=r"must be \[B, T, H, D\]"):
        OPS.lsq_rope_w8_q8(x[0], *consts, cos, sin, F32)
    with pytest.raises(RuntimeError, match="x_scale must be one float32 value"):
        OPS.lsq_rope_w8_q8(x, torch.ones(2), consts[1], cos, sin, F32)
    for bad_c, bad_s in ((cos.double(), sin.double()), (cos, sin[:, :8]), (cos.t(), sin.t()), (cos[0], sin[0])):
        with pytest.raises(RuntimeError, match="cos and sin must be dense float32 tensors of one shape"):
            OPS.lsq_rope_w8_q8(x, *consts, bad_c, bad_s, F32)
    for bad in (pos.long(), pos[:1], torch.zeros(4, dtype=torch.int32)[::2], pos.reshape(2, 1)):
        with pytest.raises(RuntimeError, match="positions must be a dense int32 tensor of"):
            OPS.lsq_rope_w8_q8_q(x, *consts, cos, sin, *C.OUT_U8, F32, bad)
    with pytest.raises(RuntimeError, match="positions must be on the levels' device"):
        E.rope_w8(x, *consts, cos, sin, F32, pos.to("meta"))
    with pytest.raises(RuntimeError, match="out_dtype must be float32"):
        OPS.lsq_rope_w8_q8(x, *consts, cos, sin, torch.float64)
    with pytest.raises(RuntimeError, match=r"must lie within 0..255 or within -128..127"):
        OPS.lsq_rope_w8_q8_q(x, *consts, cos, sin, C.OUT_U8[0], C.OUT_U8[1], -1, 255, 0, 255, F32)
    with pytest.raises(RuntimeError, match=r"lsq_rope_w8_q8 failed \(-1\).*at most D = 32"):
        OPS.lsq_rope_w8_q8(x, *consts, *C.tables(34, 16, F32), F32)
    with pytest.raises(RuntimeError, match="scatter needs `out`"):
        E.rope_w8(x, *consts, cos, sin, F32, None, False, None, True)
    with pytest.raises(RuntimeError, match="`out` must be a int8 tensor"):
        E.rope_w8_q(x, *consts, cos, sin, *C.OUT_I8, F32, out=torch.zeros(x.shape, dtype=U8))
    with pytest.raises(RuntimeError, match=r"`out` must be a uint8 tensor of shape \[2, Tout, 3, 32\]"):
        E.rope_w8_q(x, *consts, cos, sin, *C.OUT_U8, F32, out=torch.zeros((2, 5, 3, 16), dtype=U8))
    with pytest.raises(RuntimeError, match="Tout = 4 must be at least T = 5"):
        E.rope_w8_q(x, *consts, cos, sin, *C.OUT_U8, F32, out=torch.zeros((2, 4, 3, 32), dtype=U8))
    with pytest.raises(RuntimeError, match="two rows of D = 32 elements overlap"):
        E.rope_w8_q(x, *consts, cos, sin, *C.OUT_U8, F32, out=torch.zeros((1, 5, 3, 32), dtype=U8).expand(2, 5, 3, 32))
    # `out` on top of an input: refused on the host, on the CPU as the library refuses it on the GPU
    room = torch.zeros(2 * 5 * 3 * 32 + 64, dtype=U8)
    xin = room[:960].view(2, 5, 3, 32)
    with pytest.raises(RuntimeError, match="`out` overlaps x: the op in place is not served"):
        E.rope_w8_q(xin, *consts, cos, sin, *C.OUT_U8, F32, out=room[32:992].view(2, 5, 3, 32))
    with pytest.raises(RuntimeError, match="`out` overlaps x"):
        OPS.lsq_kv_copy_w8(xin, xin, None, False)
    with pytest.raises(RuntimeError, match="`out` overlaps cos"):
        E.rope_w8(C.levels((1, 1, 1, 32), 0), *consts, cos, sin, F32, out=cos.view(-1)[32:64].view(1, 1, 1, 32))
    ipos = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="`out` overlaps positions"):
        OPS.lsq_kv_copy_w8(C.levels((2, 1, 1, 8), 0, I8), ipos.view(I8)[:16].view(2, 1, 1, 8), ipos[:2], False)
    E.rope_w8_q(xin, *consts, cos, sin, *C.OUT_U8, F32, out=torch.zeros_like(xin))       # (a separate `out` is served)
    # COPY
    with pytest.raises(RuntimeError, match="x and `out` must have one level dtype"):
        OPS.lsq_kv_copy_w8(x, torch.zeros(x.shape, dtype=I8), None, False)
    with pytest.raises(RuntimeError, match=r"of shape \[2, Tout, 3, 32\]"):
        OPS.lsq_kv_copy_w8(x, torch.zeros((2, 5, 4, 32), dtype=U8), None, False)
    with pytest.raises(RuntimeError, match="must be at least T"):
        OPS.lsq_kv_copy_w8(x, torch.zeros((2, 3, 3, 32), dtype=U8), None, False)
    # the functions
    lt = LevelsTensor(x, *consts, 0, 255)
    with pytest.raises(AssertionError, match="scatter needs `out`"):
        lsq_rope_w8_q(lt, cos, sin, *C.OUT_U8, scatter=True)
    with pytest.raises(AssertionError, match=r"needs levels of \[B, T, H, D\]"):
        lsq_rope_w8(LevelsTensor(x[0], *consts, 0, 255), cos, sin)
    with pytest.raises(AssertionError, match=r"needs levels of \[B, T, H, D\]"):
        lsq_kv_append_w8(LevelsTensor(x[0], *consts, 0, 255), torch.zeros_like(x))
    with pytest.raises(AssertionError, match="needs the output quantizer"):
        lsq_rope_w8_q(lt, cos, sin)
    for bad in (dict(dim=3), dict(dim=0), dict(max_positions=0), dict(mid_dtype=torch.float64)):
        kw = dict(dim=8, max_positions=4)
        kw.update(bad)
        with pytest.raises(AssertionError, match="lsq_rope_tables"):
            lsq_rope_tables(**kw)
    # inference only
    with pytest.raises(RuntimeError, match="grad|inference"):
        OPS.lsq_rope_w8_q8_q(x, *consts, cos, sin, C.OUT_U8[0].clone().requires_grad_(True), *C.OUT_U8[1:], F32)
    with pytest.raises(RuntimeError, match="grad|inference"):
        OPS.lsq_rope_w8_q8(x, consts[0].clone().requires_grad_(True), consts[1], cos, sin, F32)


# ---------------------------------------------------------------------------------------------------
# 3: the plan on both sides of every threshold
# ---------------------------------------------------------------------------------------------------
def test_plan_thresholds():
    from torchlsq import extension as E
    P = E.rope_w8_plan
    pk = dict(family="packets", grid=1, block=256, heads_per_lane=1, lds_bytes=0)
    assert P(2, 5, 3, 32, P=16) == dict(pk, units=1, rotating_units=1, kernel="packets_half")
    assert P(2, 5, 3, 128, P=16) == dict(pk, units=4, rotating_units=4, kernel="packets_half")
    assert P(2, 5, 3, 64, R=32, P=16) == dict(pk, units=3, rotating_units=1, kernel="packets_half")
    assert P(2, 5, 3, 16, P=16, interleaved=True) == dict(pk, units=1, rotating_units=1, kernel="packets_interleaved")
    assert P(2, 5, 3, 64, R=16, P=16, interleaved=True) == dict(pk, units=4, rotating_units=1, kernel="packets_interleaved")
    # D % 16
    for D in (15, 17, 24, 6):
        assert P(2, 5, 3, D, R=4, P=16)["kernel"] == "generic" and P(2, 5, 3, D, copy=True)["kernel"] == "copy_generic", D
    assert P(2, 5, 3, 6, R=4, P=16) == dict(family="generic", grid=1, block=256, heads_per_lane=1, units=4, rotating_units=2, lds_bytes=0, kernel="generic")
    # R % 32 for the half style, R % 16 for the interleaved one
    for R, half, inter in ((32, "packets_half", "packets_interleaved"), (16, "generic", "packets_interleaved"), (48, "generic", "packets_interleaved"),
                           (64, "packets_half", "packets_interleaved"), (8, "generic", "generic"), (40, "generic", "generic")):
        assert P(2, 5, 3, 64, R=R, P=16)["kernel"] == half and P(2, 5, 3, 64, R=R, P=16, interleaved=True)["kernel"] == inter, R
    # each alignment class: the bases, every stride of x, every stride of y in bytes of its element
    assert P(2, 5, 3, 32, P=16, aligned=False)["family"] == "generic" and P(2, 5, 3, 32, copy=True, aligned=False)["kernel"] == "copy_generic"
    for bad, good in (((504, 96, 32), (512, 96, 32)), ((640, 104, 32), (640, 112, 32)), ((640, 128, 40), (800, 160, 48))):
        for which in ("x_strides", "y_strides"):
            assert P(2, 5, 3, 32, P=16, **{which: bad})["family"] == "generic", (which, bad)
            assert P(2, 5, 3, 32, copy=True, **{which: bad})["family"] == "generic", (which, bad)
            assert P(2, 5, 3, 32, P=16, **{which: good})["family"] == "packets", (which, good)
            assert P(2, 5, 3, 32, copy=True, **{which: good})["kernel"] == "copy_packets", (which, good)
    wide = (5 * 3 * 36, 3 * 36, 36)          # 36 elements: 144 bytes of float32, 72 of bfloat16, 36 of levels
    assert [P(2, 5, 3, 32, P=16, y_strides=wide, y_elem=e)["family"] for e in (4, 2, 1)] == ["packets", "generic", "generic"]
    wide = (5 * 3 * 40, 3 * 40, 40)
    assert [P(2, 5, 3, 32, P=16, y_strides=wide, y_elem=e)["family"] for e in (4, 2, 1)] == ["packets", "packets", "generic"]
    # heads per lane: min(H, 4), halved while the grid holds fewer than two workgroups per compute unit (512 on 256 compute units)
    fill = 2 * 256
    for H, start in ((8, 4), (6, 4), (3, 3), (2, 2), (1, 1)):
        groups = -(-H // start)
        tokens = fill * 256 // groups               # D = 32, half style: one unit per head
        full = P(1, tokens, H, 32, P=16)
        assert (full["heads_per_lane"], full["grid"]) == (start, fill), (H, full)
        less = P(1, (fill - 1) * 256 // groups, H, 32, P=16)          # one workgroup fewer
        assert less["heads_per_lane"] == start // 2 or start == 1, (H, less)
    assert P(1, fill * 256 // 4, 8, 32, P=16)["heads_per_lane"] == 2 and P(1, fill * 256 // 8 - 1, 8, 32, P=16)["heads_per_lane"] == 1
    assert P(4, 1024, 32, 128, P=2048) == dict(pk, grid=512, heads_per_lane=4, units=4, rotating_units=4, kernel="packets_half")
    assert P(4, 1024, 8, 128, P=2048)["heads_per_lane"] == 1 and P(32, 1, 32, 128, P=2048, Tout=2048, scatter=True)["heads_per_lane"] == 1
    # COPY
    assert P(32, 1, 32, 128, Tout=2048, y_strides=(32 * 2048 * 128, 128, 2048 * 128), scatter=True, copy=True) == \
        dict(family="packets", grid=32, block=256, heads_per_lane=1, units=8, rotating_units=0, lds_bytes=0, kernel="copy_packets")
    assert P(2, 5, 3, 6, copy=True) == dict(family="generic", grid=1, block=256, heads_per_lane=1, units=6, rotating_units=0, lds_bytes=0,
                                            kernel="copy_generic")


# ---------------------------------------------------------------------------------------------------
# 4 - 6: the CPU path against numpy, against the existing ops composed, interleaved against half
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [U8, I8], ids=str)
@pytest.mark.parametrize("mid", [F32, BF16, F16], ids=str)
@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
@pytest.mark.parametrize("D,R", [(32, 32), (64, 32), (6, 4)], ids=str)
def test_cpu_path_equals_the_numpy_restatement(dtype, mid, interleaved, D, R):
    x, consts = C.levels((2, 5, 3, D), D + R, dtype), C.constants(dtype)
    cos, sin = C.tables(R, 16, mid)
    assert torch.equal(cos, cos.to(mid).to(F32)) and tuple(cos.shape) == (16, R // 2)
    pos = [2, 11]
    u = C.numpy_value(x, consts, cos, sin, mid, pos, interleaved)
    assert not np.isnan(u).any() and len(np.unique(u)) > 50
    for q in (C.OUT_U8, C.OUT_I8, None):
        C.same(C.run_rope("cpu", x, consts, cos, sin, q, mid, pos, interleaved), C.finish(u, q, mid), (q is None,))


@pytest.mark.parametrize("dtype", [U8, I8], ids=str)
@pytest.mark.parametrize("mid", [F32, BF16, F16], ids=str)
@pytest.mark.parametrize("D,R", [(32, 32), (64, 32)], ids=str)
def test_cpu_path_equals_the_existing_ops_composed(dtype, mid, D, R):
    x, consts = C.levels((2, 5, 3, D), 40 + D, dtype), C.constants(dtype)
    cos, sin = C.tables(R, 16, mid)
    for q in (C.OUT_U8, C.OUT_I8, None):
        C.same(C.run_rope("cpu", x, consts, cos, sin, q, mid, [0, 7]), C.hf_composed(x, consts, cos, sin, q, mid, [0, 7]), (q is None,))
    from torchlsq.functional import LevelsTensor, lsq_rope_w8, lsq_rope_w8_q
    lt = LevelsTensor(x, *consts, 0, 255)
    y = lsq_rope_w8_q(lt, cos, sin, *C.OUT_U8, mid_dtype=mid)
    C.same(y.levels, C.hf_composed(x, consts, cos, sin, C.OUT_U8, mid))
    from torchlsq.functional import _act_constants
    assert (y.quant_min, y.quant_max) == (0, 255) and torch.equal(y.zero_point, _act_constants(*C.OUT_U8[:2], 0, 255)[1])
    C.same(lsq_rope_w8(lt, cos, sin, mid), C.hf_composed(x, consts, cos, sin, None, mid))


@pytest.mark.parametrize("mid", [F32, BF16, F16], ids=str)
def test_interleaved_is_half_on_permuted_features(mid):
    D, R = 64, 32
    x, consts = C.levels((2, 5, 3, D), 9, I8), C.constants(I8)
    cos, sin = C.tables(R, 16, mid)
    perm = torch.cat((torch.arange(0, R, 2), torch.arange(1, R, 2), torch.arange(R, D)))      # half position -> interleaved feature
    for q in (C.OUT_U8, None):
        inter = C.run_rope("cpu", x, consts, cos, sin, q, mid, [1, 4], True)
        half = C.run_rope("cpu", x[..., perm].contiguous(), consts, cos, sin, q, mid, [1, 4], False)
        back = torch.empty_like(half)
        back[..., perm] = half
        C.same(inter, back)


def test_a_strided_x_is_read_in_place_and_a_transposed_one_made_dense():
    q_, k_ = C.qkv_views(2, 5, 3, 32, 5)
    consts = C.constants(U8)
    cos, sin = C.tables(32, 16, BF16)
    for v in (q_, k_, k_.transpose(2, 3).contiguous().transpose(2, 3)):
        C.same(C.run_rope("cpu", v, consts, cos, sin, C.OUT_U8, BF16), C.run_rope("cpu", v.contiguous(), consts, cos, sin, C.OUT_U8, BF16))
    empty = C.run_rope("cpu", q_[:0], consts, cos, sin, C.OUT_U8, BF16)
    assert tuple(empty.shape) == (0, 5, 3, 32) and empty.dtype == U8


def test_tables():
    from torchlsq.functional import lsq_rope_tables
    for mid in (F32, BF16, F16):
        cos, sin = lsq_rope_tables(8, 5, 100.0, mid)
        ang = torch.arange(5, dtype=torch.float64).reshape(5, 1) * torch.tensor([100.0 ** (-2 * i / 8) for i in range(4)], dtype=torch.float64)
        assert cos.dtype == sin.dtype == F32 and tuple(cos.shape) == (5, 4) and cos.is_contiguous()
        assert torch.equal(cos, torch.cos(ang).to(F32).to(mid).to(F32)) and torch.equal(sin, torch.sin(ang).to(F32).to(mid).to(F32))


# ---------------------------------------------------------------------------------------------------
# 7: placement
# ---------------------------------------------------------------------------------------------------
PLACES = [(None, False), ([0, 9], False), ([0, 9], True), ([-2, 14], True), ([-2, 14], False), ([-7, 3], True), ([20, -5], True), ([11, 12], True)]


@pytest.mark.parametrize("positions,scatter", PLACES, ids=str)
def test_placement(positions, scatter):
    """P = 16 positions in the tables, Tout = 12: tokens with p < 0, p >= P, and with scatter p >= Tout leave the poisoned out untouched"""
    B, T, H, D, Tmax = 2, 5, 3, 32, 12
    x, consts = C.levels((B, T, H, D), 3), C.constants(U8)
    cos, sin = C.tables(32, 16, BF16)
    for q, mid in ((C.OUT_U8, BF16), (None, F32)):
        ref = C.finish(np.nan_to_num(C.numpy_value(x, consts, cos, sin, mid, positions)), q, mid)
        buf, view = C.cache_view(B, H, Tmax, D, ref.dtype)
        before = buf.clone()
        got = C.run_rope("cpu", x, consts, cos, sin, q, mid, positions, out=view, scatter=scatter)
        assert got.data_ptr() == view.data_ptr()
        want = C.placed(before[64:-64].view(B, H, Tmax, D).permute(0, 2, 1, 3), ref, positions, 16, scatter)
        C.same(view, want, (positions, scatter))
        C.same(buf[:64], before[:64])
        C.same(buf[-64:], before[-64:])
    # COPY against plain index assignment: P is replaced by Tout
    buf, view = C.cache_view(B, H, Tmax, D, U8)
    before = buf.clone()
    OPS.lsq_kv_copy_w8(x, view, C.pos_tensor(positions), scatter)
    want = before[64:-64].view(B, H, Tmax, D).permute(0, 2, 1, 3).clone()
    for b in range(B):
        for t in range(T):
            p = t + (positions[b] if positions else 0)
            if 0 <= p < Tmax:
                want[b, p if scatter else t] = x[b, t]
    C.same(view, want, (positions, scatter))
    C.same(buf[:64], before[:64])
    C.same(buf[-64:], before[-64:])
    written = sum(1 for b in range(B) for t in range(T) if 0 <= t + (positions[b] if positions else 0) < Tmax)
    assert int((view != before[64:-64].view(B, H, Tmax, D).permute(0, 2, 1, 3)).any(-1).any(-1).sum()) == written


def test_kv_append_returns_the_cache_with_xs_constants():
    from torchlsq.functional import LevelsTensor, lsq_kv_append_w8
    x, consts = C.levels((2, 1, 3, 6), 8, I8), C.constants(I8)
    cache = torch.zeros((2, 3, 9, 6), dtype=I8)
    r = lsq_kv_append_w8(LevelsTensor(x, *consts, -128, 127), cache.permute(0, 2, 1, 3), C.pos_tensor([4, 8]))
    assert r.levels.data_ptr() == cache.data_ptr() and r.scale is not None and int(r.zero_point) == -3 and (r.quant_min, r.quant_max) == (-128, 127)
    assert torch.equal(cache[0, :, 4], x[0, 0]) and torch.equal(cache[1, :, 8], x[1, 0]) and int((cache != 0).any(-1).any(1).sum()) == 2


# ---------------------------------------------------------------------------------------------------
# 8: the bound against float64
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", [F32, BF16, F16], ids=str)
@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
def test_bound_against_float64(mid, interleaved):
    """x, the table entry, the product and the sum are each rounded once in fp32 and once to mid: eight factors (1 + e), so
    |u - u*| <= ((1 + u)^4 (1 + 2^-24)^4 - 1) (|x_i c| + |x_j s|), and ((1 + u)(1 + 2^-24) - 1) |x| beyond R.  Nothing underflows
    here: |x| >= 0.025 or x = 0, and a term below float16's normal range 2^-14 is excluded from the ratio (its absolute error is at
    most 2^-25 per rounding instead).  Worst measured ratios to the bound: float32 0.36, bfloat16 0.72, float16 0.68."""
    D, R, P = 64, 32, 64
    u = C.UNIT[mid]
    K = (1 + u) ** 4 * (1 + 2.0 ** -24) ** 4 - 1
    K1 = (1 + u) * (1 + 2.0 ** -24) - 1
    worst = 0.0
    for dtype in (U8, I8):
        x, consts = C.levels((2, 40, 3, D), 60, dtype), C.constants(dtype)
        cos, sin = C.tables(R, P, mid)
        pos = [0, 24]
        got = C.run_rope("cpu", x, consts, cos, sin, None, mid, pos, interleaved).double()
        xr = (x.double() - float(consts[1])) * float(consts[0].double())
        p = torch.arange(40).reshape(1, 40) + torch.tensor(pos).reshape(2, 1)
        ang = p.double().unsqueeze(-1) * torch.pow(torch.tensor(10000.0, dtype=torch.float64), -torch.arange(0, R, 2, dtype=torch.float64) / R)
        c, s = torch.cos(ang).unsqueeze(2), torch.sin(ang).unsqueeze(2)
        xi, xj = (xr[..., 0:R:2], xr[..., 1:R:2]) if interleaved else (xr[..., :R // 2], xr[..., R // 2:R])
        gi, gj = (got[..., 0:R:2], got[..., 1:R:2]) if interleaved else (got[..., :R // 2], got[..., R // 2:R])
        for g, exact, mag in ((gi, xi * c - xj * s, (xi * c).abs() + (xj * s).abs()), (gj, xj * c + xi * s, (xj * c).abs() + (xi * s).abs())):
            err = (g - exact).abs()
            assert bool((err <= K * mag).all()), (mid, float((err / mag.clamp_min(1e-300)).max()), K)
            normal = torch.minimum((xi * c).abs(), (xj * s).abs()) >= 2.0 ** -14
            worst = max(worst, float((err[normal] / (K * mag[normal])).max()))
        rest = (got[..., R:] - xr[..., R:]).abs()
        assert bool((rest <= K1 * xr[..., R:].abs()).all())
    print("worst ratio to the bound, %s %s: %.3f" % (mid, "interleaved" if interleaved else "half", worst))
    assert 0.05 < worst <= 1.0


# ---------------------------------------------------------------------------------------------------
# 9: decode equals prefill
# ---------------------------------------------------------------------------------------------------
def test_decode_equals_prefill():
    from torchlsq.quantized import KVCacheW8
    case = C.decode_case()
    B, H, T, D = case["B"], case["H"], case["T"], case["D"]
    assert tuple(case["prefill"].shape) == (B, T, H * D) and len(case["prefill"].unique()) > 32
    cache = KVCacheW8(B, H, case["Tmax"], D)
    for t in range(T):
        ctx = C.decode_step(case, case["rot"], case["core"], cache, t)
        assert tuple(ctx.shape) == (B, 1, H * D) and cache.lengths.tolist() == [t + 1] * B
        assert torch.equal(ctx[:, 0], case["prefill"][:, t]), "decode step %d is not the prefill's row" % t
    assert not bool(cache.k[:, :, T:].any()) and not bool(cache.v[:, :, T:].any())
    assert torch.equal(cache.v[:, :, :T].permute(0, 2, 1, 3), case["qkv"][:, :, 2])


# ---------------------------------------------------------------------------------------------------
# 10, 11: fake kernels, autograd refusal, the modules
# ---------------------------------------------------------------------------------------------------
def test_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    x, consts = C.levels((2, 5, 3, 32), 0), C.constants(U8)
    cos, sin = C.tables(32, 16, BF16)
    with FakeTensorMode() as mode:
        f = [mode.from_tensor(t) for t in (x,) + consts + (cos, sin)]
        a = OPS.lsq_rope_w8_q8_q(*f, *[mode.from_tensor(t) for t in C.OUT_I8[:2]], *C.OUT_I8[2:], BF16, None, True)
        b = OPS.lsq_rope_w8_q8(*f, BF16)
        c = OPS.lsq_kv_copy_w8(f[0], mode.from_tensor(torch.zeros((2, 9, 3, 32), dtype=U8)), None, True)
    assert (a.dtype, tuple(a.shape)) == (I8, (2, 5, 3, 32)) and (b.dtype, tuple(b.shape)) == (BF16, (2, 5, 3, 32)) and c is None
    torch.library.opcheck(OPS.lsq_rope_w8_q8.default, (x,) + consts + (cos, sin, BF16), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(OPS.lsq_kv_copy_w8.default, (x, torch.zeros((2, 9, 3, 32), dtype=U8), C.pos_tensor([1, 3]), True),
                          test_utils=("test_schema", "test_faketensor"))


def test_modules_state_dict_and_reset():
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import KVCacheW8, RotaryW8Q
    rot = RotaryW8Q(C.trained(-4.0, 4.0), 64, 16, base=500.0, rotary_dim=32, interleaved=True, mid_dtype=F16)
    assert sorted(rot.state_dict()) == ["output_scale", "output_shift"] and tuple(rot.cos.shape) == (16, 16)
    assert sorted(n for n, _ in rot.named_buffers()) == ["cos", "output_scale", "output_shift", "sin"]
    want = C.tables(32, 16, F16, 500.0)
    assert torch.equal(rot.cos, want[0]) and torch.equal(rot.sin, want[1])
    other = RotaryW8Q(C.trained(-1.0, 1.0), 64, 16, base=500.0, rotary_dim=32, interleaved=True, mid_dtype=F16)
    other.load_state_dict(rot.state_dict())
    x = LevelsTensor(C.levels((2, 5, 3, 64), 4), *C.constants(U8), 0, 255)
    y = rot(x, positions=C.pos_tensor([0, 6]))
    C.same(other(x, positions=C.pos_tensor([0, 6])).levels, y.levels)
    C.same(y.levels, C.run_rope("cpu", x.levels, C.constants(U8), *want, (rot.output_scale, rot.output_shift) + rot.output_range, F16, [0, 6], True))
    fl = RotaryW8Q(None, 64, 16, mid_dtype=BF16)
    assert fl(x).dtype == BF16 and "floats out" in repr(fl) and "interleaved" in repr(rot)
    with pytest.raises(AssertionError, match="rotary_dim must be even"):
        RotaryW8Q(None, 64, 16, rotary_dim=66)
    with pytest.raises(AssertionError, match=r"needs levels of \[B, T, H, 64\]"):
        rot(LevelsTensor(C.levels((2, 5, 3, 32), 4), *C.constants(U8), 0, 255))

    cache = KVCacheW8(2, 3, 8, 64, k_dtype=U8, v_dtype=I8)
    assert sorted(cache.state_dict()) == ["k", "lengths", "v"] and cache.lengths.dtype == torch.int32 and cache.v.dtype == I8
    v = LevelsTensor(C.levels((2, 5, 3, 64), 6, I8), *C.constants(I8), -128, 127)
    kl, vl, lens = cache.append(x, v, rotary=rot)
    assert lens is cache.lengths and lens.tolist() == [5, 5] and kl.levels is cache.k and vl.levels is cache.v
    C.same(cache.k[:, :, :5].permute(0, 2, 1, 3), rot(x).levels)
    C.same(cache.v[:, :, :5].permute(0, 2, 1, 3), v.levels)
    assert int(vl.zero_point) == -3 and torch.equal(kl.zero_point, rot(x).zero_point) and kl.quant_max == rot.output_range[1]
    kl, vl, lens = cache.append(x, v, rotary=rot)             # 5 more: the last two fall outside max_len = 8 and are skipped
    assert lens.tolist() == [10, 10]
    C.same(cache.k[:, :, 5:].permute(0, 2, 1, 3), rot(x, positions=C.pos_tensor([5, 5])).levels[:, :3])
    with pytest.raises(AssertionError, match="level range"):
        cache.append(x, LevelsTensor(v.levels, *C.constants(I8), -127, 127))
    with pytest.raises(AssertionError, match=r"k must be \[2, T, 3, 64\]"):
        cache.append(LevelsTensor(x.levels[:, :, :2], *C.constants(U8), 0, 255), v)
    cache.reset()
    assert cache.lengths.tolist() == [0, 0]
    plain = KVCacheW8(2, 3, 8, 64)
    plain.append(x, x)
    C.same(plain.k[:, :, :5].permute(0, 2, 1, 3), x.levels)
