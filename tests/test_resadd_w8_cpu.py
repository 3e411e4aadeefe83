"""No GPU: the W8A8 layers that close a residual block (include/lsq_hip_resadd_w8.h, liblsq_hip_resadd_w8.so,
torch.ops.torchlsq.lsq_linear_w8_q8_add_q / lsq_conv2d_w8_q8_add_q, torchlsq.quantized.LinearW8A8AddQ / Conv2dW8A8AddQ / AddW8A8Q /
convert_w8a8_add_q).

  * the header's declarations == the library's exports == the _abi.py table, the two structs field by field;
  * the kernel set read from the built library: twelve tiles kernels and two generic ones, nothing else; no scratch, no atomics;
    tiles kernels: v_mfma_i32_16x16x64_i8 only, at most 128 VGPRs, packet loads and stores and the byte store;
  * the plan field by field and every refusal without a GPU;
  * the CPU ops against the existing ops composed (the definition), rounding at ties against integers, the NaN rule, and one
    float32 case in which a fused multiply-add of the residual's product and the add would change levels;
  * the modules' state dicts, convert_w8a8_add_q on a BasicBlock against the existing modules written out.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import qconv_w8_cases as V
import qlinear_w8_cases as W
import requant_w8_cases as R
import resadd_w8_cases as A
from helpers import LLVM, demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_resadd_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_resadd_w8.so")
NAMES = sorted(["lsq_resadd_w8_abi_version", "lsq_resadd_w8_last_error", "lsq_resadd_w8_linear_levels", "lsq_resadd_w8_conv_levels",
                "lsq_resadd_w8_plan_linear", "lsq_resadd_w8_plan_conv"])
LSQ_EINVAL = -1
CL = torch.channels_last
OPS = torch.ops.torchlsq


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    return [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(const void\*|int64_t)", "", decl.strip()).split(",") if f.strip()]


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_\w+)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_RESADD_W8) == NAMES and len(NAMES) == 6
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_", "lsq_requant_", "lsq_resadd_"):
        assert other not in und, other
    assert E.resadd_w8_library().lsq_resadd_w8_abi_version() == E.RESADD_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_RESADD_W8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    assert _fields(text, "lsq_resadd_w8_res") == [f[0] for f in E.LsqResaddW8Res._fields_] and ctypes.sizeof(E.LsqResaddW8Res) == 4 * 8
    assert _fields(text, "lsq_resadd_w8_pre") == [f[0] for f in E.LsqResaddW8Pre._fields_] and ctypes.sizeof(E.LsqResaddW8Pre) == 6 * 8


def test_kernels(tmp_path):
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    tiles, single = set(), set()
    for sym, dm in names.items():
        m = re.match(r"^void lsq::resadd_w8_(linear|conv)_tiles_kernel<(?:\(int\))?([248]), (?:\(bool\))?(true|false|0|1)>\(", dm)
        if m:
            tiles.add((m.group(1), int(m.group(2)), m.group(3) in ("true", "1")))
            continue
        m = re.match(r"^lsq::resadd_w8_(linear_generic|conv_generic)_kernel\(", dm)
        assert m, "not a kernel of this library: %s" % dm
        single.add(m.group(1))
    assert tiles == {(src, s, k) for src in ("linear", "conv") for s in (2, 4, 8) for k in (False, True)}
    assert single == {"linear_generic", "conv_generic"} and len(every) == 14
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
            assert "global_store_dwordx4" in ops and "global_store_byte" in ops, sym
            assert "global_load_ubyte" in ops, sym                                       # the byte fill of the residual tile
            assert 0 < vgprs[sym] <= 128, (sym, vgprs[sym])
        else:
            assert not mfma, sym


def test_plan_without_a_gpu():
    from torchlsq import extension as E
    lib = E.resadd_w8_library()
    out = (ctypes.c_int32 * 10)()
    g = E.LsqQconvW8Geom(2, 16, 5, 7, 17, 3, 3, 1, 1, 1, 1, 1, 1)
    err = lib.lsq_resadd_w8_last_error
    assert lib.lsq_resadd_w8_plan_conv(ctypes.byref(g), 1, 1, 1, None) == LSQ_EINVAL and b"NULL" in err()
    assert lib.lsq_resadd_w8_plan_conv(None, 1, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"NULL geometry" in err()
    assert lib.lsq_resadd_w8_plan_linear(3, 16, 16, 1, 1, 1, None) == LSQ_EINVAL and b"NULL" in err()
    assert lib.lsq_resadd_w8_plan_linear(0, 16, 16, 1, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"at least 1" in err()
    nine = ("form", "shape", "grid", "block", "rows_per_tile", "cols_per_tile", "lds_bytes", "k_split", "store")
    # res_load: packets if and only if form 1, N % 16 == 0 and the residual aligned -- whatever y's store is; the other nine
    # fields are lsq_hip_requant_w8.h's plan
    for N in (5, 16, 17, 64, 80, 1000, 1008, 16321):
        for y_aligned in (True, False):
            for res_aligned in (True, False):
                for aligned in (True, False):
                    for M in (1, 16, 17, 32, 33, 40, 64, 65, 2048):
                        pl = E.resadd_w8_plan_linear(M, N, 144, aligned, y_aligned, res_aligned)
                        assert pl["res_load"] == ("packets" if aligned and N % 16 == 0 and res_aligned else "bytes"), (M, N, pl)
                        ref = E.requant_w8_plan_linear(M, N, 144, aligned, y_aligned)
                        assert all(pl[f] == ref[f] for f in nine), (M, N, pl, ref)
                        pc = E.resadd_w8_plan_conv(1, 16, 1, M, N, 3, 1, 1, 1, aligned, y_aligned, res_aligned)
                        rc = E.requant_w8_plan_conv(1, 16, 1, M, N, 3, 1, 1, 1, aligned, y_aligned)
                        assert pc["res_load"] == pl["res_load"] and all(pc[f] == rc[f] for f in nine + ("M", "N", "K")), (M, N, pc, rc)
    assert E.resadd_w8_plan_linear(40, 16, 40)["res_load"] == "bytes" and E.resadd_w8_plan_conv(1, 3, 8, 8, 16, 3)["res_load"] == "bytes"
    for Cin, k, aligned in ((16, 3, True), (32, 1, True), (65536, 1, True), (3, 7, True), (24, 3, True), (65552, 1, True), (16, 3, False)):
        for B in (1, 40):
            a, b = E.resadd_w8_plan_conv(B, Cin, 8, 8, 64, k, 1, 0, 1, aligned), E.requant_w8_plan_conv(B, Cin, 8, 8, 64, k, 1, 0, 1, aligned)
            assert all(a[f] == b[f] for f in nine + ("M", "N", "K")), (Cin, k, aligned, a, b)
    for K, aligned, form in ((16, True, "mfma"), (65536, True, "mfma"), (40, True, "generic"), (65552, True, "generic"), (0, True, "generic"),
                             (16, False, "generic")):
        for M in (1, 40):
            c, d = E.resadd_w8_plan_linear(M, 64, K, aligned), E.requant_w8_plan_linear(M, 64, K, aligned)
            assert c["form"] == d["form"] == form and all(c[f] == d[f] for f in nine), (K, c, d)
    assert W.plan_row_thresholds(lambda M, N, K: E.resadd_w8_plan_linear(M, N, K), 17, 144) == [33, 65]


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.resadd_w8_library()
    ok = 1 << 20
    far = 1 << 24                       # the residual: far from y
    base = dict(B=2, Cin=16, H=5, W=7, Cout=8, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)
    U8, I8 = 0, 1

    def oq(scale=ok, shift=ok, r=(0, 255, 0, 255), relu=0, mid=E.LSQ_BF16, null=False):
        return None if null else ctypes.byref(E.LsqRequantW8Out(scale, shift, r[0], r[1], r[2], r[3], relu, mid))

    def rq(rl=far, rd=U8, rs=ok, rz=ok, rnull=False):
        return None if rnull else ctypes.byref(E.LsqResaddW8Res(rl, rd, rs, rz))

    def pq(pre=False, ps=ok, pb=ok, pr=(0, 255, 0, 255)):
        return ctypes.byref(E.LsqResaddW8Pre(ps, pb, *pr)) if pre else None

    def split(o):
        r = {k: o.pop(k) for k in ("rl", "rd", "rs", "rz", "rnull") if k in o}
        p = {k: o.pop(k) for k in ("pre", "ps", "pb", "pr") if k in o}
        return o, r, p

    def geom(kw):
        return ctypes.byref(E.LsqQconvW8Geom(**dict(base, **kw)))

    def ll(ld=U8, x=ok, M=3, s=ok, z=ok, wd=I8, w=ok, N=8, K=32, ws=ok, wz=ok, bias=None, bd=E.LSQ_F32, y=ok, **o):
        o, r, p = split(o)
        return lib.lsq_resadd_w8_linear_levels(ld, x, M, s, z, wd, w, N, K, ws, wz, bias, bd, oq(**o), rq(**r), pq(**p), y, None)

    def cl(ld=U8, x=ok, s=ok, z=ok, wd=I8, w=ok, ws=ok, wz=ok, bias=None, bd=E.LSQ_F32, y=ok, g=None, **o):
        o, r, p = split(o)
        return lib.lsq_resadd_w8_conv_levels(ld, x, s, z, geom(g or {}), wd, w, ws, wz, bias, bd, oq(**o), rq(**r), pq(**p), y, None)

    err = lib.lsq_resadd_w8_last_error
    for f, mn in ((ll, 3 * 8), (cl, 2 * 5 * 7 * 8)):
        # the new refusals
        assert f(rnull=True) == LSQ_EINVAL and b"NULL residual" in err()
        assert f(rl=None) == LSQ_EINVAL and b"NULL residual levels" in err()
        assert f(rs=None) == LSQ_EINVAL and b"NULL residual" in err()
        assert f(rz=None) == LSQ_EINVAL and b"NULL residual" in err()
        assert f(rs=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(rz=ok + 1) == LSQ_EINVAL and b"element-aligned" in err()
        for rd in (2, -1):
            assert f(rd=rd) == LSQ_EINVAL and b"residual's level_dtype" in err(), rd
        assert f(pre=True, ps=None) == LSQ_EINVAL and b"pre-quantizer" in err()
        assert f(pre=True, pb=None) == LSQ_EINVAL and b"pre-quantizer" in err()
        assert f(pre=True, ps=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
        for r in ((-1, 255, 0, 255), (0, 256, 0, 256), (-128, 127, 0, 255), (5, 4, 0, 255), (-129, 127, -129, 127), (0, 255, 9, 8)):
            assert f(pre=True, pr=r) == LSQ_EINVAL and b"pre-quantizer's" in err() and b"0..255 or within -128..127" in err(), r
        # an in-place add, and every other overlap of the two byte ranges
        for rl in (ok, ok + 1, ok + mn - 1, ok - mn + 1):
            assert f(rl=rl) == LSQ_EINVAL and b"overlap" in err() and b"in-place" in err(), rl
        # what lsq_hip_requant_w8.h refuses
        assert f(null=True) == LSQ_EINVAL and b"NULL output quantizer" in err()
        assert f(scale=None) == LSQ_EINVAL and b"NULL out_scale or out_shift" in err()
        assert f(shift=None) == LSQ_EINVAL and b"NULL out_scale or out_shift" in err()
        assert f(scale=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
        for r in ((-1, 255, 0, 255), (0, 256, 0, 256), (-128, 127, 0, 255), (5, 4, 0, 255), (-129, 127, -129, 127), (0, 255, 9, 8)):
            assert f(r=r) == LSQ_EINVAL and b"output's" in err() and b"0..255 or within -128..127" in err(), r
        for mid in (E.LSQ_F64, 9, -1):
            assert f(mid=mid) == LSQ_EINVAL and b"mid_dtype" in err(), mid
        assert f(wd=2) == LSQ_EINVAL and b"w_level_dtype" in err()
        assert f(ld=2) == LSQ_EINVAL and b"level_dtype" in err()
        for null in ("x", "w", "ws", "wz", "y", "s", "z"):
            assert f(**{null: None}) == LSQ_EINVAL and b"NULL" in err(), null
        assert f(wz=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(ws=ok + 1) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(s=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(z=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(bias=ok, bd=E.LSQ_F16) == LSQ_EINVAL and b"bias" in err()      # neither float32 nor mid_dtype (bfloat16)
        assert f(bias=ok + 2, bd=E.LSQ_F32) == LSQ_EINVAL and b"element-aligned" in err()
    assert ll(M=0) == LSQ_EINVAL and b"at least 1" in err()
    assert ll(N=-1) == LSQ_EINVAL and b"negative" in err()
    assert ll(K=-1) == LSQ_EINVAL and b"negative" in err()
    assert ll(M=1 << 62) == LSQ_EINVAL and b"64-bit offsets" in err()
    assert ll(N=0) == 0 and ll(N=0, pre=True) == 0                             # nothing to do, nothing launched
    for name in ("B", "Cin", "H", "W"):
        assert cl(g={name: 0}) == LSQ_EINVAL and b"at least 1" in err(), name
    assert cl(g=dict(Cout=-1)) == LSQ_EINVAL and b"negative Cout" in err()
    assert cl(g=dict(kh=0)) == LSQ_EINVAL and b"kernel" in err()
    assert cl(g=dict(sh=0)) == LSQ_EINVAL and b"stride" in err()
    assert cl(g=dict(dw=0)) == LSQ_EINVAL and b"dilation" in err()
    assert cl(g=dict(ph=-1)) == LSQ_EINVAL and b"negative padding" in err()
    assert cl(g=dict(kh=8)) == LSQ_EINVAL and b"empty output" in err()
    assert cl(g=dict(H=1 << 31)) == LSQ_EINVAL and b"31 bits" in err()
    assert cl(g=dict(B=1 << 62)) == LSQ_EINVAL and b"64-bit offsets" in err()
    assert cl(g=dict(B=1 << 20, H=1 << 10, W=1 << 10, Cout=1 << 20, kh=1, kw=1, ph=0, pw=0), rl=1 << 62) == LSQ_EINVAL and b"31-bit grid" in err()
    assert cl(g=dict(Cout=0)) == 0


def test_host_checks_of_the_ops():
    case = list(A.linear_case(3, 7, 32, V.VARIANTS[0], R.OUT_VARIANTS[0], A.RES_VARIANTS[2], 0))
    assert A.linear_add(*case).dtype == torch.uint8

    def bad(**kw):
        c = list(case)
        names = ("lx", "s", "z", "lw", "s_w", "zw", "bias", "osc", "osh", "rng", "relu", "mid", "rl", "rs", "rz", "psc", "psh", "prng")
        for k, v in kw.items():
            c[names.index(k)] = v
        return A.linear_add(*c)

    with pytest.raises(RuntimeError, match="residual levels must be uint8"):
        bad(rl=case[12].float())
    with pytest.raises(RuntimeError, match="residual levels have shape"):
        bad(rl=case[12][:, :6])
    with pytest.raises(RuntimeError, match="res_scale must be one float32"):
        bad(rz=case[14].float())
    with pytest.raises(RuntimeError, match="come together"):
        bad(psh=None)
    with pytest.raises(RuntimeError, match="pre-quantizer"):
        bad(prng=(0, 256, 0, 256))
    with pytest.raises(RuntimeError, match="pre_scale and pre_shift must be float32"):
        bad(psc=torch.tensor([0.1, 0.2]))
    with pytest.raises(RuntimeError, match="mid_dtype"):
        bad(mid=torch.float64)
    with pytest.raises(RuntimeError, match="inference-only"):
        bad(rs=case[13].clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="inference-only"):
        bad(psc=case[15].clone().requires_grad_(True))
    assert bad(rng=(-128, 127, -128, 127), osh=torch.tensor([0.0])).dtype == torch.int8


@pytest.mark.parametrize("res_variant", A.RES_VARIANTS, ids=A.res_id)
@pytest.mark.parametrize("out_variant", R.OUT_VARIANTS, ids=R.out_id)
def test_cpu_ops_equal_the_existing_ops_composed(out_variant, res_variant):
    """the definition, for every output level type, relu on and off, every mid_dtype, pre on and off and both residual level
    types: linear (M N = 40 * 37) and conv2d (every geometry of qconv_w8_cases; the conditions where M N >= 336)"""
    unsigned = out_variant[0]
    for i, variant in enumerate(V.VARIANTS):
        case = A.linear_case(40, 37, 80, variant, out_variant, res_variant, i)
        got = A.linear_add(*case)
        assert got.dtype == (torch.uint8 if unsigned else torch.int8) and got.shape == (40, 37)
        assert torch.equal(got, A.linear_composed(*case))
        A.assert_conditions(got, case, False, ("linear", i))
    for i, geometry in enumerate(V.GEOMETRIES):
        case = A.conv_case(geometry, V.VARIANTS[i % len(V.VARIANTS)], out_variant, res_variant, i)
        got = A.conv_add(*case)
        assert got.is_contiguous(memory_format=CL) and torch.equal(got, A.conv_composed(*case))
        if got.numel() >= 336:
            A.assert_conditions(got, case, True, V.geom_id(geometry))
        # a residual in NCHW memory is the same residual
        nchw = list(case)
        nchw[13] = case[13].contiguous()
        assert torch.equal(A.conv_add(*nchw), got)


@pytest.mark.parametrize("relu", [False, True])
def test_rounding_at_ties_is_half_to_even_and_a_nan_goes_to_quant_min(relu):
    """power-of-two scales: v = I * 2^-10 and d = (l_r - z_r) * 2^-10 exactly (in every mid_dtype: |I| <= 144, |l_r - z_r| <= 40),
    pre on the same grid (scale 2^-10: the identity inside its range), out_scale 2^-9, so t / s_o = (I + l_r - z_r) / 2 lands on
    .5 for every odd sum; the expected level comes from the integers.  A NaN w_scale row gives quant_min."""
    g = torch.Generator().manual_seed(11)
    lx = torch.randint(-3, 4, (24, 16), generator=g).to(torch.int8)
    lw = torch.randint(-3, 4, (19, 16), generator=g).to(torch.int8)
    s, z = W.act(2.0 ** -4, 0)
    s_w, zw = torch.full((19,), 2.0 ** -6), torch.zeros(19, dtype=torch.int32)
    I = lx.to(torch.int64) @ lw.to(torch.int64).t()
    assert bool((I % 2 == 1).any()) and int(I.abs().max()) <= 144
    for res_dt, z_r in ((torch.uint8, 100), (torch.int8, -7)):
        k = torch.randint(-40, 41, (24, 19), generator=g)
        rl, rs, rz = (k + z_r).to(torch.int32).to(res_dt), torch.tensor([2.0 ** -10]), torch.tensor([z_r], dtype=torch.int32)
        for pre in (A.NO_PRE, (torch.tensor([2.0 ** -10]), torch.tensor([-128 * 2.0 ** -10]), (0, 255, 0, 255))):
            for (lo, hi), zp in (((0, 255), 128), ((-128, 127), 0), ((0, 255), 3), ((-128, 127), -125)):
                osc, osh = torch.tensor([2.0 ** -9]), torch.tensor([-zp * 2.0 ** -9])
                T = (I.clamp(-128, 127) if pre[0] is not None else I) + k
                Tr = T.clamp_min(0) if relu else T
                want = torch.round(Tr.double() / 2 + zp).clamp(lo, hi).to(torch.int64)         # torch.round: half to even
                ties = (Tr % 2 == 1) & (want > lo) & (want < hi)
                assert bool(ties.any()) and bool(((I + k) != I).any())
                for mid in R.MIDS:
                    got = A.linear_add(lx, s, z, lw, s_w, zw, None, osc, osh, (lo, hi, lo, hi), relu, mid, rl, rs, rz, *pre)
                    assert torch.equal(got.to(torch.int64), want), (res_dt, lo, hi, zp, mid)
                    if pre[0] is None:              # (with pre a NaN becomes pre's quant_min, a number)
                        bad = s_w.clone()
                        bad[5] = float("nan")
                        got = A.linear_add(lx, s, z, lw, bad, zw, None, osc, osh, (lo + 1, hi, lo, hi), relu, mid, rl, rs, rz, *pre)
                        got = got.to(torch.int64)
                        assert bool((got[:, 5] == lo + 1).all()) and torch.equal(got[:, :5], want[:, :5].clamp_min(lo + 1)), (lo, hi, zp, mid)


def test_the_definition_is_the_unfused_one():
    """float32, s_w s_x = 1 so that p = I exactly, s_r = 1 + 2^-23, I = -(l_r - z_r): p + d cancels to the rounding error of
    the product d.  Rounded once (an fma of the product and the add) t = (l_r - z_r) 2^-23 exactly; rounded twice, as the
    definition has it, t is a multiple of ulp(d).  With the output scale 2^-23 the two differ by whole levels."""
    case, k, two_step, fused = A.contraction_case()
    assert bool((two_step != fused).any()) and float((two_step != fused).double().mean()) > 0.25
    got = A.linear_add(*case)
    assert torch.equal(got.to(torch.int64), two_step)
    assert torch.equal(got, A.linear_composed(*case))


def test_state_dict_round_trips():
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import Conv2dW8A8AddQ, LinearW8A8AddQ
    from torchlsq.quantized.modules.w8a8_add_q import PendingAdd
    block, qs, x = A.basic_block()
    xl = LevelsTensor.from_quantized(qs["mid"].quantize(torch.relu(torch.randn(2, 32, 5, 5))))
    res = LevelsTensor(W.levels((2, 5, 5, 32), 0, 255, 3).permute(0, 3, 1, 2), torch.tensor([0.02]), torch.tensor([120], dtype=torch.int32), 0, 255)
    for pre in (None, block.conv2.activation_post_process):
        m = Conv2dW8A8AddQ.from_float(block.conv2, qs["mid"], block.add_relu.activation_post_process, pre_quantizer=pre, relu=True,
                                      mid_dtype=torch.bfloat16)
        assert (m.pre_range is None) == (pre is None) and {"pre_scale", "pre_shift", "output_scale"} <= set(dict(m.named_buffers()))
        fresh = Conv2dW8A8AddQ(32, 32, 3, padding=1)
        fresh.load_state_dict(m.state_dict())
        assert fresh.pre_range == m.pre_range and fresh.relu and fresh.mid_dtype == torch.bfloat16 and fresh.output_range == m.output_range
        want = m(xl, res)
        assert isinstance(want, LevelsTensor) and torch.equal(fresh(xl, res).levels, want.levels) and len(want.levels.unique()) > 16
        pending = fresh(xl)
        assert isinstance(pending, PendingAdd) and torch.equal(pending.add(res).levels, want.levels)
        assert torch.equal(pending.add(res, relu=False).levels, m._launch(xl, res, False).levels)
    with_pre, without = m(xl, res).levels, Conv2dW8A8AddQ.from_float(block.conv2, qs["mid"], block.add_relu.activation_post_process,
                                                                     pre_quantizer=None, relu=True, mid_dtype=torch.bfloat16)(xl, res).levels
    assert not torch.equal(with_pre, without)
    # the default pre-quantizer is the layer's own activation_post_process
    assert Conv2dW8A8AddQ.from_float(block.conv2, qs["mid"], block.add_relu.activation_post_process).pre_range is not None
    assert Conv2dW8A8AddQ.from_float(block.conv1, qs["in"], qs["mid"]).pre_range is None       # (an nn.Identity: none)
    model, q_in, q_mid = W.qat_model()
    q_out = R.trained_quantizer(torch.randn(8, 8))
    lin = LinearW8A8AddQ.from_float(model[2], q_mid, q_out, pre_quantizer=R.trained_quantizer(torch.randn(8, 8) * 2), mid_dtype=torch.float16)
    fresh = LinearW8A8AddQ(32, 8, bias=lin.bias is not None)
    fresh.load_state_dict(lin.state_dict())
    xl = LevelsTensor.from_quantized(q_mid.quantize(torch.rand(5, 32)))
    res = LevelsTensor(W.levels((5, 8), -128, 127, 4), torch.tensor([0.01]), torch.tensor([3], dtype=torch.int32), -128, 127)
    assert fresh.pre_range == lin.pre_range and fresh.mid_dtype == torch.float16
    assert torch.equal(fresh(xl, res).levels, lin(xl, res).levels) and "residual add" in repr(fresh)


@pytest.mark.parametrize("mid", R.MIDS, ids=lambda v: str(v).replace("torch.", ""))
def test_convert_w8a8_add_q_on_a_basic_block_equals_the_existing_modules_written_out(mid):
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import AddW8A8Q, Conv2dW8A8AddQ, Conv2dW8A8Q, convert_w8a8_add_q
    from torchlsq.quantized.modules.w8a8_add_q import PendingAdd
    block, qs, x = A.basic_block()
    new = A.convert_block(block, qs, mid)
    assert isinstance(new.conv2, Conv2dW8A8AddQ) and isinstance(new.add_relu, AddW8A8Q) and isinstance(new.conv1, Conv2dW8A8Q)
    assert isinstance(new.downsample, Conv2dW8A8Q) and not isinstance(new.conv1, Conv2dW8A8AddQ)
    assert new.conv2.pre_range is not None and new.conv2.mid_dtype == mid
    assert not isinstance(block.conv2, Conv2dW8A8AddQ)                                         # a deep copy: the model is untouched
    xl = LevelsTensor.from_quantized(qs["in"].quantize(x))
    got = new(xl)                                                                             # the block's own forward
    assert isinstance(got, LevelsTensor) and got.levels.shape == (4, 32, 5, 5) and got.levels.is_contiguous(memory_format=CL)
    want = A.block_written_out(block, qs, xl, mid)
    assert torch.equal(got.levels, want) and len(want.unique()) > 32
    assert int(got.levels.min()) == int(got.zero_point)                                       # add_relu: nothing below zero
    # add (no ReLU) and the operands in either order
    h, identity = new.conv1(xl), new.downsample(xl)
    pending = new.conv2(h)
    assert isinstance(pending, PendingAdd)
    assert torch.equal(new.add_relu.add_relu(identity, pending).levels, want)
    lin = new.add_relu.add(pending, identity).levels
    assert torch.equal(lin, new.add_relu.add(identity, pending).levels) and torch.equal(lin, new.conv2._launch(h, identity, False).levels)
    with pytest.raises(TypeError, match="one pending layer output"):
        new.add_relu.add(identity, identity)
    with pytest.raises(TypeError, match="one pending layer output"):
        new.add_relu.add_relu(pending, pending)
    with pytest.raises(RuntimeError, match="not intended"):
        new.add_relu(identity)
    # refusals of the converter
    with pytest.raises(ValueError, match="input_quantizers"):
        convert_w8a8_add_q(block, {"add_relu": "conv2"}, {})
    with pytest.raises(ValueError, match="not a FloatFunctional"):
        convert_w8a8_add_q(block, {"relu": "conv2"}, {"conv2": qs["mid"]})
    with pytest.raises(ValueError, match="not a linear layer or a 2-D convolution"):
        convert_w8a8_add_q(block, {"add_relu": "relu"}, {"relu": qs["mid"]})


def test_a_layer_with_a_batch_norm_is_refused_by_name():
    import torch.ao.nn.intrinsic as nni
    import torch.ao.nn.intrinsic.qat as nniqat
    from torch.ao.quantization import QConfig
    from torch.ao.quantization.observer import MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer, convert_w8a8_add_q
    block, qs, x = A.basic_block()
    weight = LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                        qscheme=torch.per_channel_symmetric)
    f = nni.ConvBn2d(torch.nn.Conv2d(32, 32, 3, padding=1), torch.nn.BatchNorm2d(32))
    for mod in (f, f[0], f[1]):
        mod.qconfig = QConfig(activation=torch.nn.Identity, weight=weight)
    f.train()
    block.conv2 = nniqat.ConvBn2d.from_float(f)
    with pytest.raises(ValueError, match="'conv2' is a ConvBn2d module: its batch norm"):
        convert_w8a8_add_q(block, {"add_relu": "conv2"}, {"conv2": qs["mid"]})
