"""The masked softmax on 8-bit levels (include/lsq_hip_attn_mask_w8.h), everything that needs no GPU: the library's exports against
its header and `_abi.py`, its kernel set and their resources, the plan against the unmasked op's, every refusal, and the CPU path --
the definition the GPU tests compare against -- held BIT FOR BIT to the existing unmasked op applied to every row's prefix, to the
derived bound with C replaced by n_r and to ATen's softmax of the -inf-masked scores within one level, with the modules and the
fake kernels on top.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import attn_mask_w8_cases as M
import attn_w8_cases as A
from helpers import demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_attn_mask_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_attn_mask_w8.so")
NAMES = sorted(["lsq_attn_mask_w8_abi_version", "lsq_attn_mask_w8_last_error", "lsq_softmax_mask_w8", "lsq_softmax_mask_w8_plan"])
LSQ_EINVAL = -1
OPS = torch.ops.torchlsq
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
one = A.one


# ---------------------------------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------------------------------
def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_(?:attn|softmax)_mask_w8\w*)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_ATTN_MASK_W8) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_", "lsq_requant_", "lsq_resadd_",
                  "lsq_pool_", "lsq_dwconv_", "lsq_eltwise_", "lsq_norm_", "lsq_attn_", "lsq_bmm_", "lsq_softmax_"):
        assert other not in und, other
    assert E.attn_mask_w8_library().lsq_attn_mask_w8_abi_version() == E.ATTN_MASK_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_ATTN_MASK_W8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    body = re.search(r"typedef struct lsq_softmax_mask_w8_geom \{(.*?)\} lsq_softmax_mask_w8_geom;", text, re.S).group(1)
    fields = [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*int64_t", "", decl.strip()).split(",") if f.strip()]
    assert fields == [f[0] for f in E.LsqSoftmaxMaskW8Geom._fields_] and ctypes.sizeof(E.LsqSoftmaxMaskW8Geom) == 9 * 8


def test_kernels(tmp_path):
    """the eight packet instantiations and the generic kernel: no scratch, the 1 KB table in LDS, one barrier, packet loads and stores,
    the packed byte max, no exp"""
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    short = {}
    for sym, dm in names.items():
        m = re.match(r"^(?:void )?lsq::(softmax_mask_w8_packets|softmax_mask_w8_generic)_kernel(?:<([^>]*)>)?\(", dm)
        assert m, "not a kernel of this library: %s" % dm
        short[sym] = m.group(1) + "".join("_" + n for n in re.findall(r"\d+", re.sub(r"\((?:int|bool)\)", "", m.group(2) or "")))
    want = ["softmax_mask_w8_generic"] + ["softmax_mask_w8_packets_%d_1" % L for L in (4, 8, 16, 32, 64)] + \
           ["softmax_mask_w8_packets_64_%d" % P for P in (2, 4, 8)]
    assert sorted(short.values()) == sorted(want)
    for sym, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0, "%s uses %d bytes of scratch" % (sym, scratch)
        assert "v_exp_f32_e32" not in ops and not any(o.startswith(("global_atomic", "ds_add", "buffer_atomic")) for o in ops), sym
        if short[sym].startswith("softmax_mask_w8_packets"):
            P = int(short[sym].split("_")[-1])
            assert ops.count("global_load_dwordx4") >= P and "global_store_dwordx4" in ops and ops.count("s_barrier") == 1, sym
            assert "v_pk_max_u16" in ops, sym


# ---------------------------------------------------------------------------------------------------
# 7: the plan is the unmasked op's
# ---------------------------------------------------------------------------------------------------
def test_plan_equals_the_unmasked_plan():
    from torchlsq import extension as E
    for C in (1, 16, 64, 65, 197, 257, 1024, 1025, 2049, 4100, 8192, 8193, 65536):
        ld = (C + 15) // 16 * 16
        for R in (35, 4 * 35 * 512 * 64):
            for ldx, ldy, aligned in ((ld, ld, True), (ld, ld, False), (C, ld, True), (ld, ld + 1, True)):
                want = E.attn_w8_plan_softmax(R, C, ldx, ldy, aligned, I8)
                for kw in (dict(), dict(causal=True, causal_offset=3), dict(rows_per_length=35), dict(causal=True, rows_per_length=R)):
                    assert E.attn_mask_w8_plan_softmax(R, C, 35, ldx, ldy, aligned, I8, **kw) == want, (C, R, ldx, ldy, aligned, kw)
    pl = E.attn_mask_w8_plan_softmax(2 * 12 * 197, 197, 197, 208, 208, causal=True)
    assert pl == dict(family="packets", grid=296, block=256, lanes_per_row=16, packets_per_lane=1, rows_per_workgroup=16, lds_bytes=1024)
    assert E.attn_mask_w8_plan_softmax(32 * 32, 2048, 1, rows_per_length=32)["packets_per_lane"] == 2


# ---------------------------------------------------------------------------------------------------
# 6: refusals
# ---------------------------------------------------------------------------------------------------
def test_library_refusals():
    from torchlsq import extension as E
    lib = E.attn_mask_w8_library()
    G = E.LsqSoftmaxMaskW8Geom
    out = (ctypes.c_int32 * 8)()

    def err():
        return lib.lsq_attn_mask_w8_last_error()

    def plan(g, aligned=1, has=0, o=out):
        return lib.lsq_softmax_mask_w8_plan(ctypes.byref(g) if g is not None else None, aligned, has, ctypes.byref(o) if o is not None else None)
    ok = (8, 16, 16, 16, 0, 4, 8, 1, 0)
    assert plan(G(*ok), has=1) == 0 and list(out)[:7] == [1, 1, 256, 4, 1, 64, 1024]
    # everything lsq_softmax_w8 refuses
    assert plan(None) == LSQ_EINVAL and b"NULL geometry" in err()
    assert plan(G(*ok), o=None) == LSQ_EINVAL and b"NULL output" in err()
    assert plan(G(8, 16, 16, 16, 2, 4, 8, 1, 0)) == LSQ_EINVAL and b"x_dtype must be" in err()
    for bad in ((0, 16), (8, 0), (-1, 16)):
        assert plan(G(*bad, 16, 16, 0, 1, 1, 0, 0)) == LSQ_EINVAL and b"at least 1" in err(), bad
    assert plan(G(4, 65537, 65537, 65537, 0, 4, 4, 0, 0)) == LSQ_EINVAL and b"at most 65536" in err()
    assert plan(G(4, 65536, 65536, 65536, 0, 4, 4, 0, 0)) == 0
    assert plan(G(1 << 29, 16, 16, 16, 0, 1, 1, 0, 0)) == LSQ_EINVAL and b"beyond 29 bits" in err()
    assert plan(G(4 * ((1 << 24) - 1) + 4, 16, 20, 16, 0, 4, 4, 0, 0)) == LSQ_EINVAL and b"workgroups are beyond 2^24 - 1" in err()
    assert plan(G(4, 16, 15, 16, 0, 4, 4, 0, 0)) == LSQ_EINVAL and b"ldx = 15 and ldy = 16 must be at least C = 16" in err()
    assert plan(G(4, 16, 16, 15, 0, 4, 4, 0, 0)) == LSQ_EINVAL and b"must be at least C" in err()
    # Tq
    for Tq in (0, -4, 3):
        assert plan(G(8, 16, 16, 16, 0, Tq, 8, 0, 0)) == LSQ_EINVAL and b"must be at least 1 and divide R = 8" in err(), Tq
    # rows_per_length: read with lengths only
    for rpl in (0, -8, 2, 6, 12, 16):
        assert plan(G(8, 16, 16, 16, 0, 4, rpl, 0, 0), has=1) == LSQ_EINVAL and b"a multiple of Tq = 4 and divide R = 8" in err(), rpl
        assert plan(G(8, 16, 16, 16, 0, 4, rpl, 0, 0), has=0) == 0, rpl
    # causal and its offset
    for c in (2, -1):
        assert plan(G(8, 16, 16, 16, 0, 4, 8, c, 0)) == LSQ_EINVAL and b"causal must be 0 or 1" in err(), c
    for off in (-1, 1 << 31, 1 << 40):
        assert plan(G(8, 16, 16, 16, 0, 4, 8, 1, off)) == LSQ_EINVAL and b"at least 0 and within 31 bits" in err(), off
    assert plan(G(8, 16, 16, 16, 0, 4, 8, 1, (1 << 31) - 1)) == 0

    x, yy, tab = torch.zeros(8 * 16, dtype=U8), torch.zeros(8 * 16 * 4 + 16, dtype=U8), torch.zeros(260, dtype=torch.int32)
    lens = torch.zeros(4, dtype=torch.int32)
    s = torch.ones(4)

    def outq(**kw):
        base = dict(out_scale=s.data_ptr(), out_shift=s.data_ptr() + 4, quant_min=0, quant_max=255, type_min=0, type_max=255, mid_dtype=E.LSQ_F32)
        base.update(kw)
        return E.LsqAttnW8Out(*[base[f[0]] for f in E.LsqAttnW8Out._fields_])

    def call(g=ok, o=None, tp=tab.data_ptr(), lp=lens.data_ptr(), xp=x.data_ptr(), yp=yy.data_ptr(), no=()):
        o = outq() if o is None else o
        return lib.lsq_softmax_mask_w8(None if "g" in no else ctypes.byref(G(*g)), None if "o" in no else ctypes.byref(o), tp, lp, xp, yp, None)
    assert call(no="g") == LSQ_EINVAL and b"NULL geometry" in err()
    assert call(no="o") == LSQ_EINVAL and b"NULL output description" in err()
    assert call(g=(8, 16, 8, 16, 0, 4, 8, 1, 0)) == LSQ_EINVAL and b"must be at least C" in err()
    assert call(o=outq(mid_dtype=7)) == LSQ_EINVAL and b"mid_dtype must be" in err()
    assert call(o=outq(out_shift=None)) == LSQ_EINVAL and b"they come together" in err()
    assert call(o=outq(quant_min=-1)) == LSQ_EINVAL and b"must lie within" in err()
    for ptr in ("tp", "xp", "yp"):
        assert call(**{ptr: None}) == LSQ_EINVAL and b"NULL buffer" in err(), ptr
    assert call(tp=tab.data_ptr() + 2) == LSQ_EINVAL and b"the table must be element-aligned" in err()
    assert call(o=outq(out_scale=None, out_shift=None), yp=yy.data_ptr() + 1) == LSQ_EINVAL and b"a floating y must be element-aligned" in err()
    assert call(yp=x.data_ptr() + 127) == LSQ_EINVAL and b"the softmax in place is not served" in err()
    assert call(yp=tab.data_ptr() + 1000) == LSQ_EINVAL and b"or the table" in err()
    # the lengths: their pointer, what they divide, and y on top of them
    assert call(lp=lens.data_ptr() + 2) == LSQ_EINVAL and b"key_lengths must be 4-byte aligned" in err()
    assert call(g=(8, 16, 16, 16, 0, 4, 6, 1, 0)) == LSQ_EINVAL and b"rows_per_length = 6" in err()
    big = torch.zeros(64, dtype=torch.int32)
    assert call(lp=big.data_ptr() + 4 * 8, yp=big.data_ptr(), g=(8, 16, 16, 16, 0, 4, 8, 1, 0)) == LSQ_EINVAL and b"overlap the 1 entries of key_lengths" in err()
    assert call(g=(8, 16, 16, 16, 0, 3, 8, 1, 0), lp=None) == LSQ_EINVAL and b"Tq = 3" in err()
    assert call(g=(8, 16, 16, 16, 0, 4, 8, 3, 0)) == LSQ_EINVAL and b"causal must be 0 or 1" in err()
    assert call(g=(8, 16, 16, 16, 0, 4, 8, 1, -2)) == LSQ_EINVAL and b"causal_offset = -2" in err()


def test_op_and_functional_refusals():
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, lsq_masked_softmax_w8, lsq_masked_softmax_w8_q
    x, tab = A.score_rows(2 * 3 * 5, 19, 0, U8).view(2, 3, 5, 19), A.table()
    lens = torch.tensor([3, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="levels must be uint8"):
        OPS.lsq_softmax_mask_w8_q8(x.float(), tab, F32, True, 0, None)
    with pytest.raises(RuntimeError, match="at least 2 axes"):
        OPS.lsq_softmax_mask_w8_q8(x[0, 0, 0], tab, F32, True, 0, None)
    with pytest.raises(RuntimeError, match="key_lengths needs levels of at least 3 axes"):
        OPS.lsq_softmax_mask_w8_q8(x[0, 0], tab, F32, False, 0, lens[:1])
    with pytest.raises(RuntimeError, match=r"key_lengths must be a dense int32 tensor of \[2\].*'int64'"):
        OPS.lsq_softmax_mask_w8_q8(x, tab, F32, False, 0, lens.long())
    for bad in (lens[:1], torch.zeros(3, dtype=torch.int32), lens.reshape(2, 1), torch.zeros(4, dtype=torch.int32)[::2]):
        with pytest.raises(RuntimeError, match="key_lengths must be a dense int32 tensor"):
            OPS.lsq_softmax_mask_w8_q8_q(x, tab, *A.PROB_Q, F32, False, 0, bad, 1)
    with pytest.raises(RuntimeError, match="key_lengths must be on the levels' device"):
        E.attn_mask_w8_softmax(x, tab, F32, False, 0, lens.to("meta"))      # (called directly: the dispatcher sends a meta tensor elsewhere)
    with pytest.raises(RuntimeError, match="causal_offset = -1 must be at least 0"):
        OPS.lsq_softmax_mask_w8_q8(x, tab, F32, True, -1, None)
    with pytest.raises(RuntimeError, match=r"lsq_softmax_mask_w8_q8 failed \(-1\).*within 31 bits"):
        OPS.lsq_softmax_mask_w8_q8(x, tab, F32, True, 1 << 31, None)
    with pytest.raises(RuntimeError, match="table must be a dense int32"):
        OPS.lsq_softmax_mask_w8_q8(x, tab.long(), F32, True, 0, None)
    with pytest.raises(RuntimeError, match="out_dtype must be float32"):
        OPS.lsq_softmax_mask_w8_q8(x, tab, torch.float64, True, 0, None)
    with pytest.raises(RuntimeError, match="row_pad = 0"):
        OPS.lsq_softmax_mask_w8_q8_q(x, tab, *A.PROB_Q, F32, True, 0, None, 0)
    with pytest.raises(RuntimeError, match="`out` must be a int8 tensor"):
        E.attn_mask_w8_softmax_q(x, tab, *M.INT8_Q, F32, True, 0, None, 1, out=torch.zeros(x.shape, dtype=U8))
    with pytest.raises(RuntimeError, match="C = 65537"):
        OPS.lsq_softmax_mask_w8_q8(torch.zeros(1, 1, 65537, dtype=U8), tab, F32, True, 0, None)
    # the functions: causal=True needs Tk >= Tq; an offset is an int >= 0
    lt = LevelsTensor(x, one(0.05), one(128, torch.int32), 0, 255)
    tall = LevelsTensor(x.transpose(-1, -2).contiguous(), one(0.05), one(128, torch.int32), 0, 255)
    with pytest.raises(AssertionError, match="needs Tk >= Tq, got Tq = 19 and Tk = 5"):
        lsq_masked_softmax_w8_q(tall, tab, *A.PROB_Q, causal=True)
    with pytest.raises(AssertionError, match="needs Tk >= Tq"):
        lsq_masked_softmax_w8(tall, tab, causal=True)
    for bad in (-1, 1.5, "yes"):
        with pytest.raises(AssertionError, match="causal must be None, a bool or an offset >= 0"):
            lsq_masked_softmax_w8(lt, tab, causal=bad)
    M.same(lsq_masked_softmax_w8(tall, tab, causal=0), M.composed(tall.levels, tab, None, F32, M.prefix_lengths(tall.shape, 0)))
    # inference only
    with pytest.raises(RuntimeError, match="grad|inference"):
        OPS.lsq_softmax_mask_w8_q8_q(x, tab, A.PROB_Q[0].clone().requires_grad_(True), *A.PROB_Q[1:], F32, True, 0, None, 1)


# ---------------------------------------------------------------------------------------------------
# 1 - 4: the CPU path against the existing op on every row's prefix
# ---------------------------------------------------------------------------------------------------
SHAPE = (2, 2, 7, 37)            # Tq = 7 against Tk = 37: offsets 0 and Tk - Tq = 30
MASKS = ((0, None), (30, None), (None, [21, 5]), (0, [21, 5]), (30, [33, 36]), (3, [0, 40]))


def _x(dtype, seed=0, shape=SHAPE):
    R = int(np.prod(shape[:-1]))
    return A.score_rows(R, shape[-1], 300 + seed, dtype).view(shape)


@pytest.mark.parametrize("dtype", [U8, I8], ids=str)
@pytest.mark.parametrize("offset,lengths", MASKS, ids=str)
def test_composition_with_the_existing_op(dtype, offset, lengths):
    """y[r, :n] is the existing lsq_softmax_w8(_q) of x[r, :n]; y[r, n:] is the output side's level of 0, or +0.0"""
    x, tab = _x(dtype), A.table(0.05 if dtype == U8 else 0.02, 1.0)
    n = M.prefix_lengths(SHAPE, offset, lengths)
    assert min(n) < max(n)
    for q, mid in M.SIDES:
        got = M.run_masked("cpu", x, tab, q, mid, offset, lengths)
        M.same(got, M.composed(x, tab, q, mid, n), (q is None, mid))
        if q is not None:
            zero = M.zero_of(q, mid)
            rows = got.reshape(-1, SHAPE[-1])
            assert all(bool((rows[r, v:] == zero).all()) for r, v in enumerate(n))
    # the zero levels are the quantizers' own: not the byte 0 everywhere
    assert int(M.zero_of(M.INT8_Q, F32)) == -128 and int(M.zero_of(M.SHIFTED_Q, F16)) == 20 and int(M.zero_of(A.PROB_Q, BF16)) == 0
    # row by row, as the issue states it (one side: the grouped form above is the same comparison)
    got = M.run_masked("cpu", x, tab, A.PROB_Q, BF16, offset, lengths).reshape(-1, SHAPE[-1])
    rows = x.reshape(-1, SHAPE[-1])
    for r, v in enumerate(n):
        if v:
            assert torch.equal(got[r:r + 1, :v], A.run_softmax("cpu", rows[r:r + 1, :v].contiguous(), tab, A.PROB_Q, BF16)), r


def test_no_mask_is_the_existing_op():
    """with no mask, and with every n_r = C, the result is the existing op's, `row_pad` and `out=` included"""
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, lsq_masked_softmax_w8, lsq_masked_softmax_w8_q, lsq_softmax_w8, lsq_softmax_w8_q
    for dtype in (U8, I8):
        x, tab = _x(dtype, 1), A.table()
        full = (None, None), (36, None), (None, [37, 99]), (40, [37, 37])
        for q, mid in M.SIDES:
            want = A.run_softmax("cpu", x, tab, q, mid)
            for offset, lengths in full:
                M.same(M.run_masked("cpu", x, tab, q, mid, offset, lengths), want, (offset, lengths))
        want = A.run_softmax("cpu", x, tab, A.PROB_Q, BF16, 16)
        got = M.run_masked("cpu", x, tab, A.PROB_Q, BF16, None, None, 16)
        assert got.stride() == want.stride() == (2 * 7 * 48, 7 * 48, 48, 1) and torch.equal(got, want)
        lt = LevelsTensor(x, one(0.05), one(3, torch.int32), *((0, 255) if dtype == U8 else (-128, 127)))
        buf = torch.full((2, 2, 7, 64), 77, dtype=U8)
        y = lsq_masked_softmax_w8_q(lt, tab, *A.PROB_Q, BF16, causal=False, out=buf[..., 5:42])
        assert y.levels.data_ptr() == buf[..., 5:42].data_ptr()
        assert torch.equal(y.levels, lsq_softmax_w8_q(lt, tab, *A.PROB_Q, BF16).levels)
        assert bool((buf[..., :5] == 77).all()) and bool((buf[..., 42:] == 77).all())
        E.attn_mask_w8_softmax_q(x, tab, *A.PROB_Q, BF16, True, 36, None, 1, out=buf[..., 5:42])
        assert torch.equal(buf[..., 5:42], want) and bool((buf[..., 42:] == 77).all())
        M.same(lsq_masked_softmax_w8(lt, tab, F16), lsq_softmax_w8(lt, tab, F16))
        # views that do not collapse to rows are made dense first, as in the existing op
        xt = LevelsTensor(x.transpose(1, 2), lt.scale, lt.zero_point, lt.quant_min, lt.quant_max)
        M.same(lsq_masked_softmax_w8(xt, tab, F32, causal=True), lsq_masked_softmax_w8(
            LevelsTensor(x.transpose(1, 2).contiguous(), lt.scale, lt.zero_point, lt.quant_min, lt.quant_max), tab, F32, causal=True))
        assert lsq_masked_softmax_w8(LevelsTensor(x[:0], lt.scale, lt.zero_point, lt.quant_min, lt.quant_max), tab, causal=True).shape == (0, 2, 7, 37)


@pytest.mark.parametrize("dtype", [U8, I8], ids=str)
def test_bytes_beyond_the_prefix_never_matter(dtype):
    x, tab = _x(dtype, 2), A.table()
    for offset, lengths in MASKS:
        n = M.prefix_lengths(SHAPE, offset, lengths)
        for q, mid in ((A.PROB_Q, BF16), (None, F32)):
            want = M.run_masked("cpu", x, tab, q, mid, offset, lengths)
            for how in ("max", "random"):
                px = M.poisoned(x, n, how)
                assert not torch.equal(px, x)
                M.same(M.run_masked("cpu", px, tab, q, mid, offset, lengths), want, (offset, lengths, how))


def test_edge_lengths():
    """0, negative and beyond C: clamped; an n = 0 row is all level-of-0; no NaN anywhere"""
    x, tab = _x(U8, 3, (6, 1, 3, 37)), A.table()
    lengths = [0, -5, 37, 1000, 1, -(1 << 31)]
    n = M.prefix_lengths(x.shape, None, lengths)
    assert n == [0] * 6 + [37] * 6 + [1] * 3 + [0] * 3
    for mid in A.MIDS:
        fl = M.run_masked("cpu", x, tab, None, mid, None, lengths)
        assert not bool(fl.isnan().any()) and bool((A.bits(fl[0]) == 0).all()) and bool((A.bits(fl[5]) == 0).all())
        assert bool((fl[4, ..., 0] == 1).all()) and bool((A.bits(fl[4, ..., 1:]) == 0).all())
        M.same(fl, M.composed(x, tab, None, mid, n))
    for q, mid in M.SIDES[:3]:
        lv = M.run_masked("cpu", x, tab, q, mid, 0, lengths)
        assert bool((lv[0] == M.zero_of(q, mid)).all()) and bool((lv[1] == M.zero_of(q, mid)).all())
        M.same(lv, M.composed(x, tab, q, mid, M.prefix_lengths(x.shape, 0, lengths)))
    # a table with zeros, and every entry 2^24
    for t in (A.table_with_zeros(), A.full_table()):
        M.same(M.run_masked("cpu", x, t, None, F32, 1, lengths), M.composed(x, t, None, F32, M.prefix_lengths(x.shape, 1, lengths)))


# ---------------------------------------------------------------------------------------------------
# 5: the bound with C replaced by n_r, and ATen's softmax of the -inf-masked scores
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_x,alpha,C", [(0.05, 1.0, 197), (0.1, 0.125, 197), (0.02, 1.0, 1024), (0.3, 1.0, 64)], ids=str)
def test_masked_softmax_against_float64_and_aten(s_x, alpha, C):
    """the derived bound (C -> n_r) against the softmax over the prefix in float64, and at most one level against F.softmax of the
    dequantized scores with -inf beyond the prefix, taken to levels through bfloat16, on rows with n >= 1; the share of levels that
    differ is measured and printed, not capped"""
    from torchlsq.functional import LevelsTensor
    Tq = 32
    tab = A.table(s_x, alpha)
    lengths = [C, C // 2 + 1, 9, 0]
    shape = (4, 1, Tq, C)
    off = C - Tq                                                        # causal=True's: the last query sees every key
    n = np.array(M.prefix_lengths(shape, off, lengths))
    assert n.min() == 0 and n.max() == C and len(set(n.tolist())) > 20
    worst, differ, total = 0.0, 0, 0
    for dtype, z in ((U8, 128), (I8, 0)):
        x = A.score_rows(4 * Tq, C, C, dtype, spread=min(200, 8.0 / (s_x * alpha))).view(shape)
        p = M.run_masked("cpu", x, tab, None, F32, off, lengths).reshape(-1, C).numpy().astype(np.float64)
        b = x.reshape(-1, C).numpy().astype(np.int64)
        valid = np.arange(C)[None, :] < n[:, None]
        live = n >= 1
        m = np.where(valid, b, -1000).max(-1, keepdims=True)
        E = np.where(valid, tab.numpy().astype(np.int64)[np.where(valid, m - b, 0)], 0)
        S = E.sum(-1, keepdims=True).astype(np.float64)
        t = np.float64(np.float32(s_x)) * np.float64(np.float32(alpha))
        e = np.where(valid, np.exp(-t * np.where(valid, m - b, 0).astype(np.float64)), 0.0)
        p_star = e[live] / e[live].sum(-1, keepdims=True)
        err = np.abs(p[live] - p_star)
        bound = A.softmax_bound(p[live], p_star, S[live], n[live][:, None].astype(np.float64))
        assert (err <= bound).all() and (p[~live] == 0).all() and (p[~valid] == 0).all()
        worst = max(worst, float((err * (S[live] / 2.0 ** 24)).max()))
        lt = LevelsTensor(x, one(s_x), one(z, torch.int32), *((0, 255) if dtype == U8 else (-128, 127)))
        scores = (lt.dequantize(F32) * np.float32(alpha)).masked_fill(~torch.from_numpy(valid).view(shape), float("-inf"))
        keep = torch.from_numpy(live).view(shape[:-1])
        ref = torch.softmax(scores[keep], -1).to(BF16)
        assert not bool(ref.isnan().any())
        ref = OPS.lsq_levels_per_tensor(ref, *A.PROB_Q, 0).view(U8).to(torch.int16)
        got = M.run_masked("cpu", x, tab, A.PROB_Q, BF16, off, lengths)[keep].to(torch.int16)
        assert int((got - ref).abs().max()) <= 1
        differ, total = differ + int((got != ref).sum()), total + got.numel()
    print("masked softmax s_x=%g alpha=%g C=%d: worst error * S / 2^24 = %.3g; %d of %d levels differ from F.softmax's" % (s_x, alpha, C, worst, differ, total))
    assert worst < 1.0


# ---------------------------------------------------------------------------------------------------
# 8: the modules
# ---------------------------------------------------------------------------------------------------
STATE_KEYS = ["scores.output_scale", "scores.output_shift", "softmax.table", "softmax.output_scale", "softmax.output_shift",
              "context.output_scale", "context.output_shift"]


def _core(D, **kw):
    from torchlsq.quantized import AttentionCoreW8Q
    span = 6.0 * A.QKV_S * A.QKV_S * 74 * 74 * D ** 0.5
    return AttentionCoreW8Q(A.trained(-span, span), A.trained(0.0, 1.0), A.trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16, **kw)


def _qkv(B, H, Tq, Tk, D, seed):
    from torchlsq.functional import LevelsTensor
    s, z = one(A.QKV_S), one(A.QKV_Z, torch.int32)
    return [LevelsTensor(A.levels((B, H, T, D), 70 + seed + i, U8), s, z, 0, 255) for i, T in enumerate((Tq, Tk, Tk))]


@pytest.mark.parametrize("Tq,Tk,causal,lengths", [(19, 19, True, [19, 7]), (19, 19, True, None), (1, 40, True, [40, 13]), (5, 40, 2, [0, 33]),
                                                  (7, 40, False, [12, 40])], ids=str)
def test_attention_core_masked_is_the_hand_composition(Tq, Tk, causal, lengths):
    from torchlsq.functional import LevelsTensor, lsq_bmm_w8_q, lsq_masked_softmax_w8_q
    B, H, D = 2, 3, 32
    core = _core(D, causal=causal)
    q, k, v = _qkv(B, H, Tq, Tk, D, Tq)
    lens = M.lens_tensor(lengths)
    got = core(q, k, v, key_lengths=lens)
    s = lsq_bmm_w8_q(q, k, True, *core.scores._out("output"), BF16)
    p = lsq_masked_softmax_w8_q(s, core.softmax.table, *core.softmax._out("output"), BF16, causal=causal, key_lengths=lens)
    y = lsq_bmm_w8_q(p, v, False, *core.context._out("output"), BF16)
    assert isinstance(got, LevelsTensor) and got.levels.shape == (B, Tq, H * D) and len(got.levels.unique()) > 16
    assert torch.equal(got.levels, y.levels.permute(0, 2, 1, 3).reshape(B, Tq, H * D))
    assert torch.equal(got.scale, y.scale) and torch.equal(got.zero_point, y.zero_point)
    # the probabilities beyond a row's prefix are the quantizer's level of 0, and the mask shows in the result
    off = None if causal is False else (Tk - Tq if causal is True else causal)
    n = torch.tensor(M.prefix_lengths((B, H, Tq, Tk), off, lengths)).view(B, H, Tq, 1)
    assert bool((p.levels[torch.arange(Tk).view(1, 1, 1, -1) >= n] == 0).all())
    if Tq == Tk:
        assert not torch.equal(got.levels, _core(D)(q, k, v).levels)
    # fused=True: a masked call runs the same three launches, the same bytes
    fused = _core(D, causal=causal, fused=True)
    assert torch.equal(fused(q, k, v, key_lengths=lens).levels, got.levels)
    assert list(core.state_dict()) == list(fused.state_dict()) == list(_core(D).state_dict()) == STATE_KEYS
    assert "causal" in repr(core) or causal is False


def test_unmasked_modules_call_the_unmasked_ops(monkeypatch):
    import torchlsq.quantized.modules.attn_w8 as W
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import SoftmaxW8Q
    calls = []

    def spy(name):
        real = getattr(W, name)

        def f(*a, **kw):
            calls.append(name)
            return real(*a, **kw)
        monkeypatch.setattr(W, name, f)
    for name in ("lsq_softmax_w8_q", "lsq_softmax_w8", "lsq_masked_softmax_w8_q", "lsq_masked_softmax_w8", "lsq_attention_w8_q"):
        spy(name)
    q, k, v = _qkv(2, 3, 19, 19, 32, 0)
    plain = _core(32)
    assert plain.causal is False and plain.softmax.causal is False
    want = plain(q, k, v)
    assert calls == ["lsq_softmax_w8_q"]
    with pytest.raises(AssertionError, match="q, k and v of one shape"):
        plain(q, *(LevelsTensor(t.levels[:, :, :7], t.scale, t.zero_point, 0, 255) for t in (k, v)))
    del calls[:]
    assert torch.equal(_core(32, causal=None)(q, k, v).levels, want.levels) and calls == ["lsq_softmax_w8_q"]
    del calls[:]
    assert torch.equal(_core(32, fused=True)(q, k, v).levels, want.levels) and calls[0] == "lsq_attention_w8_q" and "lsq_masked_softmax_w8_q" not in calls
    del calls[:]
    plain.causal = True
    assert plain.softmax.causal is True
    masked = plain(q, k, v)
    assert calls == ["lsq_masked_softmax_w8_q"] and not torch.equal(masked.levels, want.levels)
    del calls[:]
    full = torch.tensor([19, 19], dtype=torch.int32)
    plain.causal = False
    assert torch.equal(plain(q, k, v, key_lengths=full).levels, want.levels) and calls == ["lsq_masked_softmax_w8_q"]
    # SoftmaxW8Q alone: floats and levels, masked and not
    del calls[:]
    s = plain.scores(q, k)
    sm = SoftmaxW8Q(s.scale, None, 1.0, F32)
    sm(s)
    sm(s, key_lengths=full)
    smc = SoftmaxW8Q(s.scale, A.trained(0.0, 1.0), 1.0, BF16, causal=3)
    y = smc(s)
    assert calls == ["lsq_softmax_w8", "lsq_masked_softmax_w8", "lsq_masked_softmax_w8_q"] and y.levels.stride(-2) == 32
    M.same(y.levels, M.composed(s.levels, smc.table, smc._out("output"), BF16, M.prefix_lengths(s.shape, 3)))
    assert list(smc.state_dict()) == list(sm.state_dict()) == ["table", "output_scale", "output_shift"] and "causal=3" in repr(smc)


def test_decode_one_query_against_forty_keys():
    """Tq = 1, Tk = 40: the query sees the keys its batch has written, whatever the slots beyond hold"""
    core = _core(32, causal=True)
    q, k, v = _qkv(2, 3, 1, 40, 32, 5)
    lens = torch.tensor([40, 13], dtype=torch.int32)
    got = core(q, k, v, key_lengths=lens)
    assert got.levels.shape == (2, 1, 96)
    # batch 1 is the unmasked core on its first 13 keys; batch 0 on all 40
    from torchlsq.functional import LevelsTensor

    def cut(t, b, T):
        return LevelsTensor(t.levels[b:b + 1, :, :T], t.scale, t.zero_point, 0, 255)
    plain = _core(32)
    plain.softmax.row_pad = 16
    for b, T in ((0, 40), (1, 13)):
        from torchlsq.functional import lsq_bmm_w8_q, lsq_softmax_w8_q
        s = lsq_bmm_w8_q(cut(q, b, 1), cut(k, b, T), True, *plain.scores._out("output"), BF16)
        p = lsq_softmax_w8_q(s, plain.softmax.table, *plain.softmax._out("output"), BF16)
        y = lsq_bmm_w8_q(p, cut(v, b, T), False, *plain.context._out("output"), BF16)
        assert torch.equal(got.levels[b], y.levels[0].permute(1, 0, 2).reshape(1, 96)), b
    # unwritten slots: whatever k and v hold beyond the length does not reach the result -- p there is the level 0 and the
    # probabilities' zero point is 0, so v's bytes are multiplied by 0
    k2, v2 = k.levels.clone(), v.levels.clone()
    k2[1, :, 13:] = 255
    v2[1, :, 13:] = 255
    again = core(q, LevelsTensor(k2, k.scale, k.zero_point, 0, 255), LevelsTensor(v2, v.scale, v.zero_point, 0, 255), key_lengths=lens)
    assert torch.equal(again.levels, got.levels)


# ---------------------------------------------------------------------------------------------------
# 9: the ops' fake kernels and autograd kernels
# ---------------------------------------------------------------------------------------------------
def test_fake_kernels_and_autograd():
    from torch._subclasses.fake_tensor import FakeTensorMode
    x, tab = A.score_rows(2 * 3 * 5, 197, 0, I8).view(2, 3, 5, 197), A.table()
    lens = torch.tensor([3, 4], dtype=torch.int32)
    real = OPS.lsq_softmax_mask_w8_q8_q(x, tab, *M.INT8_Q, BF16, True, 0, lens, 16)
    real1 = OPS.lsq_softmax_mask_w8_q8_q(x, tab, *A.PROB_Q, BF16)
    with FakeTensorMode() as mode:
        def fk(args):
            return tuple(mode.from_tensor(t) if isinstance(t, torch.Tensor) else t for t in args)
        fx, ft, fl = fk((x, tab, lens))
        y = OPS.lsq_softmax_mask_w8_q8_q(fx, ft, *fk(M.INT8_Q), BF16, True, 0, fl, 16)
        assert y.shape == real.shape == x.shape and y.dtype == real.dtype == I8 and y.stride() == real.stride() == (3 * 5 * 208, 5 * 208, 208, 1)
        y = OPS.lsq_softmax_mask_w8_q8_q(fx, ft, *fk(A.PROB_Q), BF16)
        assert y.shape == x.shape and y.dtype == real1.dtype == U8 and y.stride() == real1.stride() == (3 * 5 * 197, 5 * 197, 197, 1)
        for mid in A.MIDS:
            y = OPS.lsq_softmax_mask_w8_q8(fx, ft, mid, False, 0, fl)
            assert y.shape == x.shape and y.dtype == mid and y.is_contiguous()
    for i in (0, 1):
        q = list(A.PROB_Q)
        q[i] = q[i].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="grad|inference"):
            OPS.lsq_softmax_mask_w8_q8_q(x, tab, *q, BF16, True, 0, lens, 1)
    assert not OPS.lsq_softmax_mask_w8_q8(x, tab, F32, True, 0, lens).requires_grad
