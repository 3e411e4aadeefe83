"""Split-key decode attention on 8-bit levels without a GPU (liblsq_hip_attn_decode_split_w8.so, include/lsq_hip_attn_decode_split_w8.h):
what the library exports, its plan, its workspace size and every refusal with its message (all host only); an EMULATION of the three
launches in int64 torch ops -- chunked score bytes, the maximum and the sum over a row's whole prefix, per-chunk context integers
corrected with the chunk's own key count, their sum over the chunks that start below nmax -- equal to the definition
(`attn_decode_w8_cases.definition`, the op's CPU path), which holds the algebra of the split before any kernel runs; and the wiring:
the op, the functional's `split=` and the module's attribute on CPU tensors give the bytes of `split=None`.
"""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch

import attn_decode_w8_cases as C
import attn_w8_cases as A
from helpers import demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_attn_decode_split_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_attn_decode_split_w8.so")
NAMES = sorted(["lsq_attn_decode_split_w8_abi_version", "lsq_attn_decode_split_w8_last_error", "lsq_attn_decode_split_w8",
                "lsq_attn_decode_split_w8_plan", "lsq_attn_decode_split_w8_workspace"])
LSQ_EINVAL = -1
OPS = torch.ops.torchlsq
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
Z3 = (A.QKV_Z,) * 3
NOTHING = dict(family="composition", grid=0, reduce_grid=0, threads=0, rows=0, chunk=0, splits=0, lds_bytes=0, store="elements",
               workspace_bytes=0)
STATE_KEYS = ["scores.output_scale", "scores.output_shift", "softmax.table", "softmax.output_scale", "softmax.output_shift",
              "context.output_scale", "context.output_shift"]
ASSUMED_CUS = 256


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_attn_decode_split_w8\w*)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_ATTN_DECODE_SPLIT_W8) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_"))) == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "hipMalloc", "Synchronize", "lsq_hip_", "lsq_group_", "lsq_attn_", "lsq_bmm_", "lsq_softmax_", "lsq_rope_"):
        assert other not in und, other
    assert E.attn_decode_split_w8_library().lsq_attn_decode_split_w8_abi_version() == E.ATTN_DECODE_SPLIT_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_ATTN_DECODE_SPLIT_W8_ABI_VERSION (\d+)", raw).group(1) == "1"
    assert int(re.search(r"#define LSQ_ATTN_DECODE_SPLIT_W8_CUS (\d+)", raw).group(1)) == ASSUMED_CUS


def test_the_kernels(tmp_path):
    """three kernels: no scratch, no atomics; the int8 matrix-core instruction in the first two, 64-bit stores of the chunk's integers"""
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    short = sorted(re.search(r"lsq::(\w+)\(", n).group(1) for n in names.values())
    assert short == ["attn_split_context_kernel", "attn_split_reduce_kernel", "attn_split_scores_kernel"], names
    for mangled, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0, "%s uses %d bytes of scratch" % (names[mangled], scratch)
        assert not any("atomic" in o for o in ops), names[mangled]
        if "reduce" not in names[mangled]:
            assert ops.count("v_mfma_i32_16x16x64_i8") >= 5 and "s_barrier" in ops, names[mangled]
        if "scores" in names[mangled]:
            assert ops.count("global_load_dwordx4") >= 8 and "global_store_dwordx4" in ops, "four sub-tiles of two k packets in flight"
        if "context" in names[mangled]:
            assert "global_store_dwordx2" in ops


# ---------------------------------------------------------------------------------------------------
# the plan and the workspace
# ---------------------------------------------------------------------------------------------------
def _ws(B, H, Hkv, Tq, Tk, D, splits):
    R = H // Hkv * Tq
    return B * Hkv * R * 16 * ((Tk + 15) // 16) + 8 * B * Hkv * splits * R * D


def _expected(B, H, Hkv, Tq, Tk, D, chunk, store="packets"):
    S = -(-Tk // chunk)
    return dict(family="split", grid=B * Hkv * S, reduce_grid=B * Hkv, threads=256, rows=H // Hkv * Tq, chunk=chunk, splits=S,
                lds_bytes=3840 + 160 * D, store=store, workspace_bytes=_ws(B, H, Hkv, Tq, Tk, D, S))


def test_plans_without_a_gpu():
    from torchlsq import extension as E
    P = E.attn_decode_split_w8_plan
    # the shape single-stream decoding against a long cache has: 8 workgroups in the single-launch kernel, 256 here
    miss = P(1, 32, 8, 1, 8192, 128)
    assert miss == _expected(1, 32, 8, 1, 8192, 128, 256) and miss["grid"] >= ASSUMED_CUS and miss["splits"] == 32
    assert E.attn_decode_w8_plan(1, 32, 8, 1, 8192, 128)["grid"] == 8
    assert P(1, 32, 8, 1, 8192, 128, "auto") == miss
    # a grid that fills the part: "auto" keeps the single-launch kernel
    full = P(32, 32, 32, 1, 2048, 128, "auto")
    assert full["family"] == "decode" and full["splits"] == 0 and full == dict(E.attn_decode_w8_plan(32, 32, 32, 1, 2048, 128), splits=0)
    assert P(32, 32, 8, 1, 2048, 128, "auto")["family"] == "split"            # 256 workgroups: one a CU, the largest measured to win
    assert P(33, 32, 8, 1, 2048, 128, "auto")["family"] == "decode"
    assert P(1, 32, 8, 1, 8192, 128, "auto", cu_count=4)["family"] == "decode"          # eight workgroups on four CUs
    assert P(1, 32, 8, 1, 511, 128, "auto")["family"] == "decode"              # less than two chunks
    assert P(1, 32, 8, 1, 512, 128, "auto")["family"] == "split"
    # beyond the single-launch kernel: split where that plan says composition
    assert E.attn_decode_w8_plan(1, 32, 8, 1, 8193, 128)["family"] == "composition"
    assert P(1, 32, 8, 1, 8193, 128) == _expected(1, 32, 8, 1, 8193, 128, 256) == P(1, 32, 8, 1, 8193, 128, "auto")
    assert P(32, 32, 32, 1, 8193, 128, "auto")["family"] == "split"
    assert P(1, 1, 1, 1, 65536, 16) == _expected(1, 1, 1, 1, 65536, 16, 1024) and P(1, 32, 8, 1, 32768, 128)["chunk"] == 512
    # the library's chunk: the fewest splits whose grid reaches four workgroups a CU, at most 64, dealt evenly, the chunk taken into
    # [256, 2048]
    assert P(64, 32, 8, 1, 8192, 128)["chunk"] == 2048 and P(32, 32, 8, 1, 8192, 128)["chunk"] == 2048 and P(32, 32, 8, 1, 8192, 128)["grid"] == 1024
    assert P(16, 32, 8, 1, 8192, 128)["chunk"] == 1024 and P(8, 32, 8, 1, 8192, 128)["chunk"] == 512
    assert P(4, 32, 8, 1, 8192, 128)["chunk"] == 256 and P(2, 32, 8, 1, 8192, 128)["chunk"] == 256
    assert P(1, 1, 1, 1, 100, 16) == _expected(1, 1, 1, 1, 100, 16, 256) and P(12, 96, 8, 1, 8192, 128)["chunk"] == 768
    # forced splits: the chunk is 64 ceil(ceil(Tk / 64) / s)
    for shape, s, chunk in (((1, 1, 1, 1, 130, 16), 3, 64), ((1, 16, 1, 1, 65, 64), 2, 64), ((2, 8, 2, 1, 200, 32), 2, 128),
                            ((2, 8, 2, 1, 200, 32), 4, 64), ((1, 8, 1, 2, 197, 128), 4, 64), ((1, 4, 1, 1, 1024, 64), 1, 1024),
                            ((1, 4, 1, 1, 1024, 64), 4, 256), ((1, 4, 1, 1, 1024, 64), 16, 64), ((1, 1, 1, 1, 65536, 16), 1, 65536)):
        pl = P(*shape, s)
        assert pl == _expected(*shape, chunk) and pl["splits"] == s, (shape, s)
    assert P(1, 1, 1, 1, 320, 16, 4)["splits"] == 3                           # five 64-key units over at most four splits: chunks of 128
    # what is not served: R 17, D 24 / 8 / 144, strides and bases that are not multiples of 16; y's only changes the store
    assert P(1, 17, 1, 1, 64, 64) == NOTHING and P(1, 6, 2, 6, 64, 64) == NOTHING and P(1, 16, 1, 1, 64, 64)["rows"] == 16
    assert P(1, 2, 1, 1, 64, 24) == NOTHING and P(1, 2, 1, 1, 64, 8) == NOTHING and P(1, 2, 1, 1, 64, 144) == NOTHING
    q_dense, kv_dense = (4 * 2 * 64, 2 * 64, 64), (2 * 40 * 64, 40 * 64, 64)
    for name, dense in (("q_strides", q_dense), ("k_strides", kv_dense), ("v_strides", kv_dense)):
        for i in range(3):
            bad = tuple(s + (8 if j == i else 0) for j, s in enumerate(dense))
            assert P(2, 4, 2, 2, 40, 64, **{name: bad}) == NOTHING, (name, i)
        assert P(2, 4, 2, 2, 40, 64, **{name: tuple(s + 16 for s in dense)})["family"] == "split"
    assert P(2, 4, 2, 2, 40, 64, qkv_aligned=False) == NOTHING
    assert P(2, 4, 2, 2, 40, 64, 1, y_aligned=False) == _expected(2, 4, 2, 2, 40, 64, 64, "elements")
    # neither the dtypes nor the mask move the plan
    assert P(2, 6, 3, 1, 19, 32, 1, q_dtype=I8, k_dtype=U8, v_dtype=I8, causal=True, causal_offset=18, has_lengths=False) == \
        _expected(2, 6, 3, 1, 19, 32, 64)


def _geom(E, B=1, H=2, Hkv=2, Tq=8, Tk=8, D=16, dt=(0, 0, 0), causal=0, off=0, lens=0, q=None, k=None, v=None, y=None):
    d = E.LsqAttnW8Strides(H * 8 * 16, 8 * 16, 16)
    return E.LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, *dt, causal, off, lens, q or d, k or d, v or d, y or d)


def test_plan_and_workspace_refusals_without_a_gpu():
    from torchlsq import extension as E
    lib = E.attn_decode_split_w8_library()
    err = lib.lsq_attn_decode_split_w8_last_error
    out, ws = (ctypes.c_int32 * 8)(), ctypes.c_int64(-1)
    S = E.LsqAttnW8Strides

    def plan(g, splits=0):
        return lib.lsq_attn_decode_split_w8_plan(ctypes.byref(g), 1, 1, splits, ctypes.byref(out))

    def space(g, splits=0):
        return lib.lsq_attn_decode_split_w8_workspace(ctypes.byref(g), splits, ctypes.byref(ws))

    assert plan(_geom(E)) == 0 and list(out) == [1, 2, 256, 8, 256, 1, 3840 + 160 * 16, 1]    # (the last: packets)
    assert space(_geom(E)) == 0 and ws.value == 2 * 8 * 16 + 8 * 2 * 8 * 16
    assert lib.lsq_attn_decode_split_w8_plan(None, 1, 1, 0, ctypes.byref(out)) == LSQ_EINVAL and b"NULL geometry" in err()
    assert lib.lsq_attn_decode_split_w8_plan(ctypes.byref(_geom(E)), 1, 1, 0, None) == LSQ_EINVAL and b"NULL output" in err()
    assert lib.lsq_attn_decode_split_w8_workspace(None, 0, ctypes.byref(ws)) == LSQ_EINVAL and b"NULL geometry" in err()
    assert lib.lsq_attn_decode_split_w8_workspace(ctypes.byref(_geom(E)), 0, None) == LSQ_EINVAL and b"NULL bytes" in err()
    for f in (plan, space):
        for bad in (dict(B=0), dict(H=0), dict(Hkv=0), dict(Tq=0), dict(Tk=0), dict(D=0)):
            assert f(_geom(E, **bad)) == LSQ_EINVAL and b"at least 1" in err(), bad
        assert f(_geom(E, H=6, Hkv=4)) == LSQ_EINVAL and b"H = 6 query heads are not a multiple of Hkv = 4" in err()
        assert f(_geom(E, causal=1, off=-1)) == LSQ_EINVAL and b"causal_offset = -1 must be at least 0" in err()
        assert f(_geom(E, dt=(0, 2, 0))) == LSQ_EINVAL and b"must be LSQ_ATTN_W8_U8" in err()
        assert f(_geom(E, Tk=65537)) == LSQ_EINVAL and b"at most 65536" in err()
        assert f(_geom(E, Tq=(1 << 20) + 1)) == LSQ_EINVAL and b"2^20" in err()
        assert f(_geom(E, k=S(256, 128, 15))) == LSQ_EINVAL and b"k's row stride 15 is smaller" in err()
        assert f(_geom(E, v=S(-16, 128, 16))) == LSQ_EINVAL and b"must not be negative" in err()
        assert f(_geom(E, y=S(256, 64, 16))) == LSQ_EINVAL and b"overlap each other" in err()
        # splits: 0 .. ceil(Tk / 64)
        assert f(_geom(E), -1) == LSQ_EINVAL and b"splits = -1 must be 0" in err()
        assert f(_geom(E), 2) == LSQ_EINVAL and b"1 .. ceil(Tk / 64) = 1" in err()
        assert f(_geom(E, Tk=65), 2) == 0 and f(_geom(E, Tk=65), 3) == LSQ_EINVAL and b"ceil(Tk / 64) = 2" in err()
    assert plan(_geom(E, Tk=65536)) == 0 and out[0] == 1 and out[4] == 1024 and out[5] == 64
    big = S(0, 0, 1 << 17)
    assert plan(_geom(E, D=65552, q=big, k=big, v=big, y=big)) == LSQ_EINVAL and b"at most 65536" in err()
    # a geometry whose extents alone make it composition needs no workspace
    assert space(_geom(E, H=34, Hkv=2, Tq=1)) == 0 and ws.value == 0
    with pytest.raises(RuntimeError, match="splits must be an int"):
        E.attn_decode_split_w8_plan(1, 2, 2, 1, 64, 16, -1)
    with pytest.raises(RuntimeError, match=r"ceil\(Tk / 64\) = 1"):
        E.attn_decode_split_w8_plan(1, 2, 2, 1, 64, 16, 2)


def test_entry_refusals_without_a_gpu():
    """everything is checked before anything is enqueued: none of these calls reaches the runtime (the pointers are host memory)"""
    from torchlsq import extension as E
    lib = E.attn_decode_split_w8_library()
    err = lib.lsq_attn_decode_split_w8_last_error
    S = E.LsqAttnW8Strides
    B, H, Hkv, T, D = 2, 4, 2, 8, 16
    nq, nk = B * H * T * D, B * Hkv * T * D
    need = _ws(B, H, Hkv, T, T, D, 1)
    qkv = torch.zeros(8 * nq + 64, dtype=U8)
    ybuf = torch.zeros(4 * nq + 64, dtype=U8)
    wbuf = torch.full((need + 64,), 0x5A, dtype=U8)
    base = qkv.data_ptr() + (-qkv.data_ptr()) % 16
    yp = ybuf.data_ptr() + (-ybuf.data_ptr()) % 16
    wp = wbuf.data_ptr() + (-wbuf.data_ptr()) % 16
    f, z, tab = torch.ones(1), torch.zeros(1, dtype=torch.int32), A.table()
    lens = torch.zeros(B + 1, dtype=torch.int32)
    dq, dk = S(H * T * D, T * D, D), S(Hkv * T * D, T * D, D)

    def geom(**kw):
        a = dict(B=B, H=H, Hkv=Hkv, Tq=T, Tk=T, D=D, causal=0, off=0, has=1, q=dq, k=dk, v=dk, y=dq)
        a.update(kw)
        return E.LsqAttnDecodeW8Geom(a["B"], a["H"], a["Hkv"], a["Tq"], a["Tk"], a["D"], 0, 0, 0, a["causal"], a["off"], a["has"], a["q"], a["k"],
                                     a["v"], a["y"])

    def call(g=None, consts="ok", sides=None, table=tab.data_ptr(), kl=lens.data_ptr(), ptrs=None, y=yp, no_geom=False, ws=wp, ws_bytes=need,
             splits=0):
        g = g or geom()
        c = E.LsqAttnDecodeW8Consts(*([f.data_ptr(), z.data_ptr()] * 4)) if consts == "ok" else consts
        side = E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), 0, 255, 0, 255, 0)
        s = [side, side, side] if sides is None else sides
        p = ptrs or (base, base + nq, base + nq + nk)
        return lib.lsq_attn_decode_split_w8(None if no_geom else ctypes.byref(g), None if c is None else ctypes.byref(c),
                                            *(None if x is None else ctypes.byref(x) for x in s), table, kl, p[0], p[1], p[2], y, ws, ws_bytes,
                                            splits, None)

    # the decode entry's refusals
    assert call(no_geom=True) == LSQ_EINVAL and b"NULL geometry" in err()
    assert call(g=geom(H=6, Hkv=4)) == LSQ_EINVAL and b"not a multiple of Hkv" in err()
    assert call(g=geom(causal=1, off=-3)) == LSQ_EINVAL and b"causal_offset = -3" in err()
    assert call(consts=None) == LSQ_EINVAL and b"NULL constants" in err()
    assert call(consts=E.LsqAttnDecodeW8Consts(f.data_ptr(), z.data_ptr(), None, z.data_ptr(), f.data_ptr(), z.data_ptr(), f.data_ptr(),
                                               z.data_ptr())) == LSQ_EINVAL and b"NULL scale or zero point" in err()
    assert call(consts=E.LsqAttnDecodeW8Consts(*([f.data_ptr() + 1, z.data_ptr()] * 4))) == LSQ_EINVAL and b"element-aligned" in err()
    ok = E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), 0, 255, 0, 255, 0)
    assert call(sides=[ok, None, ok]) == LSQ_EINVAL and b"NULL output description" in err()
    assert call(sides=[ok, ok, E.LsqAttnW8Out(None, None, 0, 255, 0, 255, 0)]) == LSQ_EINVAL and b"levels out only" in err()
    assert call(sides=[ok, E.LsqAttnW8Out(f.data_ptr(), None, 0, 255, 0, 255, 0), ok]) == LSQ_EINVAL and b"come together" in err()
    assert call(sides=[ok, ok, E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), 0, 255, 0, 255, 2)]) == LSQ_EINVAL and b"one mid_dtype" in err()
    assert call(sides=[E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), 0, 255, 0, 255, 1)] * 3) == LSQ_EINVAL and b"mid_dtype must be" in err()
    assert call(sides=[ok, E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), -1, 255, 0, 255, 0), ok]) == LSQ_EINVAL and b"must lie within" in err()
    assert call(table=None) == LSQ_EINVAL and b"NULL buffer" in err()
    assert call(table=tab.data_ptr() + 2) == LSQ_EINVAL and b"table must be element-aligned" in err()
    assert call(y=None) == LSQ_EINVAL and b"NULL buffer" in err()
    assert call(kl=None) == LSQ_EINVAL and b"key_lengths is NULL" in err()
    assert call(g=geom(has=0)) == LSQ_EINVAL and b"key_lengths is given" in err()
    assert call(kl=lens.data_ptr() + 2) == LSQ_EINVAL and b"key_lengths must be 4-byte aligned" in err()
    assert call(y=base + 5) == LSQ_EINVAL and b"overlap" in err()
    assert call(ptrs=(base, base + nq, yp + 16)) == LSQ_EINVAL and b"overlap" in err()
    assert call(y=tab.data_ptr() + 16) == LSQ_EINVAL and b"overlap" in err()
    assert call(kl=yp + 4) == LSQ_EINVAL and b"overlap" in err()
    # legal, not served: the message says what to compose instead
    assert call(ptrs=(base + 1, base + nq, base + nq + nk)) == LSQ_EINVAL and b"not served by the split kernels" in err()
    d24q, d24k = S(H * T * 24, T * 24, 24), S(Hkv * T * 24, T * 24, 24)
    assert call(g=geom(D=24, q=d24q, k=d24k, v=d24k, y=d24q), ptrs=(base, base + 2 * nq, base + 4 * nq)) == LSQ_EINVAL and b"compose lsq_hip_attn_w8.h" in err()
    assert call(g=geom(H=2, Hkv=1, Tq=9, q=S(2 * 9 * D, 9 * D, D), y=S(2 * 9 * D, 9 * D, D))) == LSQ_EINVAL and b"G Tq <= 16" in err()
    # the splits and the workspace
    assert call(splits=-1) == LSQ_EINVAL and b"splits = -1" in err()
    assert call(splits=2) == LSQ_EINVAL and b"ceil(Tk / 64) = 1" in err()
    assert call(ws=None) == LSQ_EINVAL and b"NULL workspace" in err() and str(need).encode() in err()
    assert call(ws=wp + 8) == LSQ_EINVAL and b"workspace must be 16-byte aligned" in err()
    assert call(ws_bytes=need - 1) == LSQ_EINVAL and ("the workspace has %d bytes, %d are needed" % (need - 1, need)).encode() in err()
    assert call(ws_bytes=0) == LSQ_EINVAL and b"are needed" in err()
    for other, name in ((base + 16, "q"), (base + nq, "k"), (base + nq + nk + 32, "v"), (yp, "y"), (tab.data_ptr(), "table"),
                        (lens.data_ptr() - need + 4 + (-(lens.data_ptr() - need + 4)) % 16, "key_lengths")):
        assert call(ws=other) == LSQ_EINVAL and b"the workspace's" in err() and b"overlap" in err(), name
    assert bool((ybuf == 0).all()) and bool((wbuf == 0x5A).all())


# ---------------------------------------------------------------------------------------------------
# the three launches in int64 torch ops
# ---------------------------------------------------------------------------------------------------
def _levels(u, side):
    """the bytes of a quantizer's levels as integers in the quantizer's own range (signed where it is int8)"""
    lv = OPS.lsq_levels_per_tensor(u.contiguous(), *side, 0)
    return lv.view(I8 if max(side[3], side[5]) <= 127 else U8).to(torch.int64)


def _emulate(c, chunk):
    """scores per chunk, m and S over the whole prefix, I_c per chunk with the chunk's own key count, the sum over the chunks that
    start below nmax -> the levels [B, Tq, H D]"""
    from torchlsq.functional import _act_constants
    B, H, Hkv, Tq, Tk, D = c.shape
    G, S = c.G, -(-Tk // chunk)
    i64, f32 = torch.int64, torch.float32
    n = torch.tensor(C.key_counts(B, Tq, Tk, c.causal, None if c.lengths is None else c.lengths.tolist()))          # [B, Tq]
    nmax = n[:, -1]
    assert bool((n.max(dim=1).values == nmax).all())
    zq, zk, zv = (int(x.zero_point) for x in (c.q, c.k, c.v))
    sq, sk, sv = (x.scale.to(f32) for x in (c.q, c.k, c.v))
    p_s, p_z = _act_constants(c.sides[1][0], c.sides[1][1], c.sides[1][4], c.sides[1][5])
    zp = int(p_z)
    q = c.q.levels.to(i64) - zq                                                                                  # [B, H, Tq, D]
    k = (c.k.levels.to(i64) - zk).repeat_interleave(G, dim=1)                                                    # [B, H, Tk, D]
    v = c.v.levels.to(i64).repeat_interleave(G, dim=1)                                                           # raw levels: the raw sums
    j = torch.arange(Tk).reshape(1, 1, 1, Tk)
    nr = n.reshape(B, 1, Tq, 1)
    live = j < nr                                                                                                # [B, 1, Tq, Tk]
    # launch 1: the score bytes chunk by chunk (one workgroup each), nothing at or beyond nmax is formed
    scores = torch.zeros((B, H, Tq, Tk), dtype=i64)
    written = torch.zeros((B, 1, 1, Tk), dtype=torch.bool)
    for s in range(S):
        for b in range(B):
            c0, c1 = s * chunk, min((s + 1) * chunk, int(nmax[b]))
            if c0 >= c1:
                continue
            I = torch.einsum("htd,hjd->htj", q[b], k[b, :, c0:c1])
            u = ((sk * I.to(f32)) * sq).to(c.mid)
            scores[b, :, :, c0:c1] = _levels(u, c.sides[0])
            written[b, :, :, c0:c1] = True
    assert bool((written | ~live).all()), "a row reads a score nobody wrote"
    # launch 2, per row: the byte maximum and the exact sum over the WHOLE prefix, the same for every chunk
    low = torch.iinfo(i64).min
    m = torch.where(live, scores, torch.full_like(scores, low)).max(dim=-1, keepdim=True).values
    E = torch.where(live, c.table.to(i64)[(m - scores).clamp(0, 255)], torch.zeros_like(scores))
    Ssum = E.sum(dim=-1, keepdim=True)
    rcp = torch.where(Ssum > 0, 1.0 / Ssum.to(f32), torch.zeros_like(Ssum, dtype=f32))
    p = _levels((E.to(f32) * rcp).to(c.mid), c.sides[1])
    p = torch.where(live, p, torch.full_like(p, zp))                                                             # the byte z_p from n_r on
    # launch 2, per chunk: the raw sums over the chunk's keys and the correction with the chunk's own count; launch 3: their sum
    total = torch.zeros((B, H, Tq, D), dtype=i64)
    for b in range(B):
        for s in range(S):
            c0, c1 = s * chunk, min((s + 1) * chunk, int(nmax[b]))
            if c0 >= int(nmax[b]):
                continue                                                                                         # never written, never read
            pc, vc = p[b, :, :, c0:c1], v[b, :, c0:c1]
            P = torch.einsum("htj,hjd->htd", pc, vc)
            Cs = vc.sum(dim=1).reshape(H, 1, D)
            Rs = pc.sum(dim=-1, keepdim=True)
            total[b] += P - zp * Cs - zv * Rs + (c1 - c0) * zp * zv
    u = ((sv * total.to(f32)) * p_s.to(f32)).to(c.mid)
    return _levels(u, c.sides[2]).permute(0, 2, 1, 3).reshape(B, Tq, H * D)


def _want_ints(c):
    return c.want.to(torch.int64)


@pytest.mark.parametrize("shape,chunk,causal,lengths", [((1, 2, 3, 5, 197, 32), 64, 125, None), ((1, 2, 3, 5, 197, 32), 64, True, (131,)),
                                                        ((2, 2, 4, 1, 200, 32), 128, True, (200, 129)), ((2, 2, 4, 1, 200, 32), 128, True, (0, -4)),
                                                        ((2, 2, 4, 1, 200, 32), 128, False, (128, 64))], ids=str)
@pytest.mark.parametrize("combo", [0, 1])
def test_the_three_launches_in_integers_equal_the_definition(shape, chunk, causal, lengths, combo):
    dtypes, unsigned = C.COMBOS[combo]
    c = C.case(*shape, 50, dtypes, unsigned, BF16, Z3, None, causal, lengths)
    C.check_not_degenerate(c)
    if lengths is None or min(lengths) > 0:
        assert len(c.want.unique()) > 16
    assert torch.equal(_emulate(c, chunk), _want_ints(c))
    assert torch.equal(_emulate(c, 64), _emulate(c, 256))                       # the chunk does not move a byte


def test_the_three_launches_with_quant_min_5():
    """the probabilities quantizer with quant_min = 5: its level of 0.0 is 5, its z_p is 0 -- the byte z_p, not the level of 0.0,
    fills [n_r, chunk end)"""
    c = C.case(2, 2, 4, 1, 200, 32, 51, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (150, 70))
    d = C.Case()
    d.shape, d.G, d.mid, d.causal, d.lengths, d.table = c.shape, c.G, c.mid, c.causal, c.lengths, c.table
    d.q, d.k, d.v = c.q, c.k, c.v
    p = c.sides[1]
    d.sides = (c.sides[0], (p[0], p[1], 5) + tuple(p[3:]), c.sides[2])
    C.finish(d)
    assert not torch.equal(d.want, c.want) and len(d.want.unique()) > 16
    assert torch.equal(_emulate(d, 128), _want_ints(d)) and torch.equal(_emulate(d, 64), _want_ints(d))


# ---------------------------------------------------------------------------------------------------
# the wiring: the op, the functional, the module
# ---------------------------------------------------------------------------------------------------
def _core(D, **kw):
    from torchlsq.quantized import AttentionCoreW8Q
    span = 6.0 * A.QKV_S * A.QKV_S * 74 * 74 * D ** 0.5
    return AttentionCoreW8Q(A.trained(-span, span), A.trained(0.0, 1.0), A.trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16, **kw)


def test_op_and_functional_with_split_on_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torchlsq import extension as E
    from torchlsq.functional import lsq_attention_decode_w8_q
    c = C.case(2, 2, 4, 1, 200, 32, 52, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (200, 129))
    C.check_not_degenerate(c)
    args = C.flat_args(c, "cpu")
    for splits in (0, 1, 2, 4):
        assert torch.equal(OPS.lsq_attention_decode_split_w8_q8_q(*args, splits), c.want), splits
    assert torch.equal(OPS.lsq_attention_decode_split_w8_q8_q(*args), c.want)
    with pytest.raises(RuntimeError, match=r"ceil\(Tk / 64\) = 4"):
        OPS.lsq_attention_decode_split_w8_q8_q(*args, 5)
    with pytest.raises(RuntimeError, match="splits must be an int"):
        OPS.lsq_attention_decode_split_w8_q8_q(*args, -1)
    out = torch.empty(2, 8, 1, 32, dtype=c.want.dtype)
    assert E.attn_decode_split_w8_q(*args, splits=2, out=out) is out and torch.equal(out.permute(0, 2, 1, 3).reshape(2, 1, 256), c.want)
    for split in (None, "auto", 1, 2, 4, 100):                                 # an int is at most one split per 64 keys
        y = lsq_attention_decode_w8_q(c.q, c.k, c.v, c.table, *c.sides, c.mid, causal=True, key_lengths=c.lengths, split=split)
        assert torch.equal(y.levels, c.want), split
    for bad in (0, -2, "yes", True, 1.5):
        with pytest.raises(AssertionError, match="split must be None"):
            lsq_attention_decode_w8_q(c.q, c.k, c.v, c.table, *c.sides, c.mid, causal=True, key_lengths=c.lengths, split=bad)
    # the decode op's schema is untouched; the new op's fake kernel and its refusal of grad
    assert "splits" not in str(OPS.lsq_attention_decode_w8_q8_q.default._schema)
    assert str(OPS.lsq_attention_decode_split_w8_q8_q.default._schema).endswith("Tensor? key_lengths=None, int splits=0) -> Tensor")
    with FakeTensorMode() as mode:
        fake = tuple(mode.from_tensor(t) if isinstance(t, torch.Tensor) else t for t in args)
        y = OPS.lsq_attention_decode_split_w8_q8_q(*fake, 2)
        assert y.shape == (2, 1, 256) and y.dtype == c.want.dtype
    a = list(args)
    a[1] = args[1].clone().requires_grad_(True)
    with pytest.raises(RuntimeError):
        OPS.lsq_attention_decode_split_w8_q8_q(*a, 2)


def test_module_split_attribute(monkeypatch):
    import pickle
    import torchlsq.quantized.modules.attn_w8 as W
    from torchlsq.quantized import AttentionCoreW8Q
    calls = []
    real = W.lsq_attention_decode_w8_q

    def spy(*a, **kw):
        calls.append(kw.get("split", "absent"))
        return real(*a, **kw)
    monkeypatch.setattr(W, "lsq_attention_decode_w8_q", spy)
    q, k, v = C.inputs(2, 2, 4, 1, 200, 32, 53)
    lens = C.lens_tensor((200, 77))
    dec, spl = _core(32, causal=True, decode=True), _core(32, causal=True, decode=True, split=2)
    assert AttentionCoreW8Q.split is None and dec.split is None and spl.split == 2
    assert list(dec.state_dict()) == list(spl.state_dict()) == STATE_KEYS
    want = dec(q, k, v, key_lengths=lens).levels
    assert calls == ["absent"] and len(want.unique()) > 16
    del calls[:]
    assert torch.equal(spl(q, k, v, key_lengths=lens).levels, want) and calls == [2]
    # the attribute round-trips through deepcopy and pickle and is no part of the state
    for clone in (copy.deepcopy(spl), pickle.loads(pickle.dumps(spl))):
        assert clone.split == 2 and torch.equal(clone(q, k, v, key_lengths=lens).levels, want)
    spl.load_state_dict(dec.state_dict())
    auto = copy.deepcopy(dec)
    auto.split = "auto"
    del calls[:]
    assert torch.equal(auto(q, k, v, key_lengths=lens).levels, want) and calls == ["auto"]
    # a module pickled before the attribute existed reads the class default and goes where it went
    old = copy.deepcopy(spl)
    del old.__dict__["split"]
    old = pickle.loads(pickle.dumps(old))
    del calls[:]
    assert "split" not in old.__dict__ and old.split is None and torch.equal(old(q, k, v, key_lengths=lens).levels, want)
    assert calls == ["absent"]
    # prefill=True with split: rows that fit the tile go through the split functional, a prompt goes where it went
    pre = _core(32, causal=True, prefill=True, split=4)
    del calls[:]
    assert torch.equal(pre(q, k, v, key_lengths=lens).levels, want) and calls == [4]
    q5 = C.inputs(2, 2, 4, 5, 200, 32, 54)[0]                                  # R = 20
    del calls[:]
    plain = _core(32, causal=True, prefill=True)
    assert torch.equal(pre(q5, k, v, key_lengths=lens).levels, plain(q5, k, v, key_lengths=lens).levels) and calls == []
    # neither decode nor prefill: split changes nothing
    three = _core(32, causal=True, split=2)
    k8, v8 = C.expanded(k, 4), C.expanded(v, 4)
    assert torch.equal(three(q, k8, v8, key_lengths=lens).levels, _core(32, causal=True)(q, k8, v8, key_lengths=lens).levels) and calls == []
    assert "split=2" in repr(spl) and "split" not in repr(dec) and "split" not in repr(three) and "split='auto'" in repr(auto)
    with pytest.raises(AssertionError, match="split must be None"):
        _core(32, split=0)
