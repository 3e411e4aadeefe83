"""Prefill attention on 8-bit levels (include/lsq_hip_attn_prefill_w8.h), everything that needs no GPU: the library's exports against
its header and `_abi.py`, its one kernel (scratch, the matrix-core instruction and the barriers, from the code object), the plan and
its LDS formula over a sweep and on both sides of every threshold, every refusal with its message, the order in which the host
dispatches, the op on the CPU (the decode op's path: the definition), the module's `prefill=` option, the fake kernel and the
Autograd kernel, and the non-degeneracy of the references the GPU tests compare against.
"""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch

import attn_decode_w8_cases as C
import attn_prefill_w8_cases as P
import attn_w8_cases as A
from helpers import demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_attn_prefill_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_attn_prefill_w8.so")
NAMES = sorted(["lsq_attn_prefill_w8_abi_version", "lsq_attn_prefill_w8_last_error", "lsq_attn_prefill_w8", "lsq_attn_prefill_w8_plan"])
LSQ_EINVAL = -1
OPS = torch.ops.torchlsq
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
NOTHING = dict(family="composition", grid=0, threads=0, rows=0, lds_row_stride=0, lds_bytes=0, lds_dynamic=False, store="elements")
STATE_KEYS = ["scores.output_scale", "scores.output_shift", "softmax.table", "softmax.output_scale", "softmax.output_shift",
              "context.output_scale", "context.output_shift"]


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_attn_prefill_w8\w*)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_ATTN_PREFILL_W8) == NAMES
    # the geometry, the constants, the strides and the output side are the decode header's: included, not copied
    assert '#include "lsq_hip_attn_decode_w8.h"' in raw and "typedef struct" not in text
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_"))) == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_", "lsq_requant_", "lsq_resadd_",
                  "lsq_pool_", "lsq_dwconv_", "lsq_eltwise_", "lsq_norm_", "lsq_attn_", "lsq_bmm_", "lsq_softmax_", "lsq_rope_"):
        assert other not in und, other
    assert E.attn_prefill_w8_library().lsq_attn_prefill_w8_abi_version() == E.ATTN_PREFILL_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_ATTN_PREFILL_W8_ABI_VERSION (\d+)", raw).group(1) == "1"
    assert E.C_ABI_ATTN_PREFILL_W8["lsq_attn_prefill_w8"] == E.C_ABI_ATTN_DECODE_W8["lsq_attn_decode_w8"], "the same argument list"


def test_the_kernel(tmp_path):
    """one kernel: no scratch, no atomics, the int8 matrix-core instruction, packet loads of q and k and packet stores of y, LDS in
    use; five workgroup barriers: the table's, two per step of the context's loop, two around the level tile"""
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    assert len(every) == 1 and re.match(r"^(?:void )?lsq::attn_prefill_w8_kernel\(", list(names.values())[0]), names
    (body, scratch), = every.values()
    ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
    assert scratch == 0, "the kernel uses %d bytes of scratch" % scratch
    assert ops.count("v_mfma_i32_16x16x64_i8") >= 8 and not any("atomic" in o for o in ops)
    assert ops.count("global_load_dwordx4") >= 4, "q's and k's packets"
    assert "global_store_dwordx4" in ops and any(o.startswith("ds_read_b128") or o.startswith("ds_load_b128") for o in ops)
    assert ops.count("s_barrier") == 5


# ---------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------
def _expected(B, H, Hkv, Tq, Tk, D, causal=False, off=0, store="packets"):
    tk_eff = min(Tk, Tq + min(off, Tk)) if causal else Tk
    ld = P.ld_of(tk_eff)
    lds = 64 * ld + 1024 + 80 * D
    return dict(family="prefill", grid=B * H * ((Tq + 63) // 64), threads=256, rows=64, lds_row_stride=ld, lds_bytes=lds,
                lds_dynamic=lds > 65536, store=store)


def test_plans_without_a_gpu():
    from torchlsq import extension as E
    Pl = E.attn_prefill_w8_plan
    # a sweep of (Tq, Tk, D, causal, offset): every served plan by the header's formulas
    n = 0
    for Tq in (1, 16, 17, 64, 65, 130, 512, 2048, 5000):
        for Tk in (1, 17, 64, 197, 1024, 2048, 8192):
            for D in (16, 64, 80, 128):
                for causal, off in ((False, 0), (True, 0), (True, 5), (True, max(Tk - Tq, 0)), (True, 70000)):
                    pl = Pl(2, 8, 2, Tq, Tk, D, causal=causal, causal_offset=off)
                    tk_eff = min(Tk, Tq + min(off, Tk)) if causal else Tk
                    if tk_eff <= 2048:
                        assert pl == _expected(2, 8, 2, Tq, Tk, D, causal, off), (Tq, Tk, D, causal, off)
                        assert pl["lds_bytes"] <= 143360 and pl["lds_row_stride"] % 32 == 16
                        n += 1
                    else:
                        assert pl == NOTHING, (Tq, Tk, D, causal, off)
    assert n > 500
    # any Tq and any G are served, G Tq <= 16 too (the host's dispatch, not the library, prefers the decode kernel there)
    assert Pl(1, 16, 1, 1, 64, 64)["family"] == "prefill" and Pl(1, 32, 8, 1000, 64, 64)["grid"] == 32 * 16
    # Tk_eff on both sides of 2048: not causal it is Tk; causal it is min(Tk, Tq + offset), and the offset is clamped to Tk
    assert Pl(1, 1, 1, 17, 2048, 32) == _expected(1, 1, 1, 17, 2048, 32) and Pl(1, 1, 1, 17, 2049, 32) == NOTHING
    assert Pl(1, 1, 1, 2048, 8192, 128, causal=True, causal_offset=0)["lds_bytes"] == 64 * 2064 + 1024 + 10240 == 143360
    assert Pl(1, 1, 1, 2049, 8192, 128, causal=True, causal_offset=0) == NOTHING
    assert Pl(1, 1, 1, 2000, 8192, 128, causal=True, causal_offset=48)["family"] == "prefill"
    assert Pl(1, 1, 1, 2000, 8192, 128, causal=True, causal_offset=49) == NOTHING
    assert Pl(1, 1, 1, 17, 2049, 32, causal=True, causal_offset=2032) == NOTHING       # causal=True of the functional form: Tk - Tq
    assert Pl(1, 1, 1, 17, 2049, 32, causal=True, causal_offset=2031)["lds_row_stride"] == 2064
    assert Pl(1, 1, 1, 32, 8192, 64, causal=True, causal_offset=100)["lds_row_stride"] == P.ld_of(132) == 144
    assert Pl(1, 1, 1, 17, 64, 32, causal=True, causal_offset=60000)["lds_row_stride"] == P.ld_of(64)
    # key_lengths lives on the device and does not enter
    assert Pl(1, 1, 1, 17, 2049, 32, has_lengths=True) == NOTHING and Pl(1, 1, 1, 17, 2048, 32, has_lengths=False)["family"] == "prefill"
    # D: 16 .. 128 in multiples of 16
    assert Pl(1, 2, 1, 20, 64, 16)["family"] == "prefill" and Pl(1, 2, 1, 20, 64, 24) == NOTHING and Pl(1, 2, 1, 20, 64, 8) == NOTHING
    assert Pl(1, 2, 1, 20, 64, 128)["family"] == "prefill" and Pl(1, 2, 1, 20, 64, 144) == NOTHING
    # one stride that is not a multiple of 16, per operand and per stride; y's only changes the store
    q_dense, kv_dense = (4 * 20 * 64, 20 * 64, 64), (2 * 40 * 64, 40 * 64, 64)
    for name, dense in (("q_strides", q_dense), ("k_strides", kv_dense), ("v_strides", kv_dense)):
        for i in range(3):
            for off in (8, 24):
                bad = tuple(s + (off if j == i else 0) for j, s in enumerate(dense))
                assert Pl(2, 4, 2, 20, 40, 64, **{name: bad}) == NOTHING, (name, i, off)
        assert Pl(2, 4, 2, 20, 40, 64, **{name: tuple(s + 16 for s in dense)})["family"] == "prefill"
    assert Pl(2, 4, 2, 20, 40, 64, qkv_aligned=False) == NOTHING
    assert Pl(2, 4, 2, 20, 40, 64, y_aligned=False) == _expected(2, 4, 2, 20, 40, 64, store="elements")
    assert Pl(2, 4, 2, 20, 40, 64, y_strides=(20 * 4 * 64 + 8, 64, 256)) == _expected(2, 4, 2, 20, 40, 64, store="elements")
    # the LDS row stride: 16 n with n odd; the bytes and where they pass 64 KB
    assert [Pl(1, 1, 1, 20, T, 64)["lds_row_stride"] for T in (1, 16, 17, 32, 33, 197, 2032, 2033, 2048)] == [16, 16, 48, 48, 48, 208, 2032, 2064, 2064]
    lo, hi = Pl(1, 1, 1, 20, 848, 128), Pl(1, 1, 1, 20, 849, 128)          # 64 * 848 + 1024 + 10240 = 65536; 64 * 880 + 11264 = 67584
    assert (lo["lds_bytes"], lo["lds_dynamic"], hi["lds_bytes"], hi["lds_dynamic"]) == (65536, False, 67584, True)
    # the dtypes do not move the plan
    assert Pl(2, 6, 3, 19, 19, 32, q_dtype=I8, k_dtype=U8, v_dtype=I8, causal=True, causal_offset=0, has_lengths=False) == \
        _expected(2, 6, 3, 19, 19, 32, True, 0)


def test_plan_refusals_without_a_gpu():
    from torchlsq import extension as E
    lib = E.attn_prefill_w8_library()
    err = lib.lsq_attn_prefill_w8_last_error
    out = (ctypes.c_int32 * 8)()
    S = E.LsqAttnW8Strides

    def G(B=1, H=2, Hkv=2, Tq=8, Tk=8, D=16, dt=(0, 0, 0), causal=0, off=0, lens=0, q=None, k=None, v=None, y=None):
        d = S(H * 8 * 16, 8 * 16, 16)
        return E.LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, *dt, causal, off, lens, q or d, k or d, v or d, y or d)

    def plan(g):
        return lib.lsq_attn_prefill_w8_plan(ctypes.byref(g), 1, 1, ctypes.byref(out))

    assert plan(G()) == 0 and out[0] == 1
    assert lib.lsq_attn_prefill_w8_plan(None, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"NULL geometry" in err()
    assert lib.lsq_attn_prefill_w8_plan(ctypes.byref(G()), 1, 1, None) == LSQ_EINVAL and b"NULL output" in err()
    for bad in (dict(B=0), dict(H=0), dict(Hkv=0), dict(Tq=0), dict(Tk=0), dict(D=0)):
        assert plan(G(**bad)) == LSQ_EINVAL and b"at least 1" in err(), bad
    assert plan(G(H=6, Hkv=4)) == LSQ_EINVAL and b"H = 6 query heads are not a multiple of Hkv = 4" in err()
    assert plan(G(causal=1, off=-1)) == LSQ_EINVAL and b"causal_offset = -1 must be at least 0" in err()
    assert plan(G(causal=0, off=-1)) == 0                                                        # not causal: the offset is not read
    assert plan(G(dt=(0, 2, 0))) == LSQ_EINVAL and b"must be LSQ_ATTN_W8_U8" in err()
    big = S(0, 0, 1 << 17)
    assert plan(G(D=65552, q=big, k=big, v=big, y=big)) == LSQ_EINVAL and b"at most 65536" in err()
    assert plan(G(Tk=65537)) == LSQ_EINVAL and b"at most 65536" in err()
    assert plan(G(Tk=65536)) == 0 and out[0] == 0
    assert plan(G(Tk=65536, causal=1, off=0)) == 0 and out[0] == 1 and out[4] == 16             # eight rows of a long cache
    assert plan(G(Tq=(1 << 20) + 1)) == LSQ_EINVAL and b"2^20" in err()
    assert plan(G(B=1 << 11, H=1 << 10, Hkv=1 << 10)) == LSQ_EINVAL and b"2^20" in err()
    assert plan(G(k=S(256, 128, 15))) == LSQ_EINVAL and b"k's row stride 15 is smaller" in err()
    assert plan(G(v=S(-16, 128, 16))) == LSQ_EINVAL and b"must not be negative" in err()
    assert plan(G(y=S(256, 64, 16))) == LSQ_EINVAL and b"overlap each other" in err()
    # a grid beyond 2^24 - 1 workgroups: B H = 2^20 with 17 row tiles
    wide = S(0, 0, 16)
    yy = S((1 << 10) * 1088 * 16, 1088 * 16, 16)
    assert plan(G(B=1 << 10, H=1 << 10, Hkv=1 << 10, Tq=1088, q=wide, k=wide, v=wide, y=yy)) == LSQ_EINVAL and b"beyond 2^24 - 1" in err()


def test_entry_refusals_without_a_gpu():
    """everything is checked before anything is enqueued: none of these calls reaches the runtime (the pointers are host memory)"""
    from torchlsq import extension as E
    lib = E.attn_prefill_w8_library()
    err = lib.lsq_attn_prefill_w8_last_error
    S = E.LsqAttnW8Strides
    B, H, Hkv, T, D = 2, 4, 2, 8, 16
    nq, nk = B * H * T * D, B * Hkv * T * D
    qkv = torch.zeros(8 * nq + 64, dtype=U8)                   # (room for the D = 24 geometry below)
    ybuf = torch.zeros(4 * nq + 64, dtype=U8)
    base = qkv.data_ptr() + (-qkv.data_ptr()) % 16
    yp = ybuf.data_ptr() + (-ybuf.data_ptr()) % 16
    f, z, tab = torch.ones(1), torch.zeros(1, dtype=torch.int32), A.table()
    lens = torch.zeros(B + 1, dtype=torch.int32)
    dq, dk = S(H * T * D, T * D, D), S(Hkv * T * D, T * D, D)

    def geom(**kw):
        a = dict(B=B, H=H, Hkv=Hkv, Tq=T, Tk=T, D=D, causal=0, off=0, has=1, q=dq, k=dk, v=dk, y=dq)
        a.update(kw)
        return E.LsqAttnDecodeW8Geom(a["B"], a["H"], a["Hkv"], a["Tq"], a["Tk"], a["D"], 0, 0, 0, a["causal"], a["off"], a["has"], a["q"], a["k"],
                                     a["v"], a["y"])

    def call(g=None, consts="ok", sides=None, table=tab.data_ptr(), kl=lens.data_ptr(), ptrs=None, y=yp, no_geom=False):
        g = g or geom()
        c = E.LsqAttnDecodeW8Consts(*([f.data_ptr(), z.data_ptr()] * 4)) if consts == "ok" else consts
        side = E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), 0, 255, 0, 255, 0)
        s = [side, side, side] if sides is None else sides
        p = ptrs or (base, base + nq, base + nq + nk)
        return lib.lsq_attn_prefill_w8(None if no_geom else ctypes.byref(g), None if c is None else ctypes.byref(c),
                                       *(None if x is None else ctypes.byref(x) for x in s), table, kl, p[0], p[1], p[2], y, None)

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
    assert call(sides=[ok, E.LsqAttnW8Out(f.data_ptr(), f.data_ptr() + 2, 0, 255, 0, 255, 0), ok]) == LSQ_EINVAL
    assert call(sides=[ok, ok, E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), 0, 255, 0, 255, 2)]) == LSQ_EINVAL and b"one mid_dtype" in err()
    assert call(sides=[E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), 0, 255, 0, 255, 1)] * 3) == LSQ_EINVAL and b"mid_dtype must be" in err()
    assert call(sides=[ok, E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), -1, 255, 0, 255, 0), ok]) == LSQ_EINVAL and b"must lie within" in err()
    assert call(sides=[ok, E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), 9, 3, 0, 255, 0), ok]) == LSQ_EINVAL
    assert call(table=None) == LSQ_EINVAL and b"NULL buffer" in err()
    assert call(table=tab.data_ptr() + 2) == LSQ_EINVAL and b"table must be element-aligned" in err()
    assert call(y=None) == LSQ_EINVAL and b"NULL buffer" in err()
    assert call(ptrs=(base, None, base + nq)) == LSQ_EINVAL and b"NULL buffer" in err()
    # key_lengths: NULL where the geometry asks for it, given where it does not, misaligned
    assert call(kl=None) == LSQ_EINVAL and b"key_lengths is NULL" in err()
    assert call(g=geom(has=0)) == LSQ_EINVAL and b"key_lengths is given" in err()
    assert call(kl=lens.data_ptr() + 2) == LSQ_EINVAL and b"key_lengths must be 4-byte aligned" in err()
    # y overlapping q, k, v, the table or key_lengths
    assert call(y=base + 5) == LSQ_EINVAL and b"overlap" in err()                                 # y inside q
    assert call(y=base + nq + 5) == LSQ_EINVAL and b"overlap" in err()                            # y reaches into k
    assert call(ptrs=(base, base + nq, yp + 16)) == LSQ_EINVAL and b"overlap" in err()            # v inside y
    assert call(y=tab.data_ptr() + 16) == LSQ_EINVAL and b"overlap" in err()                      # y inside the table
    assert call(kl=yp + 4) == LSQ_EINVAL and b"overlap" in err()                                  # key_lengths inside y
    # legal, not served: the message says what to compose instead
    assert call(ptrs=(base + 1, base + nq, base + nq + nk)) == LSQ_EINVAL and b"not served by the prefill kernel" in err()
    d24q, d24k = S(H * T * 24, T * 24, 24), S(Hkv * T * 24, T * 24, 24)
    assert call(g=geom(D=24, q=d24q, k=d24k, v=d24k, y=d24q), ptrs=(base, base + 2 * nq, base + 4 * nq)) == LSQ_EINVAL and b"compose lsq_hip_attn_w8.h" in err()
    far, long = S(0, 0, D), torch.zeros(2049 * D + 64, dtype=U8)       # Tk_eff = 2049: one cache of 2049 rows for every (b, kv head)
    lp = long.data_ptr() + (-long.data_ptr()) % 16
    assert call(g=geom(Tk=2049, k=far, v=far), ptrs=(base, lp, lp)) == LSQ_EINVAL and b"<= 2048" in err()
    assert call(g=geom(Tk=2049, k=far, v=far, causal=1, off=2041), ptrs=(base, lp, lp)) == LSQ_EINVAL and b"<= 2048" in err()
    assert bool((ybuf == 0).all())


# ---------------------------------------------------------------------------------------------------
# the host's dispatch
# ---------------------------------------------------------------------------------------------------
def test_dispatch_order(monkeypatch):
    """on the GPU: the decode kernel where its plan says "decode", else the prefill kernel where its plan says "prefill", else the
    decode host's composition; on the CPU always the decode host's path.  The device is faked: nothing is launched"""
    import torchlsq._attn_decode_w8_host as DH
    import torchlsq._attn_prefill_w8_host as PH
    calls = []
    real_checked, real_run = DH._checked, DH._run
    fake_gpu = [True]

    def checked(*a, **kw):
        st = real_checked(*a, **kw)
        st.on_gpu = fake_gpu[0]
        return st

    def run(st, what):
        calls.append(("decode host", what))
        st.on_gpu = False                   # (the operands are on the CPU)
        return real_run(st, what)

    def launch(st, lib, entry, err):
        calls.append(("launch", entry, err))
        assert lib is PH.attn_prefill_w8_library()

    monkeypatch.setattr(DH, "_checked", checked)
    monkeypatch.setattr(DH, "_run", run)
    monkeypatch.setattr(DH, "_launch", launch)
    from torchlsq import extension as E

    def go(c):
        del calls[:]
        return E.attn_prefill_w8_q(*C.flat_args(c, "cpu"))

    # 1 G Tq <= 16: the decode host, although the prefill plan serves the shape too
    c = P.case(1, 2, 2, 8, 40, 32, 20, causal=True)
    assert C.plan_of(c)["family"] == "decode" and P.plan_of(c)["family"] == "prefill"
    assert torch.equal(go(c), c.want) and calls == [("decode host", "lsq_attention_prefill_w8_q8_q")]
    # 2 G Tq = 18: ONE call of the prefill library's entry
    c = P.case(1, 2, 2, 9, 40, 32, 20, causal=True)
    assert C.plan_of(c)["family"] == "composition" and P.plan_of(c)["family"] == "prefill"
    go(c)
    assert calls == [("launch", "lsq_attn_prefill_w8", "lsq_attn_prefill_w8_last_error")]
    # 3 neither: the decode host, which composes
    c = P.case(1, 2, 2, 9, 40, 24, 20, causal=True)
    assert C.plan_of(c)["family"] == "composition" and P.plan_of(c)["family"] == "composition"
    assert torch.equal(go(c), c.want) and calls == [("decode host", "lsq_attention_prefill_w8_q8_q")]
    # G Tq <= 16 at D 24: the decode plan says "composition", the prefill plan too
    c = P.case(1, 2, 2, 4, 40, 24, 20, causal=True)
    assert torch.equal(go(c), c.want) and calls == [("decode host", "lsq_attention_prefill_w8_q8_q")]
    # the CPU: always the decode host's path, whatever the plans say
    fake_gpu[0] = False
    c = P.case(1, 2, 2, 9, 40, 32, 20, causal=True)
    assert torch.equal(go(c), c.want) and calls == [("decode host", "lsq_attention_prefill_w8_q8_q")]
    # an illegal shape is refused with the library's message before anything else happens (here: by the shared host checks)
    bad = list(C.flat_args(c, "cpu"))
    bad[30] = -1
    with pytest.raises(RuntimeError, match="lsq_attention_prefill_w8_q8_q: causal_offset = -1 must be at least 0"):
        E.attn_prefill_w8_q(*bad)


def test_the_host_never_reads_key_lengths(monkeypatch):
    import torchlsq._attn_decode_w8_host as DH
    c = P.case(1, 2, 2, 9, 40, 32, 20, causal=True, lengths=(30,))
    real = DH._checked

    class Untouchable(torch.Tensor):
        @classmethod
        def __torch_function__(cls, func, types, args=(), kwargs=None):
            name = getattr(func, "__name__", str(func))
            assert name not in ("item", "tolist", "__int__", "__index__", "__bool__", "numpy", "cpu"), name
            return super().__torch_function__(func, types, args, kwargs or {})

    def checked(*a, **kw):
        st = real(*a, **kw)
        st.on_gpu = True
        return st
    monkeypatch.setattr(DH, "_checked", checked)
    monkeypatch.setattr(DH, "_launch", lambda *a: None)
    from torchlsq import extension as E
    args = list(C.flat_args(c, "cpu"))
    args[31] = args[31].as_subclass(Untouchable)
    E.attn_prefill_w8_q(*args)


# ---------------------------------------------------------------------------------------------------
# the op on the CPU, the module
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal,lengths", [(0, None), (0, (40, 23)), (True, (19, 7)), (False, (12, 40)), (2, (0, 33))], ids=str)
def test_op_on_the_cpu_is_the_definition_and_the_masked_core_on_expanded_k_and_v(causal, lengths):
    from torchlsq.functional import LevelsTensor, lsq_attention_decode_w8_q, lsq_attention_prefill_w8_q
    B, Hkv, G, T, D = 2, 2, 4, 40, 64
    core = P.core(D, causal=causal)
    q, k, v = C.inputs(B, Hkv, G, T, T, D, 21)
    lens = C.lens_tensor(lengths)
    sides = P.core_sides(core)
    want = lsq_attention_decode_w8_q(q, k, v, core.softmax.table, *sides, BF16, causal=causal, key_lengths=lens)
    got = lsq_attention_prefill_w8_q(q, k, v, core.softmax.table, *sides, BF16, causal=causal, key_lengths=lens)
    assert isinstance(got, LevelsTensor) and got.levels.shape == (B, T, Hkv * G * D) and got.levels.dtype == U8 and len(got.levels.unique()) > 16
    assert torch.equal(got.levels, want.levels) and torch.equal(got.scale, want.scale) and torch.equal(got.zero_point, want.zero_point)
    assert (got.quant_min, got.quant_max, got.type_min, got.type_max) == (want.quant_min, want.quant_max, want.type_min, want.type_max)
    # shift 0: the probabilities quantizer's level of 0.0 is its z_p, and the masked core on expanded k and v gives the same bytes
    old = core(q, C.expanded(k, G), C.expanded(v, G), key_lengths=lens)
    assert torch.equal(got.levels, old.levels)
    dec, pre = P.core(D, causal=causal, decode=True), P.core(D, causal=causal, prefill=True)
    assert torch.equal(pre(q, k, v, key_lengths=lens).levels, dec(q, k, v, key_lengths=lens).levels)
    assert torch.equal(pre(q, k, v, key_lengths=lens).levels, got.levels)


def test_module_prefill_option(monkeypatch):
    import torchlsq.quantized.modules.attn_w8 as W
    from torchlsq.quantized import AttentionCoreW8Q
    calls = []

    def spy(name):
        real = getattr(W, name)

        def f(*a, **kw):
            calls.append(name)
            return real(*a, **kw)
        monkeypatch.setattr(W, name, f)
    for name in ("lsq_softmax_w8_q", "lsq_masked_softmax_w8_q", "lsq_attention_w8_q", "lsq_attention_decode_w8_q", "lsq_attention_prefill_w8_q"):
        spy(name)
    q, k, v = C.inputs(2, 3, 1, 19, 19, 32, 40)
    lens = C.lens_tensor((19, 7))
    plain, dec, pre = P.core(32, causal=True), P.core(32, causal=True, decode=True), P.core(32, causal=True, prefill=True)
    assert plain.prefill is False and dec.prefill is False and pre.prefill is True and pre.decode is False and AttentionCoreW8Q.prefill is False
    assert list(plain.state_dict()) == list(pre.state_dict()) == STATE_KEYS and "prefill" not in dict(pre.named_buffers())
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), pre.state_dict().values()))
    want = plain(q, k, v, key_lengths=lens)
    assert calls == ["lsq_masked_softmax_w8_q"]
    del calls[:]
    assert torch.equal(pre(q, k, v, key_lengths=lens).levels, want.levels) and calls == ["lsq_attention_prefill_w8_q"]
    del calls[:]
    # prefill=True wins over fused and decode; unmasked calls go through it too
    both = P.core(32, fused=True, decode=True, prefill=True)
    assert torch.equal(both(q, k, v).levels, P.core(32)(q, k, v).levels) and calls[0] == "lsq_attention_prefill_w8_q"
    assert "lsq_attention_decode_w8_q" not in calls and "lsq_attention_w8_q" not in calls
    del calls[:]
    # prefill=False: every combination of fused and decode goes where it went
    dec(q, k, v, key_lengths=lens)
    assert calls[0] == "lsq_attention_decode_w8_q" and "lsq_attention_prefill_w8_q" not in calls
    del calls[:]
    P.core(32)(q, k, v)
    assert calls == ["lsq_softmax_w8_q"]
    del calls[:]
    P.core(32, fused=True)(q, k, v)
    assert calls[0] == "lsq_attention_w8_q" and "lsq_attention_prefill_w8_q" not in calls
    del calls[:]
    P.core(32, fused=True, causal=True)(q, k, v)
    assert calls == ["lsq_masked_softmax_w8_q"]
    del calls[:]
    P.core(32, fused=True, decode=True)(q, k, v)
    assert calls[0] == "lsq_attention_decode_w8_q" and "lsq_attention_prefill_w8_q" not in calls
    # grouped-query k and v
    q6 = C.inputs(2, 3, 2, 19, 19, 32, 41)[0]
    with pytest.raises(AssertionError, match="masked\\) needs q"):
        plain(q6, k, v, key_lengths=lens)
    assert torch.equal(pre(q6, k, v, key_lengths=lens).levels, dec(q6, k, v, key_lengths=lens).levels)
    # `causal` may change between calls: an offset for the prompt, True for the steps
    pre.causal = 0
    assert torch.equal(pre(q6, k, v).levels, pre(q6, k, v, key_lengths=C.lens_tensor((19, 19))).levels)
    # the attribute is not a buffer; a module pickled before it existed reads the class default
    old = copy.deepcopy(dec)
    del old.__dict__["prefill"]
    assert old.prefill is False and torch.equal(old(q, k, v, key_lengths=lens).levels, want.levels)
    assert "prefill=True" in repr(pre) and "lsq_attention_prefill_w8_q" in repr(pre) and "causal=0" in repr(pre)
    assert "prefill" not in repr(plain) and "prefill" not in repr(dec) and "three launches" in repr(plain) and "decode=True" in repr(dec)
    pre.load_state_dict(plain.state_dict())


def test_functional_form_and_argument_validation():
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, _act_constants, lsq_attention_prefill_w8_q
    c = C.case(2, 3, 2, 19, 19, 32, 13, C.COMBOS[0][0], C.COMBOS[0][1], BF16, (A.QKV_Z,) * 3, None, True, (19, 6))
    y = lsq_attention_prefill_w8_q(c.q, c.k, c.v, c.table, *c.sides, c.mid, causal=True, key_lengths=c.lengths)
    o = c.sides[2]
    s, z = _act_constants(o[0], o[1], o[4], o[5])
    assert isinstance(y, LevelsTensor) and torch.equal(y.levels, c.want) and torch.equal(y.scale, s) and torch.equal(y.zero_point, z)
    with pytest.raises(AssertionError, match="lsq_attention_prefill_w8_q: probs_out must be \\(scale, shift, quant_min"):
        lsq_attention_prefill_w8_q(c.q, c.k, c.v, c.table, c.sides[0], None, c.sides[2], c.mid)
    with pytest.raises(AssertionError, match="offset >= 0"):
        lsq_attention_prefill_w8_q(c.q, c.k, c.v, c.table, *c.sides, c.mid, causal=-1)
    with pytest.raises(AssertionError, match="needs Tk >= Tq"):
        lsq_attention_prefill_w8_q(C.with_levels(c.q, c.q.levels.expand(2, 6, 19, 32)[:, :, :1].expand(2, 6, 20, 32)), c.k, c.v, c.table,
                                   *c.sides, c.mid, causal=True)
    args = list(C.flat_args(c, "cpu"))
    assert torch.equal(OPS.lsq_attention_prefill_w8_q8_q(*args), c.want)

    def bad(i, v, match):
        a = list(args)
        a[i] = v
        with pytest.raises(RuntimeError, match=match):
            OPS.lsq_attention_prefill_w8_q8_q(*a)

    bad(0, args[0].to(torch.int16), "lsq_attention_prefill_w8_q8_q: the levels of q must be uint8")
    bad(3, args[3][:, :2], r"q must be \[B, H, Tq, D\]")
    bad(0, args[0][:, :5], "H = 5 query heads are not a multiple of Hkv = 3")
    bad(1, torch.ones(2), "scale must be one float32")
    bad(9, args[9].to(torch.int64), "table must be a dense int32")
    bad(12, -129, "must lie within")
    bad(28, torch.float64, "must be float32, bfloat16 or float16")
    bad(30, -1, "causal_offset = -1 must be at least 0")
    bad(31, torch.zeros(3, dtype=torch.int32), r"key_lengths must be a dense int32 tensor of \[2\]")
    out = torch.empty(2, 6, 19, 32, dtype=c.want.dtype)
    assert E.attn_prefill_w8_q(*args, out=out) is out and torch.equal(out.permute(0, 2, 1, 3).reshape(2, 19, 192), c.want)
    a = list(args)
    a[0] = args[0][:, :, :0]
    assert OPS.lsq_attention_prefill_w8_q8_q(*a).shape == (2, 0, 192)
    # the decode op says its own name, as before
    a = list(args)
    a[30] = -1
    with pytest.raises(RuntimeError, match="lsq_attention_decode_w8_q8_q: causal_offset"):
        OPS.lsq_attention_decode_w8_q8_q(*a)


def test_op_registration_fake_kernel_and_grad_refusal():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(OPS, "lsq_attention_prefill_w8_q8_q")
    assert str(OPS.lsq_attention_prefill_w8_q8_q.default._schema).replace("prefill", "decode") == str(OPS.lsq_attention_decode_w8_q8_q.default._schema)
    for unsigned, dtype in (((True, False, True), U8), ((True, True, False), I8)):
        c = C.case(2, 3, 2, 19, 19, 32, 14, C.ALL_U8, unsigned, BF16, (A.QKV_Z,) * 3, None, True, (19, 6))
        assert c.want.dtype == dtype
        real = C.flat_args(c, "cpu")
        with FakeTensorMode() as mode:
            args = tuple(mode.from_tensor(t) if isinstance(t, torch.Tensor) else t for t in real)
            y = OPS.lsq_attention_prefill_w8_q8_q(*args)
            assert y.shape == (2, 19, 192) and y.dtype == dtype and y.stride() == (19 * 192, 192, 1)
    args = list(real)
    for i in (1, 4, 7, 10, 11, 16, 17, 22, 23):
        a = list(args)
        a[i] = args[i].clone().requires_grad_(True)
        with pytest.raises(RuntimeError):
            OPS.lsq_attention_prefill_w8_q8_q(*a)
    assert not OPS.lsq_attention_prefill_w8_q8_q(*args).requires_grad


def test_the_references_of_the_gpu_tests_are_not_degenerate():
    """the reference alone: more than 16 distinct output levels for every case with at least 16 keys in every row and at least 256
    outputs (`check_not_degenerate`), and, for the causal-offset-0 cases whose first rows see fewer keys, over the rows from 16 on"""
    import test_attn_prefill_w8_gpu as G
    for shape, causal, lengths in G.SHAPES:
        c = P.case(*shape, 0, causal=causal, lengths=lengths)
        C.check_not_degenerate(c)
        if shape[3] > 16:
            assert len(c.want[:, 16:].unique()) > 16, shape
    for c in (P.case(1, 1, 1, 16, 2048, 128, 1, causal=True), P.case(1, 1, 2, 32, 8192, 64, 3, unsigned=C.ALL_UNSIGNED, causal=100),
              P.case(1, 1, 1, 17, 2049, 32, 2, causal=True), P.case(1, 1, 2, 17, 1024, 64, 7, unsigned=P.SIGNED_PV, table="full", causal=True)):
        n = C.key_counts(c.shape[0], c.shape[3], c.shape[4], c.causal, None)
        assert min(min(r) for r in n) >= 16 and c.want.numel() >= 256
        C.check_not_degenerate(c)
