"""Decode attention on 8-bit levels against a grouped-query KV cache (include/lsq_hip_attn_decode_w8.h), everything that needs no GPU:
the library's exports against its header and `_abi.py`, its one kernel (scratch and the matrix-core instruction, from the code object),
the plan on both sides of every threshold, every refusal with its message, and the CPU path of the op -- the definition the GPU
tests compare against -- held to plain Python integers with float32 steps, to the existing `AttentionCoreW8Q` (G = 1 and on
`repeat_interleave`d k and v), to poisoned cache slots, to the edge lengths and to the prefill, with the module's `decode=` option,
the fake kernel and the Autograd kernel on top.
"""
import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import attn_decode_w8_cases as C
import attn_w8_cases as A
from helpers import demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_attn_decode_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_attn_decode_w8.so")
NAMES = sorted(["lsq_attn_decode_w8_abi_version", "lsq_attn_decode_w8_last_error", "lsq_attn_decode_w8", "lsq_attn_decode_w8_plan"])
LSQ_EINVAL = -1
OPS = torch.ops.torchlsq
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
NOTHING = dict(family="composition", grid=0, threads=0, rows=0, lds_row_stride=0, lds_bytes=0, lds_dynamic=False, store="elements")
STATE_KEYS = ["scores.output_scale", "scores.output_shift", "softmax.table", "softmax.output_scale", "softmax.output_shift",
              "context.output_scale", "context.output_shift"]


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    return [f.strip() for decl in body.split(";")
            for f in re.sub(r"^\s*(const void\*|int64_t|lsq_attn_w8_strides)", "", decl.strip()).split(",") if f.strip()]


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_attn_decode_w8\w*)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_ATTN_DECODE_W8) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_"))) == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_", "lsq_requant_", "lsq_resadd_",
                  "lsq_pool_", "lsq_dwconv_", "lsq_eltwise_", "lsq_norm_", "lsq_attn_", "lsq_bmm_", "lsq_softmax_", "lsq_rope_"):
        assert other not in und, other
    assert E.attn_decode_w8_library().lsq_attn_decode_w8_abi_version() == E.ATTN_DECODE_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_ATTN_DECODE_W8_ABI_VERSION (\d+)", raw).group(1) == "1"
    for name, cls, words in (("lsq_attn_decode_w8_geom", E.LsqAttnDecodeW8Geom, 24), ("lsq_attn_decode_w8_consts", E.LsqAttnDecodeW8Consts, 8)):
        assert _fields(text, name) == [f[0] for f in cls._fields_] and ctypes.sizeof(cls) == words * 8, name


def test_the_kernel(tmp_path):
    """one kernel: no scratch, no atomics, the int8 matrix-core instruction, packet loads of k and packet stores of y, LDS in use"""
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    assert len(every) == 1 and re.match(r"^(?:void )?lsq::attn_decode_w8_kernel\(", list(names.values())[0]), names
    (body, scratch), = every.values()
    ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
    assert scratch == 0, "the kernel uses %d bytes of scratch" % scratch
    assert ops.count("v_mfma_i32_16x16x64_i8") >= 8 and not any("atomic" in o for o in ops)
    assert ops.count("global_load_dwordx4") >= 8, "four sub-tiles of two k packets in flight"
    assert "global_store_dwordx4" in ops and "s_barrier" in ops and any(o.startswith("ds_read_b128") or o.startswith("ds_load_b128") for o in ops)


# ---------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------
def _ld(Tk):
    return 16 * (((Tk + 15) // 16) | 1)


def _expected(B, H, Hkv, Tq, Tk, D, store="packets"):
    lds = 16 * _ld(Tk) + 1024 + 160 * D
    return dict(family="decode", grid=B * Hkv, threads=256 if Tk <= 256 else 512, rows=H // Hkv * Tq, lds_row_stride=_ld(Tk), lds_bytes=lds,
                lds_dynamic=lds > 65536, store=store)


def test_plans_without_a_gpu():
    from torchlsq import extension as E
    P = E.attn_decode_w8_plan
    for shape in ((1, 1, 1, 1, 1, 16), (2, 8, 2, 1, 40, 32), (1, 16, 1, 1, 65, 64), (1, 6, 2, 5, 19, 32), (1, 8, 1, 2, 197, 128),
                  (32, 32, 8, 1, 2048, 128), (32, 32, 32, 1, 2048, 128), (32, 32, 8, 4, 2048, 128), (1, 32, 8, 1, 8192, 128)):
        pl = P(*shape)
        assert pl == _expected(*shape), shape
        assert pl["grid"] == shape[0] * shape[2] and pl["lds_bytes"] <= 163840 and pl["lds_dynamic"] == (pl["lds_bytes"] > 65536)
    # R = G Tq: 16 is served, 17 is not
    assert P(1, 16, 1, 1, 64, 64)["rows"] == 16 and P(1, 8, 1, 2, 64, 64)["rows"] == 16 and P(1, 4, 4, 16, 64, 64)["rows"] == 16
    assert P(1, 17, 1, 1, 64, 64) == NOTHING and P(1, 1, 1, 17, 64, 64) == NOTHING and P(1, 6, 2, 6, 64, 64) == NOTHING
    # Tk: up to 8192
    assert P(1, 16, 1, 1, 8192, 128) == _expected(1, 16, 1, 1, 8192, 128) and P(1, 16, 1, 1, 8193, 128) == NOTHING
    assert P(1, 16, 1, 1, 8192, 128)["lds_bytes"] == 16 * 8208 + 1024 + 20480 == 152832
    # D: 16 .. 128 in multiples of 16
    assert P(1, 2, 1, 1, 64, 16)["family"] == "decode" and P(1, 2, 1, 1, 64, 24) == NOTHING and P(1, 2, 1, 1, 64, 8) == NOTHING
    assert P(1, 2, 1, 1, 64, 128)["family"] == "decode" and P(1, 2, 1, 1, 64, 144) == NOTHING
    # one stride that is not a multiple of 16, per operand and per stride (a stride of 24 among them); y's only changes the store
    q_dense, kv_dense = (4 * 2 * 64, 2 * 64, 64), (2 * 40 * 64, 40 * 64, 64)
    for name, dense in (("q_strides", q_dense), ("k_strides", kv_dense), ("v_strides", kv_dense)):
        for i in range(3):
            for off in (8, 24):
                bad = tuple(s + (off if j == i else 0) for j, s in enumerate(dense))
                assert P(2, 4, 2, 2, 40, 64, **{name: bad}) == NOTHING, (name, i, off)
        assert P(2, 4, 2, 2, 40, 64, **{name: tuple(s + 16 for s in dense)})["family"] == "decode"
    assert P(1, 2, 1, 1, 40, 16, k_strides=(0, 0, 24)) == NOTHING
    assert P(2, 4, 2, 2, 40, 64, qkv_aligned=False) == NOTHING
    assert P(2, 4, 2, 2, 40, 64, y_aligned=False) == _expected(2, 4, 2, 2, 40, 64, "elements")
    assert P(2, 4, 2, 2, 40, 64, y_strides=(2 * 4 * 64 + 8, 64, 256)) == _expected(2, 4, 2, 2, 40, 64, "elements")
    # the LDS row stride: 16 n with n odd; the bytes, where they pass 64 KB, and the threads on both sides of Tk = 256
    assert [P(1, 1, 1, 1, T, 64)["lds_row_stride"] for T in (1, 16, 17, 32, 33, 197, 8176, 8177, 8192)] == [16, 16, 48, 48, 48, 208, 8176, 8208, 8208]
    lo, hi = P(1, 1, 1, 1, 2736, 128), P(1, 1, 1, 1, 2737, 128)        # 16 * 2736 + 1024 + 20480 = 65280; 16 * 2768 + 21504 = 65792
    assert (lo["lds_bytes"], lo["lds_dynamic"], hi["lds_bytes"], hi["lds_dynamic"]) == (65280, False, 65792, True)
    assert (P(1, 1, 1, 1, 256, 64)["threads"], P(1, 1, 1, 1, 257, 64)["threads"]) == (256, 512)
    assert max(P(1, 1, 1, 1, T, D)["lds_bytes"] for T in (1, 197, 2048, 8192) for D in (16, 64, 128)) <= 163840
    # neither the dtypes nor the mask move the plan
    assert P(2, 6, 3, 1, 19, 32, q_dtype=I8, k_dtype=U8, v_dtype=I8, causal=True, causal_offset=18, has_lengths=False) == _expected(2, 6, 3, 1, 19, 32)


def test_plan_refusals_without_a_gpu():
    from torchlsq import extension as E
    lib = E.attn_decode_w8_library()
    err = lib.lsq_attn_decode_w8_last_error
    out = (ctypes.c_int32 * 8)()
    S = E.LsqAttnW8Strides

    def G(B=1, H=2, Hkv=2, Tq=8, Tk=8, D=16, dt=(0, 0, 0), causal=0, off=0, lens=0, q=None, k=None, v=None, y=None):
        d = S(H * 8 * 16, 8 * 16, 16)
        return E.LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, *dt, causal, off, lens, q or d, k or d, v or d, y or d)

    def plan(g):
        return lib.lsq_attn_decode_w8_plan(ctypes.byref(g), 1, 1, ctypes.byref(out))

    assert plan(G()) == 0 and out[0] == 1
    assert lib.lsq_attn_decode_w8_plan(None, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"NULL geometry" in err()
    assert lib.lsq_attn_decode_w8_plan(ctypes.byref(G()), 1, 1, None) == LSQ_EINVAL and b"NULL output" in err()
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
    assert plan(G(Tq=(1 << 20) + 1)) == LSQ_EINVAL and b"2^20" in err()
    assert plan(G(B=1 << 11, H=1 << 10, Hkv=1 << 10)) == LSQ_EINVAL and b"2^20" in err()
    assert plan(G(k=S(256, 128, 15))) == LSQ_EINVAL and b"k's row stride 15 is smaller" in err()
    assert plan(G(v=S(-16, 128, 16))) == LSQ_EINVAL and b"must not be negative" in err()
    assert plan(G(y=S(256, 64, 16))) == LSQ_EINVAL and b"overlap each other" in err()


def test_entry_refusals_without_a_gpu():
    """everything is checked before anything is enqueued: none of these calls reaches the runtime (the pointers are host memory)"""
    from torchlsq import extension as E
    lib = E.attn_decode_w8_library()
    err = lib.lsq_attn_decode_w8_last_error
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
        return lib.lsq_attn_decode_w8(None if no_geom else ctypes.byref(g), None if c is None else ctypes.byref(c),
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
    assert call(sides=[ok, ok, E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), 0, 255, 0, 255, 2)]) == LSQ_EINVAL and b"one mid_dtype" in err()
    assert call(sides=[E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), 0, 255, 0, 255, 1)] * 3) == LSQ_EINVAL and b"mid_dtype must be" in err()
    assert call(sides=[ok, E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), -1, 255, 0, 255, 0), ok]) == LSQ_EINVAL and b"must lie within" in err()
    assert call(table=None) == LSQ_EINVAL and b"NULL buffer" in err()
    assert call(table=tab.data_ptr() + 2) == LSQ_EINVAL and b"table must be element-aligned" in err()
    assert call(y=None) == LSQ_EINVAL and b"NULL buffer" in err()
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
    assert call(ptrs=(base + 1, base + nq, base + nq + nk)) == LSQ_EINVAL and b"not served by the decode kernel" in err()
    d24q, d24k = S(H * T * 24, T * 24, 24), S(Hkv * T * 24, T * 24, 24)
    assert call(g=geom(D=24, q=d24q, k=d24k, v=d24k, y=d24q), ptrs=(base, base + 2 * nq, base + 4 * nq)) == LSQ_EINVAL and b"compose lsq_hip_attn_w8.h" in err()
    assert call(g=geom(H=2, Hkv=1, Tq=9, q=S(2 * 9 * D, 9 * D, D), y=S(2 * 9 * D, 9 * D, D))) == LSQ_EINVAL and b"G Tq <= 16" in err()
    assert bool((ybuf == 0).all())


# ---------------------------------------------------------------------------------------------------
# the definition: plain integers and float32 steps
# ---------------------------------------------------------------------------------------------------
def _round_mid(x, mid):
    return torch.from_numpy(np.asarray(x, dtype=np.float32).reshape(-1)).to(mid)


def _level(u, side):
    return int(OPS.lsq_levels_per_tensor(u, *side, 0).view(I8)[0]) & 0xff


@pytest.mark.parametrize("dtypes,unsigned", C.COMBOS + ((C.ALL_U8, C.ALL_UNSIGNED),), ids=str)
def test_definition_against_plain_python_integers(dtypes, unsigned):
    """B 2, Hkv 2, G 2, Tq 2, Tk 5, D 4: every byte of the chain from Python integers, numpy float32 multiplies one at a time, the
    rounding to mid and the existing levels op; keys at or beyond n are not touched"""
    from torchlsq.functional import _act_constants
    B, Hkv, G, Tq, Tk, D = 2, 2, 2, 2, 5, 4
    c = C.case(B, Hkv, G, Tq, Tk, D, 11, dtypes, unsigned, BF16, (3, 140, 250), None, 1, (4, 0))
    n = C.key_counts(B, Tq, Tk, 1, [4, 0])
    assert n == [[2, 3], [0, 0]]
    f32 = np.float32
    sq, sk, sv = (f32(float(x.scale)) for x in (c.q, c.k, c.v))
    zq, zk, zv = (int(x.zero_point) for x in (c.q, c.k, c.v))
    p_s, p_z = _act_constants(c.sides[1][0], c.sides[1][1], c.sides[1][4], c.sides[1][5])
    sp, zp = f32(float(p_s)), int(p_z)
    tab = c.table.tolist()
    s_signed, p_signed = c.sides[0][3] <= 127 and c.sides[0][5] <= 127, c.sides[1][3] <= 127 and c.sides[1][5] <= 127
    ql, kl, vl = c.q.levels.tolist(), c.k.levels.tolist(), c.v.levels.tolist()
    want = torch.empty((B, Tq, Hkv * G * D), dtype=torch.int64)
    for b in range(B):
        for h in range(Hkv * G):
            for t in range(Tq):
                hk, cnt = h // G, n[b][t]
                sb = []
                for j in range(cnt):
                    I = sum((ql[b][h][t][d] - zq) * (kl[b][hk][j][d] - zk) for d in range(D))
                    byte = _level(_round_mid((sk * f32(I)) * sq, BF16), c.sides[0])
                    sb.append(byte - 256 if s_signed and byte > 127 else byte)
                ps = []
                if cnt:
                    m = max(sb)
                    E = [tab[m - x] for x in sb]
                    r = f32(1.0) / f32(sum(E))
                    for e in E:
                        byte = _level(_round_mid(f32(e) * r, BF16), c.sides[1])
                        ps.append(byte - 256 if p_signed and byte > 127 else byte)
                for d in range(D):
                    I = sum((ps[j] - zp) * (vl[b][hk][j][d] - zv) for j in range(cnt))
                    want[b, t, h * D + d] = _level(_round_mid((sv * f32(I)) * sp, BF16), c.sides[2])
    assert torch.equal(c.want.view(U8).to(torch.int64), want)
    zero = _level(torch.zeros(1, dtype=BF16), c.sides[2])
    assert bool((c.want.view(U8)[1] == zero).all()), "n = 0: the context quantizer's level of 0.0"


# ---------------------------------------------------------------------------------------------------
# against the existing module
# ---------------------------------------------------------------------------------------------------
def _core(D, **kw):
    from torchlsq.quantized import AttentionCoreW8Q
    span = 6.0 * A.QKV_S * A.QKV_S * 74 * 74 * D ** 0.5
    return AttentionCoreW8Q(A.trained(-span, span), A.trained(0.0, 1.0), A.trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16, **kw)


def _sides(core):
    return core.scores._out("output"), core.softmax._out("output"), core.context._out("output")


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("causal,lengths", [(True, None), (True, (19, 7)), (False, (12, 19)), (2, (0, 33))], ids=str)
def test_op_equals_the_existing_core_on_expanded_k_and_v(G, causal, lengths):
    """q [2, 3 G, 5, 32] against 19 keys of 3 kv heads: G = 1 is the existing masked core as it is, G = 2 and 4 the core on
    `repeat_interleave`d k and v (the probabilities quantizer has shift 0: its level of 0.0 is its z_p)"""
    from torchlsq.functional import lsq_attention_decode_w8_q
    B, Hkv, Tq, Tk, D = 2, 3, 5, 19, 32
    core = _core(D, causal=causal)
    q, k, v = C.inputs(B, Hkv, G, Tq, Tk, D, 20 + G)
    lens = C.lens_tensor(lengths)
    want = core(q, C.expanded(k, G), C.expanded(v, G), key_lengths=lens)
    got = lsq_attention_decode_w8_q(q, k, v, core.softmax.table, *_sides(core), BF16, causal=causal, key_lengths=lens)
    assert got.levels.shape == (B, Tq, Hkv * G * D) and got.levels.dtype == U8 and len(want.levels.unique()) > 16
    assert torch.equal(got.levels, want.levels) and torch.equal(got.scale, want.scale) and torch.equal(got.zero_point, want.zero_point)
    assert (got.quant_min, got.quant_max, got.type_min, got.type_max) == (want.quant_min, want.quant_max, want.type_min, want.type_max)
    dec = _core(D, causal=causal, decode=True)
    assert torch.equal(dec(q, k, v, key_lengths=lens).levels, want.levels)
    assert torch.equal(OPS.lsq_attention_decode_w8_q8_q(q.levels, q.scale, q.zero_point, k.levels, k.scale, k.zero_point, v.levels, v.scale,
                                                        v.zero_point, core.softmax.table, *_sides(core)[0], *_sides(core)[1], *_sides(core)[2],
                                                        BF16, causal is not False, {True: Tk - Tq, False: 0}.get(causal, causal), lens),
                       want.levels)


def test_unmasked_decode_is_the_unmasked_core():
    q, k, v = C.inputs(2, 3, 1, 19, 19, 32, 30)
    assert torch.equal(_core(32, decode=True)(q, k, v).levels, _core(32)(q, k, v).levels)


# ---------------------------------------------------------------------------------------------------
# poisoned slots, edge lengths
# ---------------------------------------------------------------------------------------------------
def _quant_min_5_sides(core):
    """the probabilities quantizer with quant_min = 5: its level of 0.0 is 5 and its zero point as an operand is 0"""
    from torchlsq.functional import _act_constants
    s, p, o = _sides(core)
    p5 = (p[0], p[1], 5) + tuple(p[3:])
    assert int(_act_constants(p5[0], p5[1], p5[4], p5[5])[1]) == 0
    assert int(OPS.lsq_levels_per_tensor(torch.zeros(1, dtype=BF16), *p5, 0).view(I8)[0]) == 5
    return s, p5, o


@pytest.mark.parametrize("quant_min_5", [False, True])
def test_slots_beyond_the_key_count_never_matter(quant_min_5):
    from torchlsq.functional import lsq_attention_decode_w8_q, lsq_bmm_w8_q, lsq_masked_softmax_w8_q
    B, Hkv, G, Tq, Tk, D = 2, 2, 2, 1, 40, 32
    core = _core(D, causal=True)
    sides = _quant_min_5_sides(core) if quant_min_5 else _sides(core)
    c = C.Case()
    c.shape, c.G, c.mid, c.causal, c.lengths = (B, Hkv * G, Hkv, Tq, Tk, D), G, BF16, True, C.lens_tensor((40, 13))
    c.q, c.k, c.v = C.inputs(B, Hkv, G, Tq, Tk, D, 31)
    c.table, c.sides = core.softmax.table, sides
    C.finish(c)
    assert len(c.want.unique()) > 16
    results = []
    for fill in (0x00, 0xFF):
        k, v = C.poisoned(c, fill)
        assert bool((k.levels[1, :, 13:] == fill).all()) and torch.equal(k.levels[0], c.k.levels[0])
        results.append(C.definition(c, k=k, v=v))
    assert torch.equal(results[0], c.want) and torch.equal(results[1], c.want)
    # the three launches of the parent route on the same poisoned slots: equal with shift 0 and quant_min 0, and dependent on the
    # poison where the level of 0.0 (5) is not z_p (0)
    parent = []
    for fill in (0x00, 0xFF):
        k, v = (C.expanded(x, G) for x in C.poisoned(c, fill))
        s = lsq_bmm_w8_q(c.q, k, True, *sides[0], BF16)
        p = lsq_masked_softmax_w8_q(s, c.table, *sides[1], BF16, causal=True, key_lengths=c.lengths)
        y = lsq_bmm_w8_q(p, v, False, *sides[2], BF16).levels
        parent.append(y.permute(0, 2, 1, 3).reshape(B, Tq, Hkv * G * D))
    if quant_min_5:
        assert not torch.equal(parent[0][1], parent[1][1]), "the parent route should depend on the unwritten slots here"
        assert torch.equal(parent[0][0], c.want[0]) and torch.equal(parent[1][0], c.want[0])      # (batch 0 has no masked key)
    else:
        assert torch.equal(parent[0], c.want) and torch.equal(parent[1], c.want)


def test_edge_lengths():
    """key_lengths {-3, 0, 1, Tk, Tk + 5}: clamped on both sides; an n = 0 row is the context quantizer's level of 0.0"""
    Tk = 19
    c = C.case(5, 2, 2, 1, Tk, 32, 12, C.ALL_U8, C.ALL_UNSIGNED, BF16, (A.QKV_Z,) * 3, None, True, (-3, 0, 1, Tk, Tk + 5))
    zero = int(OPS.lsq_levels_per_tensor(torch.zeros(1, dtype=BF16), *c.sides[2], 0).view(U8)[0])
    assert bool((c.want[0] == zero).all()) and bool((c.want[1] == zero).all()) and zero not in (0, 255)
    full = C.case(5, 2, 2, 1, Tk, 32, 12, C.ALL_U8, C.ALL_UNSIGNED, BF16, (A.QKV_Z,) * 3, None, True, None)
    assert torch.equal(c.want[3], full.want[3]) and torch.equal(c.want[4], full.want[4]) and not torch.equal(c.want[2], full.want[2])
    # one key: the op on the first slot of the same k and v alone
    one = C.Case()
    one.table, one.sides, one.mid, one.causal, one.lengths = c.table, c.sides, c.mid, True, None
    one.q, one.k, one.v = c.q, C.with_levels(c.k, c.k.levels[:, :, :1]), C.with_levels(c.v, c.v.levels[:, :, :1])
    assert torch.equal(c.want[2], C.definition(one)[2])


# ---------------------------------------------------------------------------------------------------
# decode equals prefill
# ---------------------------------------------------------------------------------------------------
def test_gqa_decode_equals_prefill():
    from torchlsq.quantized import KVCacheW8
    case = C.gqa_decode_case()
    B, H, Hkv, T, D = case["B"], case["H"], case["Hkv"], case["T"], case["D"]
    assert tuple(case["prefill"].shape) == (B, T, H * D) and len(case["prefill"].unique()) > 32
    core = copy.deepcopy(case["core"])
    core.decode = True
    cache = KVCacheW8(B, Hkv, case["Tmax"], D)
    for t in range(T):
        ctx = C.gqa_decode_step(case, case["rot"], core, cache, t)
        assert tuple(ctx.shape) == (B, 1, H * D) and cache.lengths.tolist() == [t + 1] * B
        assert torch.equal(ctx[:, 0], case["prefill"][:, t]), "decode step %d is not the prefill's row" % t
    assert tuple(cache.k.shape) == (B, Hkv, case["Tmax"], D) and not bool(cache.k[:, :, T:].any())
    # decode=False refuses the cache's two kv heads against four query heads, as before
    cache.reset() if hasattr(cache, "reset") else cache.lengths.zero_()
    with pytest.raises(AssertionError, match=r"needs q \[B, H, Tq, D\] and k, v \[B, H, Tk, D\]"):
        C.gqa_decode_step(case, case["rot"], case["core"], cache, 0)


# ---------------------------------------------------------------------------------------------------
# the module, the op
# ---------------------------------------------------------------------------------------------------
def test_module_decode_option(monkeypatch):
    import torchlsq.quantized.modules.attn_w8 as W
    from torchlsq.quantized import AttentionCoreW8Q
    calls = []

    def spy(name):
        real = getattr(W, name)

        def f(*a, **kw):
            calls.append(name)
            return real(*a, **kw)
        monkeypatch.setattr(W, name, f)
    for name in ("lsq_softmax_w8_q", "lsq_masked_softmax_w8_q", "lsq_attention_w8_q", "lsq_attention_decode_w8_q"):
        spy(name)
    q, k, v = C.inputs(2, 3, 1, 19, 19, 32, 40)
    lens = C.lens_tensor((19, 7))
    plain, dec = _core(32, causal=True), _core(32, causal=True, decode=True)
    assert plain.decode is False and dec.decode is True and AttentionCoreW8Q.decode is False
    assert list(plain.state_dict()) == list(dec.state_dict()) == STATE_KEYS
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), dec.state_dict().values()))
    want = plain(q, k, v, key_lengths=lens)
    assert calls == ["lsq_masked_softmax_w8_q"]
    del calls[:]
    assert torch.equal(dec(q, k, v, key_lengths=lens).levels, want.levels) and calls[0] == "lsq_attention_decode_w8_q"
    del calls[:]
    # decode=False: unmasked and fused calls go where they went, and Hkv != H is refused
    un = _core(32)
    un(q, k, v)
    assert calls == ["lsq_softmax_w8_q"]
    del calls[:]
    _core(32, fused=True)(q, k, v)
    assert calls[0] == "lsq_attention_w8_q" and "lsq_attention_decode_w8_q" not in calls
    q6 = C.inputs(2, 3, 2, 19, 19, 32, 41)[0]
    with pytest.raises(AssertionError, match="masked\\) needs q"):
        plain(q6, k, v, key_lengths=lens)
    with pytest.raises(AssertionError, match="one shape"):
        un(q6, k, v)
    assert dec(q6, k, v, key_lengths=lens).levels.shape == (2, 19, 6 * 32)
    # the attribute is not a buffer; a module pickled before it existed reads the class default
    old = copy.deepcopy(plain)
    del old.__dict__["decode"]
    assert old.decode is False and torch.equal(old(q, k, v, key_lengths=lens).levels, want.levels)
    assert "decode=True" in repr(dec) and "lsq_attention_decode_w8_q" in repr(dec) and "causal=True" in repr(dec)
    assert "decode" not in repr(plain) and "three launches" in repr(plain)
    dec.load_state_dict(plain.state_dict())


def test_functional_form_and_argument_validation():
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, _act_constants, lsq_attention_decode_w8_q
    c = C.case(2, 3, 2, 1, 19, 32, 13, C.COMBOS[0][0], C.COMBOS[0][1], BF16, (A.QKV_Z,) * 3, None, True, (19, 6))
    y = lsq_attention_decode_w8_q(c.q, c.k, c.v, c.table, *c.sides, c.mid, causal=True, key_lengths=c.lengths)
    o = c.sides[2]
    s, z = _act_constants(o[0], o[1], o[4], o[5])
    assert isinstance(y, LevelsTensor) and torch.equal(y.levels, c.want) and torch.equal(y.scale, s) and torch.equal(y.zero_point, z)
    with pytest.raises(AssertionError, match="scale, shift, quant_min"):
        lsq_attention_decode_w8_q(c.q, c.k, c.v, c.table, c.sides[0], None, c.sides[2], c.mid)
    with pytest.raises(AssertionError, match="offset >= 0"):
        lsq_attention_decode_w8_q(c.q, c.k, c.v, c.table, *c.sides, c.mid, causal=-1)
    with pytest.raises(AssertionError, match="needs Tk >= Tq"):
        lsq_attention_decode_w8_q(C.with_levels(c.q, c.q.levels.expand(2, 6, 20, 32)), c.k, c.v, c.table, *c.sides, c.mid, causal=True)
    args = list(C.flat_args(c, "cpu"))
    assert torch.equal(OPS.lsq_attention_decode_w8_q8_q(*args), c.want)

    def bad(i, v, match):
        a = list(args)
        a[i] = v
        with pytest.raises(RuntimeError, match=match):
            OPS.lsq_attention_decode_w8_q8_q(*a)

    bad(0, args[0].to(torch.int16), "must be uint8")
    bad(3, args[3][:, :2], r"q must be \[B, H, Tq, D\]")                  # k and v differ
    bad(0, args[0][..., :16], r"q must be \[B, H, Tq, D\]")
    bad(0, args[0][:, :5], "H = 5 query heads are not a multiple of Hkv = 3")
    bad(1, torch.ones(2), "scale must be one float32")
    bad(5, torch.zeros(1), "zero point one int32")
    bad(9, args[9].to(torch.int64), "table must be a dense int32")
    bad(12, -129, "must lie within")
    bad(16, torch.ones(2), "out_scale and out_shift must be float32 tensors of one value")
    bad(28, torch.float64, "must be float32, bfloat16 or float16")
    bad(30, -1, "causal_offset = -1 must be at least 0")
    bad(31, torch.zeros(3, dtype=torch.int32), r"key_lengths must be a dense int32 tensor of \[2\]")
    bad(31, torch.zeros(2, dtype=torch.int64), r"key_lengths must be a dense int32 tensor of \[2\]")
    out = torch.empty(2, 6, 1, 32, dtype=c.want.dtype)
    assert E.attn_decode_w8_q(*args, out=out) is out and torch.equal(out.permute(0, 2, 1, 3).reshape(2, 1, 192), c.want)
    with pytest.raises(RuntimeError, match="`out` must be a"):
        E.attn_decode_w8_q(*args, out=out.view(U8 if out.dtype == I8 else I8))
    a = list(args)
    a[0] = args[0][:, :, :0]
    assert OPS.lsq_attention_decode_w8_q8_q(*a).shape == (2, 0, 192)


def test_fake_kernel_and_grad_refusal():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for unsigned, dtype in (((True, False, True), U8), ((True, True, False), I8)):
        c = C.case(2, 3, 2, 1, 19, 32, 14, C.ALL_U8, unsigned, BF16, (A.QKV_Z,) * 3, None, True, (19, 6))
        assert c.want.dtype == dtype
        real = C.flat_args(c, "cpu")
        with FakeTensorMode() as mode:
            args = tuple(mode.from_tensor(t) if isinstance(t, torch.Tensor) else t for t in real)
            y = OPS.lsq_attention_decode_w8_q8_q(*args)
            assert y.shape == (2, 1, 192) and y.dtype == dtype and y.stride() == (192, 192, 1)
    args = list(real)
    for i in (1, 4, 7, 10, 11, 16, 17, 22, 23):
        a = list(args)
        a[i] = args[i].clone().requires_grad_(True)
        with pytest.raises(RuntimeError):
            OPS.lsq_attention_decode_w8_q8_q(*a)
    assert not OPS.lsq_attention_decode_w8_q8_q(*args).requires_grad


def test_composition_shapes_on_the_cpu():
    """R 17, D 24 and Tk beyond the kernel's: legal, the plan says "composition", the op serves them"""
    for shape in ((1, 1, 17, 1, 19, 32), (1, 2, 2, 1, 19, 24)):
        c = C.case(*shape, 15, C.ALL_U8, C.ALL_UNSIGNED, BF16, (A.QKV_Z,) * 3, None, True, None)
        assert C.plan_of(c)["family"] == "composition" and len(c.want.unique()) > 16
        core_sides = c.sides
        from torchlsq.functional import lsq_bmm_w8_q, lsq_masked_softmax_w8_q
        G = c.G
        s = lsq_bmm_w8_q(c.q, C.expanded(c.k, G), True, *core_sides[0], BF16)
        p = lsq_masked_softmax_w8_q(s, c.table, *core_sides[1], BF16, causal=True)
        y = lsq_bmm_w8_q(p, C.expanded(c.v, G), False, *core_sides[2], BF16).levels
        assert torch.equal(c.want, y.permute(0, 2, 1, 3).reshape(c.want.shape))
