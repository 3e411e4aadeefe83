"""The attention core on 8-bit levels (include/lsq_hip_attn_w8.h), everything that needs no GPU: the library's exports against its
header and `_abi.py`, its kernel set and their resources, both plans on both sides of every threshold, every refusal, and the CPU
paths of the ops -- the definitions the GPU tests compare against -- held to plain Python integers, to the existing W8A8 linear, to a
numpy restatement step by step and to float64 within the derived bound, with the modules and the fake kernels on top.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import attn_w8_cases as A
from helpers import demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_attn_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_attn_w8.so")
NAMES = sorted(["lsq_attn_w8_abi_version", "lsq_attn_w8_last_error", "lsq_bmm_w8", "lsq_bmm_w8_plan", "lsq_softmax_w8", "lsq_softmax_w8_plan"])
LSQ_EINVAL = -1
OPS = torch.ops.torchlsq
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
one = A.one


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    return [f.strip() for decl in body.split(";")
            for f in re.sub(r"^\s*(const void\*|int64_t|float|lsq_attn_w8_strides)", "", decl.strip()).split(",") if f.strip()]


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_(?:attn|bmm|softmax)_w8\w*)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_ATTN_W8) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_", "lsq_requant_", "lsq_resadd_",
                  "lsq_pool_", "lsq_dwconv_", "lsq_eltwise_", "lsq_norm_", "lsq_attn_", "lsq_bmm_", "lsq_softmax_"):
        assert other not in und, other
    assert E.attn_w8_library().lsq_attn_w8_abi_version() == E.ATTN_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_ATTN_W8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    for name, cls, words in (("lsq_attn_w8_strides", E.LsqAttnW8Strides, 3), ("lsq_bmm_w8_geom", E.LsqBmmW8Geom, 17),
                             ("lsq_attn_w8_out", E.LsqAttnW8Out, 7), ("lsq_bmm_w8_consts", E.LsqBmmW8Consts, 4),
                             ("lsq_softmax_w8_geom", E.LsqSoftmaxW8Geom, 5)):
        assert _fields(text, name) == [f[0] for f in cls._fields_] and ctypes.sizeof(cls) == words * 8, name


def test_kernels(tmp_path):
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    short = {}
    for sym, dm in names.items():
        m = re.match(r"^(?:void )?lsq::(bmm_w8_mfma|bmm_w8_generic|softmax_w8_packets|softmax_w8_generic)_kernel(?:<([^>]*)>)?\(", dm)
        assert m, "not a kernel of this library: %s" % dm
        args = re.sub(r"\((?:int|bool)\)", "", m.group(2) or "").replace("true", "1").replace("false", "0")
        short[sym] = m.group(1) + "".join("_" + n for n in re.findall(r"\d+", args))
    want = ["bmm_w8_generic", "bmm_w8_mfma_0", "bmm_w8_mfma_1", "softmax_w8_generic"] + \
           ["softmax_w8_packets_%d_1" % L for L in (4, 8, 16, 32, 64)] + ["softmax_w8_packets_64_%d" % P for P in (2, 4, 8)]
    assert sorted(short.values()) == sorted(want)
    for sym, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0, "%s uses %d bytes of scratch" % (sym, scratch)
        if short[sym].startswith("bmm_w8_mfma"):
            # per K step: four products, four column sums and one row sum on the matrix core; NN transposes with v_perm_b32
            assert ops.count("v_mfma_i32_16x16x64_i8") == 9 and "global_store_dwordx4" in ops, sym
            assert (ops.count("v_perm_b32") == 8) == short[sym].endswith("_1"), sym
        elif short[sym].startswith("softmax_w8_packets"):
            P = int(short[sym].split("_")[-1])
            assert ops.count("global_load_dwordx4") >= P and "global_store_dwordx4" in ops and ops.count("s_barrier") == 1, sym
            assert "v_pk_max_u16" in ops and "v_exp_f32_e32" not in ops, sym
        else:
            assert "v_mfma_i32_16x16x64_i8" not in ops, sym


# ---------------------------------------------------------------------------------------------------
# the plans
# ---------------------------------------------------------------------------------------------------
def test_bmm_plans_without_a_gpu():
    from torchlsq import extension as E
    P = E.attn_w8_plan_bmm
    # ViT-B scores and context: the matrix cores, 64 x 64 tiles, one batch a workgroup
    assert P((32, 12), 197, 197, 64, True) == dict(family="mfma", form="nt", grid=384 * 16, block=256, tile_rows=64, tile_cols=64,
                                                   lds_bytes=5120, store="elements")
    pad = (12 * 197 * 208, 197 * 208, 208)
    assert P((32, 12), 197, 197, 64, True, y_strides=pad)["store"] == "packets"
    assert P((32, 12), 197, 64, 197, False, a_strides=pad) == dict(family="mfma", form="nn", grid=384 * 4, block=256, tile_rows=64, tile_cols=64,
                                                                   lds_bytes=5120, store="packets")
    # the family: every stride of A and B a multiple of 16 and aligned bases; K (NT), N (NN) need not be one
    assert P(2, 5, 7, 197, True)["family"] == "generic"                                     # dense rows of 197
    assert P(2, 5, 7, 197, True, a_strides=(5 * 208, 5 * 208, 208), b_strides=(7 * 208, 7 * 208, 208))["family"] == "mfma"
    assert P(2, 5, 7, 197, True, a_strides=(5 * 208, 5 * 208, 208))["family"] == "generic"  # B alone is dense
    assert P(2, 5, 7, 197, True, a_strides=(5 * 208 + 8, 5 * 208 + 8, 208), b_strides=(7 * 208, 7 * 208, 208))["family"] == "generic"
    assert P(1, 16, 16, 272, True)["family"] == "mfma" and P(1, 16, 16, 272, True, aligned=False)["family"] == "generic"
    assert P(1, 5, 72, 16, False)["family"] == "generic" and P(1, 5, 80, 16, False)["family"] == "mfma"    # NN: N is B's row
    assert P(1, 5, 72, 16, False, b_strides=(16 * 80, 16 * 80, 80))["family"] == "mfma"
    # the grid: ceil(M / 64) ceil(N / 64) workgroups a batch; generic: a thread per output
    for M, N, tiles in ((64, 64, 1), (65, 64, 2), (64, 65, 2), (129, 129, 9), (1, 1, 1)):
        assert P(3, M, N, 16, True)["grid"] == 3 * tiles, (M, N)
    assert P(3, 5, 7, 3, True) == dict(family="generic", form="nt", grid=1, block=256, tile_rows=0, tile_cols=0, lds_bytes=0, store="elements")
    assert P(3, 5, 7, 3, True)["grid"] == 1 and P(1, 16, 17, 5, True)["grid"] == 2
    # the store: packets for levels out into an aligned y whose strides are multiples of 16
    ys = (64 * 80, 64 * 80, 80)
    assert P(1, 64, 80, 16, True)["store"] == "packets" and P(1, 64, 80, 16, True, levels_out=False)["store"] == "elements"
    assert P(1, 64, 80, 16, True, y_aligned=False)["store"] == "elements" and P(1, 64, 72, 16, True)["store"] == "elements"
    assert P(1, 64, 72, 16, True, y_strides=ys)["store"] == "packets"
    assert P(2, 64, 72, 16, True, y_strides=(0, 64 * 80 + 8, 80))["store"] == "elements"


def _expected_softmax_plan(R, C, ldx, ldy, aligned):
    if not (aligned and ldx % 16 == 0 and ldy % 16 == 0 and C <= 8192):
        return dict(family="generic", grid=-(-R // 4), block=256, lanes_per_row=64, packets_per_lane=0, rows_per_workgroup=4, lds_bytes=0)
    n = -(-C // 16)
    P = next(p for p in (1, 2, 4, 8) if -(-n // p) <= 64)
    L = next(l for l in (4, 8, 16, 32, 64) if l >= -(-n // P))
    G = 256 // L
    K = 4 if -(-R // (G * 4)) >= 512 else 1
    return dict(family="packets", grid=-(-R // (G * K)), block=256, lanes_per_row=L, packets_per_lane=P, rows_per_workgroup=G * K, lds_bytes=1024)


def test_softmax_plans_without_a_gpu():
    from torchlsq import extension as E
    P = E.attn_w8_plan_softmax
    for C in (1, 16, 17, 64, 65, 128, 129, 197, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 65536):
        ld = -(-C // 16) * 16
        for R in (1, 5, 100000):
            for aligned in (True, False):
                assert P(R, C, ld, ld, aligned) == _expected_softmax_plan(R, C, ld, ld, aligned), (R, C, aligned)
    # the family: aligned bases, ldx and ldy multiples of 16, C <= 8192 -- C itself need not be a multiple of 16
    assert P(5, 197, 208, 208)["family"] == "packets" and P(5, 197)["family"] == "generic"
    assert P(5, 197, 208, 197)["family"] == "generic" and P(5, 197, 197, 208)["family"] == "generic"
    assert P(2, 8192)["family"] == "packets" and P(2, 8208)["family"] == "generic"
    # (L, P): the fewest packets a lane that fit the row into a wave, then the smallest group that holds them
    want = {1: (4, 1), 64: (4, 1), 65: (8, 1), 128: (8, 1), 129: (16, 1), 197: (16, 1), 256: (16, 1), 257: (32, 1), 512: (32, 1), 513: (64, 1),
            1024: (64, 1), 1025: (64, 2), 2048: (64, 2), 2049: (64, 4), 4096: (64, 4), 4097: (64, 8), 8192: (64, 8)}
    for C, lp in want.items():
        ld = -(-C // 16) * 16
        pl = P(9, C, ld, ld)
        assert (pl["lanes_per_row"], pl["packets_per_lane"]) == lp, (C, pl)
    # rows per workgroup: (256 / L) groups of 4 rows from 512 workgroups on, else of one
    for C, G in ((16, 64), (197, 16), (1024, 4)):
        ld = -(-C // 16) * 16
        edge = 511 * G * 4 + 1
        hi, lo = P(edge, C, ld, ld), P(edge - 1, C, ld, ld)
        assert hi["rows_per_workgroup"] == 4 * G and hi["grid"] == 512 and lo["rows_per_workgroup"] == G and lo["grid"] == 511 * 4, (C, hi, lo)
    assert P(32 * 12 * 197, 197, 208, 208) == dict(family="packets", grid=1182, block=256, lanes_per_row=16, packets_per_lane=1,
                                                   rows_per_workgroup=64, lds_bytes=1024)


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def test_bmm_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.attn_w8_library()
    err = lib.lsq_attn_w8_last_error
    out = (ctypes.c_int32 * 8)()
    S = E.LsqAttnW8Strides

    def geom(B0=1, B1=2, M=4, N=5, K=16, form=1, ad=0, bd=1, a=None, b=None, y=None):
        rb, cb = (N, K) if form == 1 else (K, N)
        return E.LsqBmmW8Geom(B0, B1, M, N, K, form, ad, bd, S(*(a or (B1 * M * K, M * K, K))), S(*(b or (B1 * rb * cb, rb * cb, cb))),
                              S(*(y or (B1 * M * N, M * N, N))))

    def plan(g, outp=out):
        return lib.lsq_bmm_w8_plan(None if g is None else ctypes.byref(g), 1, 1, 1, None if outp is None else ctypes.byref(outp))
    assert plan(None) == LSQ_EINVAL and b"NULL geometry" in err()
    assert plan(geom(), None) == LSQ_EINVAL and b"NULL output" in err()
    assert plan(geom()) == 0
    assert plan(geom(form=2)) == LSQ_EINVAL and b"form must be" in err()
    assert plan(geom(ad=2)) == LSQ_EINVAL and b"a_dtype and b_dtype must be" in err()
    assert plan(geom(bd=-1)) == LSQ_EINVAL and b"a_dtype and b_dtype must be" in err()
    for bad in (dict(B0=0), dict(B1=0), dict(M=0), dict(N=0), dict(K=0), dict(M=-3)):
        assert plan(geom(**bad)) == LSQ_EINVAL and b"at least 1" in err(), bad
    assert plan(geom(K=65537)) == LSQ_EINVAL and b"at most 65536" in err()
    assert plan(geom(K=65536)) == 0
    big = 1 << 20
    for bad in (dict(M=big + 1), dict(N=big + 1), dict(B0=big, B1=2)):
        assert plan(geom(**bad)) == LSQ_EINVAL and b"2^20 at most" in err(), bad
    assert plan(geom(B0=1, B1=big, M=1, N=1)) == 0
    assert plan(geom(B0=1, B1=big, M=big, N=big, K=3, a=(0, 3, 3), b=(0, 3, 3))) == LSQ_EINVAL and b"workgroups are beyond 2^24 - 1" in err()
    # 256 threads a workgroup and at most 2^24 - 1 workgroups: the launch stays below 2^32 threads.  Matrix cores: a tile a workgroup
    assert plan(geom(B0=1, B1=(1 << 20) - 1, M=257, N=256, a=(0, 16, 16), b=(0, 16, 16))) == LSQ_EINVAL and b"20971500 workgroups are beyond" in err()
    assert plan(geom(B0=1, B1=(1 << 20) - 1, M=256, N=256, a=(0, 16, 16), b=(0, 16, 16))) == 0 and out[2] == ((1 << 20) - 1) * 16
    assert plan(geom(B0=1, B1=1, M=1 << 16, N=1 << 16, K=3, a=(0, 0, 3), b=(0, 0, 3))) == LSQ_EINVAL and b"16777216 workgroups are beyond" in err()
    assert plan(geom(B0=1, B1=1, M=1 << 16, N=(1 << 16) - 1, K=3, a=(0, 0, 3), b=(0, 0, 3))) == 0
    assert plan(geom(a=(64, 64, 15))) == LSQ_EINVAL and b"A's row stride 15 is smaller than its row of 16" in err()
    assert plan(geom(b=(80, 80, 15))) == LSQ_EINVAL and b"B's row stride 15 is smaller" in err()
    assert plan(geom(form=0, b=(80, 80, 4))) == LSQ_EINVAL and b"B's row stride 4 is smaller than its row of 5" in err()
    assert plan(geom(y=(20, 20, 4))) == LSQ_EINVAL and b"y's row stride 4 is smaller" in err()
    assert plan(geom(a=(-64, 64, 16))) == LSQ_EINVAL and b"A's batch strides (-64, 64) must not be negative" in err()
    assert plan(geom(a=(0, 0, 16))) == 0                                                    # an operand may repeat
    assert plan(geom(y=(0, 0, 5))) == LSQ_EINVAL and b"y's rows or batches overlap each other" in err()
    assert plan(geom(y=(40, 19, 5))) == LSQ_EINVAL and b"overlap each other" in err()
    assert plan(geom(B0=2, B1=3, M=4, N=8, y=(4 * 24, 8, 24))) == 0                         # the [B, H, T, D] view of [B, T, H D]
    assert plan(geom(B0=2, B1=3, M=4, N=8, y=(4 * 24, 7, 24))) == LSQ_EINVAL and b"overlap each other" in err()

    # the call: every refusal comes before anything is enqueued, so host memory will do for the pointers
    a, b, yy = torch.zeros(2 * 4 * 16, dtype=U8), torch.zeros(2 * 5 * 16, dtype=U8), torch.zeros(2 * 4 * 5 * 4 + 16, dtype=U8)
    s, z = torch.ones(4), torch.zeros(4, dtype=torch.int32)

    def consts(**kw):
        base = dict(s_a=s.data_ptr(), z_a=z.data_ptr(), s_b=s.data_ptr() + 4, z_b=z.data_ptr() + 4)
        base.update(kw)
        return E.LsqBmmW8Consts(*[base[f[0]] for f in E.LsqBmmW8Consts._fields_])

    def outq(**kw):
        base = dict(out_scale=s.data_ptr() + 8, out_shift=s.data_ptr() + 12, quant_min=0, quant_max=255, type_min=0, type_max=255,
                    mid_dtype=E.LSQ_F32)
        base.update(kw)
        return E.LsqAttnW8Out(*[base[f[0]] for f in E.LsqAttnW8Out._fields_])

    def call(g=None, c=None, o=None, ap=a.data_ptr(), bp=b.data_ptr(), yp=yy.data_ptr(), no=()):
        g, c, o = geom() if g is None else g, consts() if c is None else c, outq() if o is None else o
        return lib.lsq_bmm_w8(None if "g" in no else ctypes.byref(g), None if "c" in no else ctypes.byref(c),
                              None if "o" in no else ctypes.byref(o), ap, bp, yp, None)
    assert call(no="g") == LSQ_EINVAL and b"NULL geometry" in err()
    assert call(no="c") == LSQ_EINVAL and b"NULL constants" in err()
    assert call(no="o") == LSQ_EINVAL and b"NULL output description" in err()
    assert call(g=geom(K=0)) == LSQ_EINVAL and b"at least 1" in err()
    for name in ("s_a", "z_a", "s_b", "z_b"):
        assert call(c=consts(**{name: None})) == LSQ_EINVAL and b"NULL scale or zero point" in err(), name
        assert call(c=consts(**{name: s.data_ptr() + 2})) == LSQ_EINVAL and b"scales and zero points must be element-aligned" in err(), name
    assert call(o=outq(mid_dtype=E.LSQ_F64)) == LSQ_EINVAL and b"mid_dtype must be" in err()
    assert call(o=outq(out_scale=None)) == LSQ_EINVAL and b"they come together" in err()
    assert call(o=outq(out_shift=None)) == LSQ_EINVAL and b"they come together" in err()
    assert call(o=outq(out_scale=s.data_ptr() + 9)) == LSQ_EINVAL and b"out_scale and out_shift must be element-aligned" in err()
    for rng in (dict(quant_min=5, quant_max=4), dict(quant_min=-1), dict(type_min=-128, type_max=127), dict(quant_max=256, type_max=256)):
        assert call(o=outq(**rng)) == LSQ_EINVAL and b"must lie within 0..255 or within -128..127" in err(), rng
    for ptr in ("ap", "bp", "yp"):
        assert call(**{ptr: None}) == LSQ_EINVAL and b"NULL buffer" in err(), ptr
    assert call(o=outq(out_scale=None, out_shift=None), yp=yy.data_ptr() + 2) == LSQ_EINVAL and b"a floating y must be element-aligned" in err()
    assert call(yp=a.data_ptr() + 100) == LSQ_EINVAL and b"overlap A's" in err()
    assert call(yp=b.data_ptr()) == LSQ_EINVAL and b"overlap A's 128 or B's 160" in err()


def test_softmax_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.attn_w8_library()
    err = lib.lsq_attn_w8_last_error
    out = (ctypes.c_int32 * 8)()
    G = E.LsqSoftmaxW8Geom

    def plan(g, outp=out):
        return lib.lsq_softmax_w8_plan(None if g is None else ctypes.byref(g), 1, None if outp is None else ctypes.byref(outp))
    assert plan(None) == LSQ_EINVAL and b"NULL geometry" in err()
    assert plan(G(4, 16, 16, 16, 0), None) == LSQ_EINVAL and b"NULL output" in err()
    assert plan(G(4, 16, 16, 16, 2)) == LSQ_EINVAL and b"x_dtype must be" in err()
    for bad in ((0, 16), (4, 0), (-1, 16)):
        assert plan(G(*bad, 16, 16, 0)) == LSQ_EINVAL and b"at least 1" in err(), bad
    assert plan(G(4, 65537, 65537, 65537, 0)) == LSQ_EINVAL and b"at most 65536" in err()
    assert plan(G(4, 65536, 65536, 65536, 0)) == 0
    assert plan(G(1 << 29, 16, 16, 16, 0)) == LSQ_EINVAL and b"beyond 29 bits" in err()
    assert plan(G((1 << 29) - 1, 16, 16, 16, 0)) == 0 and out[1] == 1 << 21            # packets: 256 rows a workgroup
    # at most 2^24 - 1 workgroups of 256 threads (the launch stays below 2^32 threads): the generic family takes four rows each
    assert plan(G(4 * ((1 << 24) - 1), 16, 20, 16, 0)) == 0 and out[1] == (1 << 24) - 1
    assert plan(G(4 * ((1 << 24) - 1) + 1, 16, 20, 16, 0)) == LSQ_EINVAL and b"16777216 workgroups are beyond 2^24 - 1" in err()
    assert plan(G(4, 16, 15, 16, 0)) == LSQ_EINVAL and b"ldx = 15 and ldy = 16 must be at least C = 16" in err()
    assert plan(G(4, 16, 16, 15, 0)) == LSQ_EINVAL and b"must be at least C" in err()
    x, yy, tab = torch.zeros(4 * 16, dtype=U8), torch.zeros(4 * 16 * 4 + 16, dtype=U8), torch.zeros(260, dtype=torch.int32)
    s = torch.ones(4)

    def outq(**kw):
        base = dict(out_scale=s.data_ptr(), out_shift=s.data_ptr() + 4, quant_min=0, quant_max=255, type_min=0, type_max=255, mid_dtype=E.LSQ_F32)
        base.update(kw)
        return E.LsqAttnW8Out(*[base[f[0]] for f in E.LsqAttnW8Out._fields_])

    def call(g=(4, 16, 16, 16, 0), o=None, tp=tab.data_ptr(), xp=x.data_ptr(), yp=yy.data_ptr(), no=()):
        o = outq() if o is None else o
        return lib.lsq_softmax_w8(None if "g" in no else ctypes.byref(G(*g)), None if "o" in no else ctypes.byref(o), tp, xp, yp, None)
    assert call(no="g") == LSQ_EINVAL and b"NULL geometry" in err()
    assert call(no="o") == LSQ_EINVAL and b"NULL output description" in err()
    assert call(g=(4, 16, 8, 16, 0)) == LSQ_EINVAL and b"must be at least C" in err()
    assert call(o=outq(mid_dtype=7)) == LSQ_EINVAL and b"mid_dtype must be" in err()
    assert call(o=outq(out_shift=None)) == LSQ_EINVAL and b"they come together" in err()
    assert call(o=outq(quant_min=-1)) == LSQ_EINVAL and b"must lie within" in err()
    for ptr in ("tp", "xp", "yp"):
        assert call(**{ptr: None}) == LSQ_EINVAL and b"NULL buffer" in err(), ptr
    assert call(tp=tab.data_ptr() + 2) == LSQ_EINVAL and b"the table must be element-aligned" in err()
    assert call(o=outq(out_scale=None, out_shift=None), yp=yy.data_ptr() + 1) == LSQ_EINVAL and b"a floating y must be element-aligned" in err()
    assert call(yp=x.data_ptr() + 63) == LSQ_EINVAL and b"the softmax in place is not served" in err()
    assert call(yp=tab.data_ptr() + 1000) == LSQ_EINVAL and b"or the table" in err()


def test_op_argument_validation():
    a = A.bmm_operands(2, 4, 5, 16, True)
    q = A.fit_quantizer(torch.tensor([-1.0, 1.0]), True)
    with pytest.raises(RuntimeError, match="levels of a must be uint8"):
        OPS.lsq_bmm_w8_q8(a[0].float(), *a[1:], F32)
    with pytest.raises(RuntimeError, match="same 2 to 4 axes"):
        OPS.lsq_bmm_w8_q8(a[0][0], *a[1:], F32)
    with pytest.raises(RuntimeError, match="same batch axes"):
        OPS.lsq_bmm_w8_q8(a[0][:1], *a[1:], F32)
    with pytest.raises(RuntimeError, match=r"K = 16.*\[.., K, N\] with K = 5"):
        OPS.lsq_bmm_w8_q8(*a[:6], False, F32)
    with pytest.raises(RuntimeError, match="a's scale must be one float32 value"):
        OPS.lsq_bmm_w8_q8(a[0], a[1].double(), *a[2:], F32)
    with pytest.raises(RuntimeError, match="b's scale must be one float32 value"):
        OPS.lsq_bmm_w8_q8(*a[:5], a[5].long(), True, F32)
    with pytest.raises(RuntimeError, match="out_dtype must be float32, bfloat16 or float16"):
        OPS.lsq_bmm_w8_q8(*a, torch.float64)
    with pytest.raises(RuntimeError, match="mid_dtype must be float32"):
        OPS.lsq_bmm_w8_q8_q(*a, *q, torch.float64)
    with pytest.raises(RuntimeError, match="out_scale and out_shift must be float32 tensors of one value"):
        OPS.lsq_bmm_w8_q8_q(*a, torch.ones(2), *q[1:], F32)
    with pytest.raises(RuntimeError, match="at most 65536"):
        OPS.lsq_bmm_w8_q8(torch.zeros(1, 65537, dtype=U8), a[1], a[2], torch.zeros(1, 65537, dtype=I8), a[4], a[5], True, F32)
    from torchlsq import extension as E
    with pytest.raises(RuntimeError, match="`out` must be a uint8 tensor of shape"):
        E.attn_w8_bmm_q(*a, *q, F32, out=torch.zeros(2, 4, 6, dtype=U8))
    x, tab = A.score_rows(3, 16, 0, U8), A.table()
    with pytest.raises(RuntimeError, match="levels must be uint8"):
        OPS.lsq_softmax_w8_q8(x.float(), tab, F32)
    with pytest.raises(RuntimeError, match=r"dense int32 tensor of \[256\]"):
        OPS.lsq_softmax_w8_q8(x, tab[:255], F32)
    with pytest.raises(RuntimeError, match=r"dense int32 tensor of \[256\]"):
        OPS.lsq_softmax_w8_q8(x, tab.long(), F32)
    with pytest.raises(RuntimeError, match="row_pad = 0 must be at least 1"):
        OPS.lsq_softmax_w8_q8_q(x, tab, *A.PROB_Q, F32, 0)
    with pytest.raises(RuntimeError, match="at most 65536"):
        OPS.lsq_softmax_w8_q8(torch.zeros(1, 65537, dtype=U8), tab, F32)
    with pytest.raises(RuntimeError, match="`out` must be a uint8 tensor"):
        E.attn_w8_softmax_q(x, tab, *A.PROB_Q, F32, 1, out=torch.zeros(3, 16, dtype=I8))
    # inference only
    with pytest.raises(RuntimeError, match="grad|inference"):
        OPS.lsq_bmm_w8_q8(a[0], a[1].clone().requires_grad_(True), *a[2:], F32)


# ---------------------------------------------------------------------------------------------------
# the batched matmul's definition
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_dtype,b_dtype", [(U8, U8), (U8, I8), (I8, U8), (I8, I8)])
@pytest.mark.parametrize("nt", [True, False])
def test_bmm_equals_plain_python_integers(a_dtype, b_dtype, nt):
    """tiny shapes, all four pairings, zero points at both ends of their range"""
    for za, zb, seed in ((0, 255, 0), (255, 0, 1), (117, 131, 2)):
        ops = A.bmm_operands((2, 2), 3, 4, 7, nt, seed, a_dtype, b_dtype, za=za, zb=zb)
        I = np.array(A.bmm_int_reference(ops[0], ops[2], ops[3], ops[5], nt), dtype=np.int64).reshape(2, 2, 3, 4)
        assert np.abs(I).max() > 10000
        want = (np.float32(A.S_B) * I.astype(np.float32)) * np.float32(A.S_A)
        got = A.run_bmm("cpu", ops, None, F32)
        assert got.dtype == F32 and got.shape == (2, 2, 3, 4) and np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
        for mid in (BF16, F16):
            g = A.run_bmm("cpu", ops, None, mid)
            assert g.dtype == mid and torch.equal(A.bits(g), A.bits(torch.from_numpy(want).to(mid)))
        for unsigned in (True, False):
            q = A.fit_quantizer(got, unsigned)
            lv = A.run_bmm("cpu", ops, q, BF16)
            ref = OPS.lsq_levels_per_tensor(torch.from_numpy(want).to(BF16), *q, 0)
            assert lv.dtype == (U8 if unsigned else I8) and torch.equal(lv.view(I8), ref.view(I8)) and len(lv.unique()) > 8


@pytest.mark.parametrize("a_dtype,b_dtype", [(U8, U8), (U8, I8), (I8, U8), (I8, I8)])
def test_bmm_equals_the_w8a8_linear_per_batch_slice(a_dtype, b_dtype):
    """B[b] wrapped as a per-tensor quantized weight with no bias, floats out: bit for bit `lsq_linear_w8a8`"""
    from torchlsq.functional import lsq_linear_w8a8
    ops = A.bmm_operands(3, 9, 11, 40, True, 5, a_dtype, b_dtype)
    for mid in A.MIDS:
        got = A.run_bmm("cpu", ops, None, mid)
        for i in range(3):
            xq = torch._make_per_tensor_quantized_tensor(ops[0][i], A.S_A, int(ops[2]))
            wq = torch._make_per_tensor_quantized_tensor(ops[3][i], A.S_B, int(ops[5]))
            assert torch.equal(A.bits(got[i]), A.bits(lsq_linear_w8a8(xq, wq, out_dtype=mid))), (mid, i)
    # the NN form is the NT form of the transposed copy
    nn = ops[:3] + (ops[3].transpose(-1, -2).contiguous(),) + ops[4:6] + (False,)
    assert torch.equal(A.run_bmm("cpu", nn, None, F32), A.run_bmm("cpu", ops, None, F32))


def test_bmm_sums_beyond_32_bits():
    """K = 65536 with extreme levels: |I| = 65536 * 255 * 255 > 2^31"""
    a = torch.full((1, 65536), 255, dtype=U8)
    b = torch.stack([torch.full((65536,), 127, dtype=I8), torch.full((65536,), -128, dtype=I8)])
    ops = (a, one(A.S_A), one(0, torch.int32), b, one(A.S_B), one(-128, torch.int32), True)
    got = A.run_bmm("cpu", ops, None, F32)
    I = np.array([[65536 * 255 * 255, 0]], dtype=np.int64)
    assert I[0, 0] > 2 ** 31
    want = (np.float32(A.S_B) * I.astype(np.float32)) * np.float32(A.S_A)
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    ops = (a, one(A.S_A), one(255, torch.int32), b, one(A.S_B), one(127, torch.int32), True)
    assert torch.equal(A.run_bmm("cpu", ops, None, F32), torch.zeros(1, 2))


def test_bmm_reads_strided_views_like_their_copies():
    from torchlsq.functional import LevelsTensor, lsq_bmm_w8, lsq_bmm_w8_q
    qkv = A.levels((2, 19, 3, 3, 32), 7, U8)
    q, k, v = A.qkv_heads(qkv)
    dense = [LevelsTensor(t.levels.contiguous(), t.scale, t.zero_point, 0, 255) for t in (q, k, v)]
    s = lsq_bmm_w8(q, k, True)
    assert s.shape == (2, 3, 19, 19) and torch.equal(s, lsq_bmm_w8(dense[0], dense[1], True))
    oq = A.fit_quantizer(s, True)
    p = lsq_bmm_w8_q(q, k, True, *oq, mid_dtype=BF16)
    # padded rows whose padding holds 0xFF, and a view without unit innermost stride (made dense first)
    pp = LevelsTensor(A.padded(p.levels, 32), p.scale, p.zero_point, 0, 255)
    c = lsq_bmm_w8(pp, v)
    assert c.shape == (2, 3, 19, 32) and torch.equal(c, lsq_bmm_w8(p, dense[2]))
    kt = LevelsTensor(k.levels.transpose(-1, -2), k.scale, k.zero_point, 0, 255)
    assert kt.levels.stride(-1) != 1 and torch.equal(lsq_bmm_w8(q, kt), s)
    # written through the [B, H, T, D] view of a [B, T, H D] buffer: the bytes of the dense result, nothing else touched
    cq = A.fit_quantizer(c, False)
    want = lsq_bmm_w8_q(p, v, False, *cq, mid_dtype=F16)
    buf = torch.full((2, 19, 96), 77, dtype=I8)
    got = lsq_bmm_w8_q(pp, v, False, *cq, mid_dtype=F16, out=buf.view(2, 19, 3, 32).permute(0, 2, 1, 3))
    assert torch.equal(buf.view(2, 19, 3, 32).permute(0, 2, 1, 3), want.levels) and got.levels.data_ptr() == buf.data_ptr()
    assert torch.equal(got.scale, want.scale) and torch.equal(got.zero_point, want.zero_point) and len(want.levels.unique()) > 32
    # 2-D and 3-D inputs, a 2-D operand beside a batched one, 1-D operands as torch.matmul takes them
    q2 = LevelsTensor(dense[0].levels[0, 0], q.scale, q.zero_point, 0, 255)
    k2 = LevelsTensor(dense[1].levels[0, 0], k.scale, k.zero_point, 0, 255)
    assert torch.equal(lsq_bmm_w8(q2, k2, True), s[0, 0])
    assert torch.equal(lsq_bmm_w8(LevelsTensor(dense[0].levels[0], q.scale, q.zero_point, 0, 255), k2, True)[1], lsq_bmm_w8(
        LevelsTensor(dense[0].levels[0, 1], q.scale, q.zero_point, 0, 255), k2, True))
    q1 = LevelsTensor(dense[0].levels[0, 0, 0], q.scale, q.zero_point, 0, 255)
    k1 = LevelsTensor(dense[1].levels[0, 0, 3], k.scale, k.zero_point, 0, 255)
    assert lsq_bmm_w8(q1, k2, True).shape == (19,) and torch.equal(lsq_bmm_w8(q1, k2, True), s[0, 0, 0])
    assert lsq_bmm_w8(q1, k1).shape == () and torch.equal(lsq_bmm_w8(q1, k1), s[0, 0, 0, 3])
    assert lsq_bmm_w8(q2, k1).shape == (19,) and torch.equal(lsq_bmm_w8(q2, k1), s[0, 0, :, 3])
    # empty batches
    e = LevelsTensor(dense[0].levels[:0], q.scale, q.zero_point, 0, 255)
    assert lsq_bmm_w8(e, LevelsTensor(dense[1].levels[:0], k.scale, k.zero_point, 0, 255), True).shape == (0, 3, 19, 19)


# ---------------------------------------------------------------------------------------------------
# the softmax's definition
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [U8, I8])
def test_softmax_step_by_step(dtype):
    for (R, C, seed), tab in (((5, 197, 0), A.table()), ((3, 16, 1), A.table_with_zeros()), ((2, 1000, 2), A.table(0.02, 1.0))):
        x = A.score_rows(R, C, seed, dtype)
        E, S, p = A.softmax_numpy(x, tab)
        assert S.min() >= 1 << 24
        got = A.run_softmax("cpu", x, tab, None, F32)
        assert got.shape == (R, C) and np.array_equal(got.numpy().view(np.int32), p.view(np.int32))
        for mid in (BF16, F16):
            g = A.run_softmax("cpu", x, tab, None, mid)
            assert torch.equal(A.bits(g), A.bits(torch.from_numpy(p).to(mid)))
            lv = A.run_softmax("cpu", x, tab, A.PROB_Q, mid)
            assert lv.dtype == U8 and torch.equal(lv, OPS.lsq_levels_per_tensor(torch.from_numpy(p).to(mid), *A.PROB_Q, 0).view(U8))
        qi = (one(1.0 / 255), one(128.0 / 255), -128, 127, -128, 127)
        lv = A.run_softmax("cpu", x, tab, qi, F32)
        assert lv.dtype == I8 and int(lv.min()) == -128 and int(lv.max()) > -128
        assert torch.equal(lv, OPS.lsq_levels_per_tensor(torch.from_numpy(p), *qi, 0))


def test_softmax_edge_rows():
    tab, tz = A.table(), A.table_with_zeros()
    # C = 1 gives exactly 1.0
    for dtype in (U8, I8):
        for b in (0, 255):
            x = torch.tensor([[b]], dtype=U8).view(dtype)
            assert A.run_softmax("cpu", x, tab, None, F32).item() == 1.0
            assert A.run_softmax("cpu", x, tab, A.PROB_Q, BF16).item() == 255
    # an all-equal row: 1 / C, one float32 division
    for C in (3, 197, 1000):
        got = A.run_softmax("cpu", torch.full((2, C), 9, dtype=I8), tab, None, F32)
        want = np.float32(1 << 24) * (np.float32(1.0) / np.float32((1 << 24) * C))
        assert (got.numpy() == want).all()
    # one maximum, the rest 255 below it, on a table whose far entries are zero: exactly one and zeros
    x = torch.zeros(2, 64, dtype=U8)
    x[0, 5] = x[1, 63] = 255
    got = A.run_softmax("cpu", x, tz, None, F32)
    assert int(tz[255]) == 0 and got.sum().item() == 2.0 and got[0, 5].item() == 1.0 and got[1, 63].item() == 1.0
    xi = (x.to(torch.int16) - 128).to(I8)
    assert torch.equal(A.run_softmax("cpu", xi, tz, None, F32), got)
    # S beyond 2^32: C = 65536 with alpha = 0, every entry 2^24, S = 2^40
    from torchlsq.functional import lsq_softmax_table
    full = lsq_softmax_table(one(0.05), 0.0)
    assert torch.equal(full, A.full_table())
    x = A.levels((1, 65536), 3, U8)
    got = A.run_softmax("cpu", x, full, None, F32)
    assert (got == 2.0 ** -16).all()


@pytest.mark.parametrize("s_x,alpha,C", A.TRIALS)
def test_softmax_against_float64_and_aten(s_x, alpha, C):
    """the derived bound against softmax in float64, and at most one level against F.softmax taken to levels through bfloat16; the
    share of levels that differ is measured and printed, not capped"""
    from torchlsq.functional import LevelsTensor
    R = 2 if C > 10000 else 64
    tab = A.table(s_x, alpha)
    worst, differ, total = 0.0, 0, 0
    for dtype, z in ((U8, 128), (I8, 0)):
        x = A.score_rows(R, C, C, dtype, spread=min(200, 8.0 / (s_x * alpha)))
        E, S, p = A.softmax_numpy(x, tab)
        t = np.float64(np.float32(s_x)) * np.float64(np.float32(alpha))
        b = x.numpy().astype(np.float64)
        e = np.exp(-t * (b.max(-1, keepdims=True) - b))
        p_star = e / e.sum(-1, keepdims=True)
        err = np.abs(p.astype(np.float64) - p_star)
        assert (err <= A.softmax_bound(p.astype(np.float64), p_star, S.astype(np.float64), C)).all()
        worst = max(worst, float((err * (S / 2.0 ** 24)).max()))
        lt = LevelsTensor(x, one(s_x), one(z, torch.int32), *((0, 255) if dtype == U8 else (-128, 127)))
        ref = torch.softmax(lt.dequantize(F32) * np.float32(alpha), -1).to(BF16)
        ref = OPS.lsq_levels_per_tensor(ref, *A.PROB_Q, 0).view(U8).to(torch.int16)
        got = A.run_softmax("cpu", x, tab, A.PROB_Q, BF16).to(torch.int16)
        assert int((got - ref).abs().max()) <= 1
        differ, total = differ + int((got != ref).sum()), total + got.numel()
    print("softmax s_x=%g alpha=%g C=%d: worst error * S / 2^24 = %.3g; %d of %d levels differ from F.softmax's" % (s_x, alpha, C, worst, differ, total))
    assert worst < 1.0          # (1 + C p*) / 2 in table units over S / 2^24 >= 1 rows, far below one unit here


def test_softmax_table():
    from torchlsq.functional import lsq_softmax_table
    for s_x, alpha in ((0.05, 1.0), (0.1, 0.125), (0.3, 1.0), (0.004, 1.0), (1e-6, 1.0)):
        t = lsq_softmax_table(one(s_x), alpha)
        assert t.dtype == torch.int32 and t.shape == (256,) and int(t[0]) == 1 << 24 and bool((t[1:] <= t[:-1]).all()) and int(t.min()) >= 0
        step = np.float64(np.float32(s_x)) * np.float64(np.float32(alpha))
        want = np.rint(np.exp(-step * np.arange(256, dtype=np.float64)) * 2.0 ** 24)
        assert np.abs(t.numpy() - want).max() <= 1
    # alpha folds into the scale: products that are the same float64 number give the same table
    assert torch.equal(lsq_softmax_table(one(0.5), 0.25), lsq_softmax_table(one(0.125), 1.0))
    assert torch.equal(lsq_softmax_table(one(0.05), 0.0), A.full_table())
    assert torch.equal(lsq_softmax_table(torch.tensor(0.05), 1.0), A.table())


def test_softmax_reads_and_writes_strided_rows():
    from torchlsq.functional import LevelsTensor, lsq_softmax_w8, lsq_softmax_w8_q
    tab = A.table()
    x = A.score_rows(2 * 3 * 5, 197, 4, U8).view(2, 3, 5, 197)
    lt = LevelsTensor(x, one(0.05), one(128, torch.int32), 0, 255)
    want = lsq_softmax_w8_q(lt, tab, *A.PROB_Q[:4], mid_dtype=BF16)
    assert want.levels.shape == x.shape and want.levels.is_contiguous()
    pad = LevelsTensor(A.padded(x, 208), lt.scale, lt.zero_point, 0, 255)
    got = lsq_softmax_w8_q(pad, tab, *A.PROB_Q[:4], mid_dtype=BF16, row_pad=16)
    assert got.levels.shape == x.shape and got.levels.stride() == (3 * 5 * 208, 5 * 208, 208, 1) and torch.equal(got.levels, want.levels)
    assert got.levels.data_ptr() % 16 == 0
    buf = torch.full((2, 3, 5, 208), 0x5A, dtype=U8)
    lsq_softmax_w8_q(lt, tab, *A.PROB_Q[:4], mid_dtype=BF16, out=buf[..., :197])
    assert torch.equal(buf[..., :197], want.levels) and bool((buf[..., 197:] == 0x5A).all())
    # a view without unit innermost stride is made dense first
    xt = LevelsTensor(x.transpose(-1, -2).contiguous().transpose(-1, -2), lt.scale, lt.zero_point, 0, 255)
    assert xt.levels.stride(-1) != 1 and torch.equal(lsq_softmax_w8(xt, tab), lsq_softmax_w8(lt, tab))
    assert lsq_softmax_w8(LevelsTensor(x[:0], lt.scale, lt.zero_point, 0, 255), tab).shape == (0, 3, 5, 197)
    assert torch.equal(lsq_softmax_w8(LevelsTensor(x[0, 0, 0], lt.scale, lt.zero_point, 0, 255), tab), lsq_softmax_w8(lt, tab)[0, 0, 0])


# ---------------------------------------------------------------------------------------------------
# modules and fake kernels
# ---------------------------------------------------------------------------------------------------
def test_modules_against_the_functional_forms():
    from torchlsq.functional import LevelsTensor, lsq_bmm_w8, lsq_bmm_w8_q, lsq_softmax_table, lsq_softmax_w8, lsq_softmax_w8_q
    from torchlsq.quantized import AttentionCoreW8Q, MatmulW8Q, SoftmaxW8Q
    from torchlsq.quantized.modules.packed_linear_a8 import _per_tensor_constants
    core, qkv, want = A.core_case(2, 3, 19, 32)
    q, k, v = A.qkv_heads(qkv)
    sq, pq, oq = (_per_tensor_constants(m, "test") for m in (A.trained(-1, 1), A.trained(0.0, 1.0), A.trained(-1.0, 1.0)))
    sq = _per_tensor_constants(A.trained(*[c * 6.0 * A.QKV_S ** 2 * 74 * 74 * 32 ** 0.5 for c in (-1, 1)]), "test")
    s = lsq_bmm_w8_q(q, k, True, *sq, mid_dtype=BF16)
    tab = lsq_softmax_table(s.scale, 32 ** -0.5)
    assert torch.equal(core.softmax.table, tab) and "table" in dict(core.softmax.named_buffers())
    p = lsq_softmax_w8_q(s, tab, *pq, mid_dtype=BF16)
    c = lsq_bmm_w8_q(p, v, False, *oq, mid_dtype=BF16)
    assert want.levels.shape == (2, 19, 96) and want.levels.is_contiguous() and len(want.levels.unique()) > 32
    assert torch.equal(want.levels.view(2, 19, 3, 32).permute(0, 2, 1, 3), c.levels)
    assert torch.equal(want.scale, c.scale) and torch.equal(want.zero_point, c.zero_point) and want.quant_max == c.quant_max
    assert len(s.levels.unique()) > 64 and len(p.levels.unique()) > 16
    # the parts
    mm = MatmulW8Q(A.trained(-1.0, 1.0), mid_dtype=BF16)
    assert torch.equal(mm(p, v).levels, c.levels) and torch.equal(mm.matmul(p, v).levels, c.levels) and "transpose_b=False" in repr(mm)
    f = MatmulW8Q(None, True, F16)(q, k)
    assert f.dtype == F16 and torch.equal(f, lsq_bmm_w8(q, k, True, F16))
    sm = SoftmaxW8Q(s.scale, None, 32 ** -0.5, F32)
    assert torch.equal(sm(s), lsq_softmax_w8(s, tab)) and "floats out" in repr(sm)
    sm2 = SoftmaxW8Q(A.trained(0.0, 1.0), A.trained(0.0, 1.0), 1.0, BF16, row_pad=16)
    y = sm2(p)
    assert isinstance(y, LevelsTensor) and y.levels.stride(-2) == 32 and torch.equal(sm2.table, lsq_softmax_table(p.scale, 1.0))
    # state: the table and the constants travel as buffers
    sd = core.state_dict()
    assert {"softmax.table", "scores.output_scale", "softmax.output_shift", "context.output_scale"} <= set(sd)
    with pytest.raises(ValueError, match="LSQFakeQuantizer"):
        MatmulW8Q(torch.nn.Identity())
    with pytest.raises(AssertionError, match="reads levels"):
        mm(p.levels, v)
    with pytest.raises(AssertionError, match="one shape"):
        core(q, k, LevelsTensor(v.levels[:, :2], v.scale, v.zero_point, 0, 255))


def test_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    a = A.bmm_operands((2, 3), 5, 7, 16, True)
    nn = A.bmm_operands((2, 3), 5, 7, 16, False)
    q = A.fit_quantizer(torch.tensor([-1.0, 1.0]), False)
    x, tab = A.score_rows(6, 197, 0, U8).view(2, 3, 197), A.table()
    with FakeTensorMode() as mode:
        def fk(args):
            return tuple(mode.from_tensor(t) if isinstance(t, torch.Tensor) else t for t in args)
        y = OPS.lsq_bmm_w8_q8(*fk(a), BF16)
        assert y.shape == (2, 3, 5, 7) and y.dtype == BF16
        y = OPS.lsq_bmm_w8_q8_q(*fk(nn), *fk(q), F32)
        assert y.shape == (2, 3, 5, 7) and y.dtype == I8
        y = OPS.lsq_softmax_w8_q8(*fk((x, tab)), F16)
        assert y.shape == (2, 3, 197) and y.dtype == F16
        y = OPS.lsq_softmax_w8_q8_q(*fk((x, tab)), *fk(A.PROB_Q), F32, 16)
        assert y.shape == (2, 3, 197) and y.dtype == U8 and y.stride() == (3 * 208, 208, 1)
    real = OPS.lsq_softmax_w8_q8_q(x, tab, *A.PROB_Q, F32, 16)
    assert real.shape == (2, 3, 197) and real.stride() == (3 * 208, 208, 1)


# ---------------------------------------------------------------------------------------------------
# views whose rows overlap, and zero points far outside the level range
# ---------------------------------------------------------------------------------------------------
def test_bmm_operands_whose_rows_overlap_are_copied_and_such_an_out_is_refused():
    """an expanded row (row stride 0) and a sliding window (row stride 2 over 40 bytes) are read like their contiguous copies: the
    library is handed the tensor's own strides or a dense copy, never a row stride the storage does not have"""
    from torchlsq import extension as E
    from torchlsq._attn_w8_host import _in_place, _rows_apart, _strides4
    base = A.levels((40,), 21, U8)
    row = base[:32].unsqueeze(0).expand(5, 32)                      # strides (0, 1) over 32 bytes
    win = base.as_strided((5, 32), (2, 1))                          # strides (2, 1) over 40 bytes
    other = A.levels((7, 32), 22, I8)
    s, za, zb = one(A.S_A), one(117, torch.int32), one(3, torch.int32)
    for v in (row, win):
        assert v.stride(-1) == 1 and not _rows_apart(v) and v.untyped_storage().nbytes() == 40
        for on_gpu in (False, True):
            c = _in_place(v, on_gpu)
            assert c.is_contiguous() and c.data_ptr() != v.data_ptr() and torch.equal(c, v) and _strides4(c).ld == 32
        dense = v.contiguous()
        for nt, b in ((True, other), (False, other.t().contiguous())):
            want = OPS.lsq_bmm_w8_q8(dense, s, za, b, s, zb, nt, F32)
            assert torch.equal(OPS.lsq_bmm_w8_q8(v, s, za, b, s, zb, nt, F32), want)
        # as the B operand, in both forms
        want = OPS.lsq_bmm_w8_q8(other, s, zb, dense, s, za, True, F32)
        assert want.shape == (7, 5) and torch.equal(OPS.lsq_bmm_w8_q8(other, s, zb, v, s, za, True, F32), want)
        a2 = A.levels((3, 5), 23, U8)
        assert torch.equal(OPS.lsq_bmm_w8_q8(a2, s, za, v, s, za, False, F32), OPS.lsq_bmm_w8_q8(a2, s, za, dense, s, za, False, F32))
    # a batch that repeats (batch stride 0) is read in place: the strides are its own
    rep = other.unsqueeze(0).expand(3, 7, 32)
    assert _in_place(rep, True) is rep and (_strides4(rep).s1, _strides4(rep).ld) == (0, 32)
    a3 = A.levels((3, 5, 32), 24, U8)
    assert torch.equal(OPS.lsq_bmm_w8_q8(a3, s, za, rep, s, zb, True, F32), OPS.lsq_bmm_w8_q8(a3, s, za, rep.contiguous(), s, zb, True, F32))
    # one row: no row stride to speak of
    assert _strides4(base[:32].unsqueeze(0)).ld == 32 and _strides4(torch.empty(1, 32, dtype=U8).as_strided((1, 32), (0, 1))).ld == 32
    # an `out` whose rows overlap is refused before the library sees it; the library refuses overlapping batches itself
    q = A.fit_quantizer(torch.tensor([-1.0, 1.0]), True)
    ops = (a3, s, za, rep, s, zb, True)
    for bad in (torch.zeros(3 * 5 * 7, dtype=U8).as_strided((3, 5, 7), (35, 2, 1)), torch.zeros(3, 1, 7, dtype=U8).expand(3, 5, 7)):
        with pytest.raises(RuntimeError, match="whose rows do not overlap"):
            E.attn_w8_bmm_q(*ops, *q, F32, out=bad)
    with pytest.raises(RuntimeError, match="y's rows or batches overlap each other"):
        E.attn_w8_bmm_q(*ops, *q, F32, out=torch.zeros(5, 7, dtype=U8).unsqueeze(0).expand(3, 5, 7))


def test_bmm_zero_points_far_outside_the_level_range():
    """|z| up to 32767 is inside the contract: the sum passes 2^31 at K = 7 already and is still the plain integers'"""
    for za, zb in ((32767, -32768), (-30000, -30000), (3, 32767)):
        a, b = A.levels((2, 3, 7), 31, U8), A.levels((2, 4, 7), 32, I8)
        ops = (a, one(A.S_A), one(za, torch.int32), b, one(A.S_B), one(zb, torch.int32), True)
        I = np.array(A.bmm_int_reference(a, za, b, zb, True), dtype=np.int64)
        assert za == 3 or np.abs(I).min() > 2 ** 31
        want = (np.float32(A.S_B) * I.astype(np.float32)) * np.float32(A.S_A)
        assert np.array_equal(A.run_bmm("cpu", ops, None, F32).numpy().view(np.int32), want.view(np.int32))
