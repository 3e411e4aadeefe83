"""The fused attention core on 8-bit levels (include/lsq_hip_attn_fused_w8.h), everything that needs no GPU: the library's exports
against its header and `_abi.py`, its one kernel (name and scratch, from the code object's metadata), the plan on both sides of every
threshold, the refusals, the CPU path of the op -- the three functional calls composed -- with the module's `fused=` option, the fake
kernel and the Autograd kernel on top, and that liblsq_hip_attn_w8.so still exports exactly its six names.
"""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch

import attn_fused_w8_cases as C
import attn_w8_cases as A
from helpers import demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_attn_fused_w8.h")
LIBDIR = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq")
LIB = os.path.join(LIBDIR, "liblsq_hip_attn_fused_w8.so")
NAMES = sorted(["lsq_attn_fused_w8_abi_version", "lsq_attn_fused_w8_last_error", "lsq_attn_fused_w8", "lsq_attn_fused_w8_plan"])
THREE_LAUNCH_NAMES = sorted(["lsq_attn_w8_abi_version", "lsq_attn_w8_last_error", "lsq_bmm_w8", "lsq_bmm_w8_plan", "lsq_softmax_w8",
                             "lsq_softmax_w8_plan"])
LSQ_EINVAL = -1
OPS = torch.ops.torchlsq
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
NOTHING = dict(family="three_launches", grid=0, block=0, rows_per_workgroup=0, lds_row_stride=0, lds_bytes=0, lds_dynamic=False,
               store="elements")


def _exported(lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    return [f.strip() for decl in body.split(";")
            for f in re.sub(r"^\s*(const void\*|int64_t|lsq_attn_w8_strides)", "", decl.strip()).split(",") if f.strip()]


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_attn_fused_w8\w*)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_ATTN_FUSED_W8) == NAMES
    assert _exported(LIB) == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear_", "lsq_qgemm_", "lsq_qconv_", "lsq_requant_", "lsq_resadd_",
                  "lsq_pool_", "lsq_dwconv_", "lsq_eltwise_", "lsq_norm_", "lsq_attn_", "lsq_bmm_", "lsq_softmax_"):
        assert other not in und, other
    assert E.attn_fused_w8_library().lsq_attn_fused_w8_abi_version() == E.ATTN_FUSED_W8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_ATTN_FUSED_W8_ABI_VERSION (\d+)", raw).group(1) == "1"
    for name, cls, words in (("lsq_attn_fused_w8_geom", E.LsqAttnFusedW8Geom, 20), ("lsq_attn_fused_w8_consts", E.LsqAttnFusedW8Consts, 8)):
        assert _fields(text, name) == [f[0] for f in cls._fields_] and ctypes.sizeof(cls) == words * 8, name


def test_the_three_launch_library_still_exports_exactly_its_six_names():
    assert _exported(os.path.join(LIBDIR, "liblsq_hip_attn_w8.so")) == THREE_LAUNCH_NAMES


def test_the_kernel(tmp_path):
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    assert len(every) == 1 and re.match(r"^(?:void )?lsq::attn_fused_w8_kernel\(", list(names.values())[0]), names
    (_, scratch), = every.values()
    assert scratch == 0, "the kernel uses %d bytes of scratch" % scratch


# ---------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------
def _ld(Tk):
    return 16 * (((Tk + 15) // 16) | 1)


def _expected(B, H, Tq, Tk, D, store="packets"):
    lds = 64 * _ld(Tk) + 1024 + 80 * D
    return dict(family="fused", grid=B * H * ((Tq + 63) // 64), block=256, rows_per_workgroup=64, lds_row_stride=_ld(Tk), lds_bytes=lds,
                lds_dynamic=lds > 65536, store=store)


def test_plans_without_a_gpu():
    from torchlsq import extension as E
    P = E.attn_fused_w8_plan
    for shape in ((1, 1, 1, 1, 16), (2, 3, 19, 19, 32), (32, 12, 197, 197, 64), (1, 2, 5, 197, 64), (1, 1, 130, 33, 32), (4, 12, 1024, 1024, 64),
                  (1, 1, 2048, 2048, 128), (3, 5, 64, 64, 128), (3, 5, 65, 64, 128)):
        assert P(*shape) == _expected(*shape), shape
    # D: 16 .. 128 in multiples of 16
    assert P(1, 2, 64, 64, 128)["family"] == "fused" and P(1, 2, 64, 64, 144) == NOTHING
    assert P(1, 2, 64, 64, 16)["family"] == "fused" and P(1, 2, 64, 64, 24) == NOTHING and P(1, 2, 64, 64, 8) == NOTHING
    # Tk: up to 2048; Tq: any
    assert P(1, 1, 64, 2048, 64)["family"] == "fused" and P(1, 1, 64, 2049, 64) == NOTHING
    assert P(1, 1, 5000, 2048, 64) == _expected(1, 1, 5000, 2048, 64)
    # one stride that is not a multiple of 16, per operand and per stride; y's only changes the store
    dense = (2 * 64 * 64, 64 * 64, 64)
    for name in ("q_strides", "k_strides", "v_strides"):
        for i in range(3):
            bad = tuple(s + (8 if j == i else 0) for j, s in enumerate(dense))
            assert P(2, 2, 64, 64, 64, **{name: bad}) == NOTHING, (name, i)
        assert P(2, 2, 64, 64, 64, **{name: tuple(s + 16 for s in dense)})["family"] == "fused"
    assert P(2, 2, 64, 64, 64, k_strides=(0, 0, 197)) == NOTHING                  # a dense [.., 197] stride
    assert P(2, 2, 64, 64, 64, qkv_aligned=False) == NOTHING
    assert P(2, 2, 64, 64, 64, y_aligned=False) == _expected(2, 2, 64, 64, 64, "elements")
    assert P(2, 2, 64, 64, 64, y_strides=(2 * 64 * 64 + 8, 64, 128)) == _expected(2, 2, 64, 64, 64, "elements")
    assert P(2, 2, 64, 64, 64, y_strides=(2 * 64 * 64 + 16, 64, 128))["store"] == "packets"
    # the LDS row stride: 16 n with n odd; the bytes, and where they pass 64 KB
    assert [P(1, 1, 1, T, 64)["lds_row_stride"] for T in (1, 16, 17, 32, 33, 197, 2032, 2033, 2048)] == [16, 16, 48, 48, 48, 208, 2032, 2064, 2064]
    assert P(1, 1, 1, 2048, 128)["lds_bytes"] == 143360 <= 163840
    lo, hi = P(1, 1, 1, 912, 64), P(1, 1, 1, 913, 64)                             # 64 * 912 + 1024 + 5120 = 64512; 64 * 944 + 6144 = 66560
    assert (lo["lds_bytes"], lo["lds_dynamic"], hi["lds_bytes"], hi["lds_dynamic"]) == (64512, False, 66560, True)
    assert max(P(1, 1, 1, T, D)["lds_bytes"] for T in (1, 197, 1024, 2048) for D in (16, 64, 128)) <= 163840
    # the dtypes do not move the plan
    assert P(2, 3, 19, 19, 32, q_dtype=I8, k_dtype=U8, v_dtype=I8) == _expected(2, 3, 19, 19, 32)


def test_plan_refusals_without_a_gpu():
    from torchlsq import extension as E
    lib = E.attn_fused_w8_library()
    err = lib.lsq_attn_fused_w8_last_error
    out = (ctypes.c_int32 * 8)()
    S = E.LsqAttnW8Strides

    def G(B=1, H=2, Tq=8, Tk=8, D=16, dt=(0, 0, 0), q=None, k=None, v=None, y=None):
        d = S(H * 8 * 16, 8 * 16, 16)
        return E.LsqAttnFusedW8Geom(B, H, Tq, Tk, D, *dt, q or d, k or d, v or d, y or d)

    def plan(g):
        return lib.lsq_attn_fused_w8_plan(ctypes.byref(g), 1, 1, ctypes.byref(out))

    assert plan(G()) == 0 and out[0] == 1
    assert lib.lsq_attn_fused_w8_plan(None, 1, 1, ctypes.byref(out)) == LSQ_EINVAL and b"NULL geometry" in err()
    assert lib.lsq_attn_fused_w8_plan(ctypes.byref(G()), 1, 1, None) == LSQ_EINVAL and b"NULL output" in err()
    for bad in (dict(B=0), dict(H=0), dict(Tq=0), dict(Tk=0), dict(D=0)):
        assert plan(G(**bad)) == LSQ_EINVAL and b"at least 1" in err(), bad
    assert plan(G(dt=(0, 2, 0))) == LSQ_EINVAL and b"must be LSQ_ATTN_W8_U8" in err()
    big = S(0, 0, 1 << 17)
    assert plan(G(D=65552, q=big, k=big, v=big, y=big)) == LSQ_EINVAL and b"at most 65536" in err()
    assert plan(G(Tk=65537)) == LSQ_EINVAL and b"at most 65536" in err()
    assert plan(G(Tk=65536)) == 0 and out[0] == 0
    assert plan(G(Tq=(1 << 20) + 1)) == LSQ_EINVAL and b"2^20" in err()
    assert plan(G(B=1 << 11, H=1 << 10)) == LSQ_EINVAL and b"2^20" in err()
    assert plan(G(k=S(256, 128, 15))) == LSQ_EINVAL and b"k's row stride 15 is smaller" in err()
    assert plan(G(v=S(-16, 128, 16))) == LSQ_EINVAL and b"must not be negative" in err()
    assert plan(G(y=S(256, 64, 16))) == LSQ_EINVAL and b"overlap each other" in err()
    assert plan(G(B=1 << 10, H=1 << 10, Tq=1 << 11, y=S(0, 0, 16))) == LSQ_EINVAL                 # (y overlaps itself)
    wide = S((1 << 31) * 16, (1 << 21) * 16, 16)
    assert plan(G(B=1 << 10, H=1 << 10, Tq=1 << 11, y=wide)) == LSQ_EINVAL and b"beyond 2^24 - 1" in err()


def test_entry_refusals_without_a_gpu():
    """everything is checked before anything is enqueued: none of these calls reaches the runtime (the pointers are host memory)"""
    from torchlsq import extension as E
    lib = E.attn_fused_w8_library()
    err = lib.lsq_attn_fused_w8_last_error
    S = E.LsqAttnW8Strides
    B, H, T, D = 1, 2, 8, 16
    qkv = torch.zeros(3 * B * H * T * D + 64, dtype=U8)
    ybuf = torch.zeros(B * H * T * D + 64, dtype=U8)
    base = qkv.data_ptr() + (-qkv.data_ptr()) % 16
    yp = ybuf.data_ptr() + (-ybuf.data_ptr()) % 16
    n = B * H * T * D
    f, z, tab = torch.ones(1), torch.zeros(1, dtype=torch.int32), A.table()
    d = S(H * T * D, T * D, D)

    def call(geom=None, consts="ok", sides=None, table=tab.data_ptr(), ptrs=None, y=yp, no_geom=False):
        g = geom or E.LsqAttnFusedW8Geom(B, H, T, T, D, 0, 0, 0, d, d, d, d)
        c = E.LsqAttnFusedW8Consts(*([f.data_ptr(), z.data_ptr()] * 4)) if consts == "ok" else consts
        side = E.LsqAttnW8Out(f.data_ptr(), f.data_ptr(), 0, 255, 0, 255, 0)
        s = [side, side, side] if sides is None else sides
        p = ptrs or (base, base + n, base + 2 * n)
        return lib.lsq_attn_fused_w8(None if no_geom else ctypes.byref(g), None if c is None else ctypes.byref(c),
                                     *(None if x is None else ctypes.byref(x) for x in s), table, p[0], p[1], p[2], y, None)

    assert call(no_geom=True) == LSQ_EINVAL and b"NULL geometry" in err()
    assert call(consts=None) == LSQ_EINVAL and b"NULL constants" in err()
    assert call(consts=E.LsqAttnFusedW8Consts(f.data_ptr(), z.data_ptr(), None, z.data_ptr(), f.data_ptr(), z.data_ptr(), f.data_ptr(),
                                              z.data_ptr())) == LSQ_EINVAL and b"NULL scale or zero point" in err()
    assert call(consts=E.LsqAttnFusedW8Consts(*([f.data_ptr() + 1, z.data_ptr()] * 4))) == LSQ_EINVAL and b"element-aligned" in err()
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
    assert call(y=base + n + 5) == LSQ_EINVAL and b"overlap" in err()                             # y inside k
    assert call(y=tab.data_ptr() + 16) == LSQ_EINVAL and b"overlap" in err()                      # y inside the table
    # legal, not served: the message says what to run instead
    assert call(ptrs=(base + 1, base + n, base + 2 * n)) == LSQ_EINVAL and b"not served by the fused kernel" in err()
    d24 = S(H * T * 24, T * 24, 24)
    assert call(geom=E.LsqAttnFusedW8Geom(B, H, T, T, 24, 0, 0, 0, d24, d24, d24, d24)) == LSQ_EINVAL and b"three launches" in err()
    assert bool((ybuf == 0).all())


# ---------------------------------------------------------------------------------------------------
# the op on the CPU: the three functional calls composed
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 16), (2, 3, 19, 19, 32), (1, 2, 65, 65, 64), (1, 2, 5, 197, 64), (1, 1, 130, 33, 32),
                                   (1, 2, 19, 19, 24), (1, 1, 40, 40, 144)], ids=str)
def test_op_on_cpu_tensors_equals_the_three_functional_calls(shape):
    for (dtypes, unsigned), mid in zip(C.COMBOS + ((C.ALL_U8, C.ALL_UNSIGNED),), (BF16, F32, F16)):
        c = C.case(*shape, 0, dtypes, unsigned, mid)
        C.check_not_degenerate(c)
        got = C.run(c, "cpu")
        assert got.shape == (shape[0], shape[2], shape[1] * shape[4]) and got.dtype == c.want.dtype and got.is_contiguous()
        assert torch.equal(got, c.want), (shape, dtypes, unsigned)
        assert torch.equal(OPS.lsq_attention_w8_q8_q(*C.flat_args(c, "cpu")), c.want)


def test_functional_form_returns_the_out_quantizers_levels_tensor():
    from torchlsq.functional import LevelsTensor, _act_constants, lsq_attention_w8_q
    c = C.case(2, 3, 19, 19, 32, 0, C.COMBOS[0][0], C.COMBOS[0][1])
    y = lsq_attention_w8_q(c.q, c.k, c.v, c.table, *c.sides, c.mid)
    o = c.sides[2]
    s, z = _act_constants(o[0], o[1], o[4], o[5])
    assert isinstance(y, LevelsTensor) and torch.equal(y.levels, c.want) and torch.equal(y.scale, s) and torch.equal(y.zero_point, z)
    assert (y.quant_min, y.quant_max, y.type_min, y.type_max) == tuple(o[2:])
    with pytest.raises(AssertionError, match="scale, shift, quant_min"):
        lsq_attention_w8_q(c.q, c.k, c.v, c.table, c.sides[0], None, c.sides[2], c.mid)
    with pytest.raises(AssertionError, match="LevelsTensor"):
        lsq_attention_w8_q(c.q.levels, c.k, c.v, c.table, *c.sides, c.mid)


def test_op_argument_validation():
    from torchlsq import extension as E
    c = C.case(2, 3, 19, 19, 32)
    args = list(C.flat_args(c, "cpu"))

    def bad(i, v, match):
        a = list(args)
        a[i] = v
        with pytest.raises(RuntimeError, match=match):
            OPS.lsq_attention_w8_q8_q(*a)

    bad(0, args[0].to(torch.int16), "must be uint8")
    bad(3, args[3][:, :2], r"q must be \[B, H, Tq, D\]")
    bad(6, args[6][:, :, :5], r"q must be \[B, H, Tq, D\]")
    bad(0, args[0][..., :16], r"q must be \[B, H, Tq, D\]")
    bad(1, torch.ones(2), "scale must be one float32")
    bad(5, torch.zeros(1), "zero point one int32")
    bad(9, args[9].to(torch.int64), "table must be a dense int32")
    bad(12, -1, "must lie within")
    bad(16, torch.ones(2), "out_scale and out_shift must be float32 tensors of one value")
    bad(28, torch.float64, "must be float32, bfloat16 or float16")
    out = torch.empty(2, 3, 19, 32, dtype=U8)
    assert E.attn_fused_w8_q(*args, out=out) is out and torch.equal(out.permute(0, 2, 1, 3).reshape(2, 19, 96), c.want)
    with pytest.raises(RuntimeError, match="`out` must be a uint8 tensor"):
        E.attn_fused_w8_q(*args, out=out.view(I8))
    with pytest.raises(RuntimeError, match="`out` must be a uint8 tensor"):
        E.attn_fused_w8_q(*args, out=out[:, :, :, :1].expand(2, 3, 19, 32))
    # nothing to compute
    a = list(args)
    a[0] = args[0][:, :, :0]
    assert OPS.lsq_attention_w8_q8_q(*a).shape == (2, 0, 96)


def test_module_fused_equals_three_launches_on_the_cpu():
    from torchlsq.quantized import AttentionCoreW8Q
    for shape in ((2, 3, 19, 32), (1, 2, 197, 64)):
        core, qkv, want = A.core_case(*shape)
        fused = copy.deepcopy(core)
        fused.fused = True
        got = fused(*A.qkv_heads(qkv))
        assert torch.equal(got.levels, want.levels) and torch.equal(got.scale, want.scale) and torch.equal(got.zero_point, want.zero_point)
        assert (got.quant_min, got.quant_max, got.type_min, got.type_max) == (want.quant_min, want.quant_max, want.type_min, want.type_max)
        assert list(fused.state_dict()) == list(core.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(fused.state_dict().values(), core.state_dict().values()))
    assert "fused=False" in repr(core) and "three launches" in repr(core) and "fused=True" in repr(fused)
    span = 6.0 * A.QKV_S * A.QKV_S * 74 * 74 * 8.0
    built = AttentionCoreW8Q(A.trained(-span, span), A.trained(0.0, 1.0), A.trained(-1.0, 1.0), alpha=0.125, mid_dtype=BF16, fused=True)
    assert built.fused is True and AttentionCoreW8Q(A.trained(-span, span), A.trained(0.0, 1.0), A.trained(-1.0, 1.0)).fused is False
    assert list(built.state_dict()) == list(core.state_dict())
    core, qkv, want = A.core_case(1, 2, 197, 64)
    assert torch.equal(built(*A.qkv_heads(qkv)).levels, want.levels)
    # fused=True serves q and k, v of different T; fused=False refuses them as before
    q, k, v = A.qkv_heads(qkv)
    from torchlsq.functional import LevelsTensor
    q5 = LevelsTensor(q.levels[:, :, :5], q.scale, q.zero_point, 0, 255)
    assert torch.equal(built(q5, k, v).levels, want.levels[:, :5])
    with pytest.raises(AssertionError, match="one shape"):
        core(q5, k, v)


def test_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for unsigned, dtype in (((True, False, True), U8), ((True, True, False), I8)):
        c = C.case(2, 3, 5, 19, 32, 0, C.ALL_U8, unsigned)
        assert c.want.dtype == dtype
        real = C.flat_args(c, "cpu")
        with FakeTensorMode() as mode:
            args = tuple(mode.from_tensor(t) if isinstance(t, torch.Tensor) else t for t in real)
            y = OPS.lsq_attention_w8_q8_q(*args)
            assert y.shape == (2, 5, 96) and y.dtype == dtype and y.stride() == (5 * 96, 96, 1)


def test_grad_is_refused():
    c = C.case(2, 3, 19, 19, 32)
    args = list(C.flat_args(c, "cpu"))
    for i in (1, 4, 7, 10, 11, 16, 17, 22, 23):
        a = list(args)
        a[i] = args[i].clone().requires_grad_(True)
        with pytest.raises(RuntimeError):
            OPS.lsq_attention_w8_q8_q(*a)
    assert not OPS.lsq_attention_w8_q8_q(*args).requires_grad
