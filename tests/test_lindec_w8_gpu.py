"""liblsq_hip_lindec_w8.so on the GPU: every byte against the plain reference of tests/test_lindec_w8_cpu.py and against the existing
GPU op on the same operands.  No tolerance anywhere."""
import copy

import pytest
import torch

import test_lindec_w8_cpu as C
from test_lindec_w8_cpu import BF16, F16, F32, I8, NONE, PRE, RES, U8
from torchlsq import _lindec_w8_host as HOST
from torchlsq import extension as E
from w8_routes import entered

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SYMBOL = "lsq_lindec_w8_linear_levels"      # the library's one launch


def _dec(c, **kw):
    """the new op on the case's operands, held to ONE entry into liblsq_hip_lindec_w8.so: the comparison below it is on that kernel's bytes"""
    with entered(HOST) as names:
        got = C.run(c, DEV, **kw)
    assert names == [SYMBOL], names
    return got


def _existing(c):
    """the op of before, which never enters that library"""
    with entered(HOST) as names:
        old = C.run(c, DEV, dec=False)
    assert names == [], names
    return old


def _big_n():
    return 16 * (torch.cuda.get_device_properties(0).multi_processor_count + 1)     # the persistent loop's second pass


# (M, N, K, residual, x, weight, residual and output level types, mid_dtype, relu, bias); N = 0 stands for 16 (CUs + 1).
# K: 16 less than one wave's step, 272 a partial step and idle waves, 4096 resident, 4112 restaged per tile; N: 40 a tail tile, clamped
# rows, byte stores.  (A case needs some hundred outputs to meet requant_w8_cases' condition: M = 1 goes with the widest N.)
# The last row: K = 8208 is a first, a middle and a last chunk of 16 k.
CASES = [(16, 16, 16, PRE, U8, I8, U8, True, BF16, False, "f32"),
         (3, 40, 16, RES, U8, I8, U8, True, BF16, False, "f32"),
         (16, 48, 16, NONE, U8, I8, U8, True, BF16, False, "f32"),
         (3, 40, 272, NONE, U8, I8, U8, True, F32, False, "f32"),
         (16, 40, 272, RES, I8, U8, I8, False, BF16, False, "f32"),
         (3, 40, 272, PRE, U8, I8, U8, True, F16, False, None),
         (16, 16, 4096, NONE, U8, I8, U8, True, BF16, False, "f32"),
         (3, 40, 4096, RES, U8, I8, U8, True, BF16, False, "f32"),
         (16, 48, 4096, PRE, U8, U8, I8, False, F16, False, "f32"),
         (16, 16, 4112, NONE, I8, I8, U8, False, BF16, False, None),
         (3, 40, 4112, RES, U8, I8, U8, True, F32, False, "f32"),
         (16, 48, 4112, PRE, U8, I8, U8, True, BF16, False, "f32"),
         (1, 0, 64, NONE, U8, I8, U8, True, BF16, True, "f32"),
         (16, 0, 64, RES, U8, I8, U8, True, BF16, True, "f32"),
         (3, 0, 64, PRE, I8, U8, I8, False, F16, False, "f32"),
         (1, 0, 64, RES, U8, I8, U8, True, F32, False, "f32"),
         (16, 48, 272, RES, U8, I8, U8, True, F32, False, None),
         (16, 16, 272, NONE, U8, I8, U8, False, BF16, False, "f32"),
         (3, 40, 8208, RES, U8, I8, U8, True, BF16, False, "f32")]


def _case(spec):
    spec = list(spec)
    spec[1] = spec[1] or _big_n()
    return C.case(*spec)


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "-".join(str(v).replace("torch.", "") for v in s))
def test_bytes_equal_the_reference_and_the_existing_op(spec):
    _assert_bytes(_case(spec), spec[0], spec[2])


def _assert_bytes(c, M, K):
    assert E.lindec_w8_plan(M, c["want"].shape[1], K)["served"]
    got, old = _dec(c), _existing(c)
    again = _dec(c)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), c["want"]) and torch.equal(got, old) and torch.equal(got, again)
    if M > 1:           # a row's bytes depend on that row alone
        one = dict(lin=(c["lin"][0][1:2],) + c["lin"][1:], res=None if c["res"] is None else (c["res"][0][1:2],) + c["res"][1:])
        assert torch.equal(_dec(one).cpu(), c["want"][1:2])


def test_rows_on_either_side_of_the_lds_opt_in():
    """K = 4096: the largest M whose plan stays within the 64 KB a kernel has without the opt-in, and the first M beyond them"""
    below = max(M for M in range(1, 17) if E.lindec_w8_plan(M, 40, 4096)["lds_bytes"] <= 65536)
    assert below == 11 and E.lindec_w8_plan(below + 1, 40, 4096)["lds_bytes"] > 65536
    for M in (below, below + 1):
        _assert_bytes(C.case(M, 40, 4096, RES), M, 4096)


@pytest.mark.parametrize("kind", [NONE, PRE])
def test_longest_k_with_border_levels(kind):
    """K = 65536, M = N = 16, tests/test_lindec_w8_cpu.py's `extreme_lin`: (15, 14) has every raw product at 2^14, the raw int32 sum at
    2^30 and I = 65536 * 255 * 255 > 2^31, and (15, 15) has I = -65536 * 255 * 255"""
    lin = C.extreme_lin()
    osc, rng, res = lin[7], lin[9], None
    if kind == PRE:
        res = (C.W.levels((16, 16), 0, 255, 5), 0.4 * osc, torch.tensor([128], dtype=torch.int32), 1.1 * osc, -128 * 1.1 * osc, 0, 255, 0, 255)
    c = dict(lin=lin, res=res)
    want = C.reference(c)
    C.R.assert_not_vacuous(want, rng, "K = 65536")
    got, old = _dec(c), _existing(c)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want) and torch.equal(got, old)


@pytest.mark.parametrize("spec", [(3, 40, 272, PRE), (16, 48, 4112, RES), (16, 16, 64, NONE)])
def test_odd_byte_offsets_and_guard_bytes(spec):
    """y and the residual at odd byte offsets inside larger buffers (byte stores and byte loads); the guard bytes stay as they were"""
    c = C.case(*spec)
    M, N = c["want"].shape
    buf = torch.full((M * N + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    out = buf[31:31 + M * N].view(M, N)
    if c["res"] is not None:
        rbuf = torch.full((M * N + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        rbuf[13:13 + M * N] = c["res"][0].to(DEV).flatten()
        c = dict(c, res=(rbuf[13:13 + M * N].view(M, N),) + c["res"][1:])
    K, has_res = spec[2], c["res"] is not None
    pl = E.lindec_w8_plan(M, N, K, True, False, not has_res)        # the call's own alignment: y at 31, the residual at 13
    assert pl["served"] and pl["store"] == "bytes" and (not has_res or pl["res_load"] == "bytes")
    assert out.data_ptr() % 16 == 15 and (not has_res or c["res"][0].data_ptr() % 16 == 13)
    _dec(c, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), c["want"])
    assert bool((buf[:31] == 0x5A).all()) and bool((buf[31 + M * N:] == 0x5A).all())
    if c["res"] is not None:
        assert bool((rbuf[:13] == 0xA5).all()) and bool((rbuf[13 + M * N:] == 0xA5).all())


@pytest.mark.parametrize("spec", [(3, 40, 4112, PRE), (16, 48, 4096, NONE)])
def test_a_call_in_a_graph(spec):
    c = C.moved(C.case(*spec), DEV)                 # nothing is copied to the device during the capture
    eager = _dec(c)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _dec(c, out=out)                            # warm-up: the LDS opt-in is not captured
        out.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            held = _dec(c, out=out)                 # the capture enters the library once
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(held, eager) and torch.equal(out, eager)


def test_a_weight_at_an_odd_byte_offset_takes_the_existing_op():
    """the control of `entered`: dense weight levels that start at an odd byte of a larger buffer are not served, so the call runs
    the requant / resadd library -- no entry into this one -- and its bytes are the reference's all the same"""
    for kind in (NONE, PRE):
        c = C.case(3, 40, 272, kind)
        lw = c["lin"][3].to(DEV)
        buf = torch.zeros(lw.numel() + 32, dtype=lw.dtype, device=DEV)
        odd = buf[17:17 + lw.numel()].view(lw.shape).copy_(lw)
        assert odd.is_contiguous() and odd.data_ptr() % 16 == 1
        with entered(HOST) as names:
            got = C.run(dict(c, lin=c["lin"][:3] + (odd,) + c["lin"][4:]), DEV)
        torch.cuda.synchronize()
        assert names == [] and torch.equal(got.cpu(), c["want"])


def test_one_decode_step_of_the_llama_layer():
    """tests/decoder_glu_w8_cases.py's layer, prompt then single-token steps: with every linear's decode=True each stage and the
    cache hold the bytes they hold with decode=False (and the CPU run's)"""
    import decoder_glu_w8_cases as L
    from torchlsq.functional import LevelsTensor
    mid, name = torch.bfloat16, "short"
    xl = L.input_levels(name)
    xg = LevelsTensor(xl.levels.to(DEV), xl.scale.to(DEV), xl.zero_point.to(DEV), xl.quant_min, xl.quant_max)
    runs = {}
    for decode in (False, True):
        layer = copy.deepcopy(L.chain(name, mid)).to(DEV)
        for lin in (layer.qkv, layer.proj, layer.mlp.gate_up, layer.mlp.down):
            lin.decode = decode
        with torch.no_grad():
            runs[decode] = L.sequence(layer, xg, L.make_cache(name, "dense", DEV), L.chunks_of(name, "steps"))
    assert L.CASES[name]["B"] <= 16 and L.CASES[name]["steps"] >= 1
    assert L.differing(runs[True], runs[False]) == [] and L.differing(runs[True], L.cpu_run(name, mid, "steps")) == []
