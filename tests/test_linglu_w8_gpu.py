"""liblsq_hip_linglu_w8.so on the GPU: every byte against the plain reference of tests/test_linglu_w8_cpu.py, against the two-launch
route on the same operands and against a second launch.  No tolerance anywhere."""
import copy

import pytest
import torch

import test_linglu_w8_cpu as C
from test_linglu_w8_cpu import BF16, F16, F32, I8, U8
from torchlsq import _linglu_w8_host as HOST
from torchlsq import extension as E
from w8_routes import entered

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS = torch.ops.torchlsq
SYMBOL = "lsq_linglu_w8"                    # the library's one launch


def _big_c():
    return 16 * (torch.cuda.get_device_properties(0).multi_processor_count + 1)     # the persistent loop's second pass


# (M, C, K, x, weight, gate / up / product levels unsigned, mid_dtype, bias, function, activation quantizer, fused); C = 0 stands for
# 16 (CUs + 1).  K: 16 less than one wave's step, 272 a partial step and idle waves, 4096 resident, 4112 restaged per tile; C: 16 one
# tile, 40 a tail tile, clamped rows, byte stores and an up strip that starts at weight row 40.  (A case needs some hundred outputs
# to meet requant_w8_cases' condition: M = 1 goes with the widest C.)
# The last four rows: K = 8208 is a first, a middle and a last chunk of 16 k with 15 idle waves, K = 12288 three full chunks, and
# (3, 0, 4112) has a workgroup's second tile restage x chunk by chunk.
CASES = [(16, 16, 16, U8, I8, True, True, True, BF16, "f32", "silu", False, True),
         (3, 40, 16, U8, I8, True, True, True, F32, "f32", "silu", False, True),
         (16, 48, 16, I8, U8, False, True, False, BF16, None, "gelu_tanh", True, False),
         (3, 40, 272, U8, I8, True, True, True, F32, "f32", "silu", False, True),
         (16, 40, 272, I8, U8, False, False, False, BF16, "f32", "gelu_tanh", False, False),
         (16, 48, 272, U8, I8, True, False, True, F16, None, "silu", True, True),
         (16, 16, 4096, U8, I8, True, True, True, BF16, "f32", "silu", False, True),
         (3, 40, 4096, U8, I8, True, False, True, BF16, "f32", "gelu_tanh", True, False),
         (16, 48, 4096, U8, U8, False, True, False, F16, "f32", "silu", False, True),
         (16, 16, 4112, U8, I8, True, False, True, F16, "f32", "silu", True, False),
         (3, 40, 4112, U8, I8, True, True, True, F32, None, "silu", False, True),
         (16, 48, 4112, I8, I8, False, False, True, BF16, "f32", "gelu_tanh", False, False),
         (1, 0, 64, U8, I8, True, True, True, BF16, "f32", "silu", False, True),
         (16, 0, 64, U8, I8, True, False, False, BF16, "f32", "silu", True, False),
         (3, 0, 64, I8, U8, False, False, True, F16, None, "gelu_tanh", False, True),
         (1, 0, 64, U8, I8, True, True, True, F32, "f32", "gelu_tanh", True, False),
         (3, 40, 8208, U8, I8, True, True, True, BF16, "f32", "silu", False, True),
         (16, 16, 12288, U8, I8, True, False, True, F32, "f32", "silu", False, False),
         (16, 48, 12288, I8, U8, False, True, False, BF16, None, "gelu_tanh", True, True),
         (3, 0, 4112, U8, I8, True, True, True, BF16, "f32", "silu", False, True)]


def _case(spec):
    spec = list(spec)
    spec[1] = spec[1] or _big_c()
    return C.case(*spec)


def _run(c, out=None, rows=None):
    """the one-launch route on the case's operands (`rows`: on those rows of x alone), held to ONE entry into liblsq_hip_linglu_w8.so:
    the comparison below it is on that kernel's bytes"""
    a = list(C.args_of(c, DEV))
    if rows is not None:
        a[0] = a[0][rows].contiguous()
    return _entered_once(a, out)


def _entered_once(args, out=None):
    with entered(HOST) as names:
        got = E.linglu_w8_q(*args, out=out)
    assert names == [SYMBOL], names
    return got


def _two_launches(c):
    """the route of before, which never enters that library"""
    with entered(HOST) as names:
        old = C.two_launches(C.args_of(c, DEV))
    assert names == [], names
    return old


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "-".join(str(v).replace("torch.", "") for v in s))
def test_bytes_equal_the_reference_and_the_two_launches(spec):
    _assert_bytes(_case(spec), spec[2])


def _assert_bytes(c, K):
    M, Cn = c["want"].shape
    assert E.linglu_w8_plan(M, Cn, K)["served"]
    got, old, again = _run(c), _two_launches(c), _run(c)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), c["want"]) and torch.equal(got, old) and torch.equal(got, again)
    if M > 1:           # a row's bytes depend on that row alone
        assert torch.equal(_run(c, rows=slice(1, 2)).cpu(), c["want"][1:2])


def test_longest_k_with_border_levels():
    """K = 65536, M = C = 16: tests/test_linglu_w8_cpu.py's `extreme_case`, 16 chunks"""
    assert E.linglu_w8_plan(16, 16, 65536)["chunks"] == 16
    _assert_bytes(C.extreme_case(), 65536)


def test_rows_on_either_side_of_the_lds_opt_in():
    """K = 4096: the largest M whose plan stays within the 64 KB a kernel has without the opt-in, and the first M beyond them"""
    below = max(M for M in range(1, 17) if E.linglu_w8_plan(M, 40, 4096)["lds_bytes"] <= 65536)
    assert below == 6 and E.linglu_w8_plan(below + 1, 40, 4096)["lds_bytes"] > 65536
    for M in (below, below + 1):
        _assert_bytes(C.case(M, 40, 4096), 4096)


def test_odd_byte_offset_and_guard_bytes():
    """y at an odd byte offset inside a larger buffer (byte stores, also where C % 16 == 0); the guard bytes stay as they were"""
    for spec in (CASES[3], CASES[8]):
        c = C.case(*spec)
        M, Cn = c["want"].shape
        buf = torch.full((M * Cn + 64,), 0x5A, dtype=c["want"].dtype, device=DEV)
        pl = E.linglu_w8_plan(M, Cn, spec[2], True, False)          # the call's own alignment: y at 31
        assert pl["served"] and pl["store"] == "bytes" and buf[31:].data_ptr() % 16 == 15
        _run(c, out=buf[31:31 + M * Cn].view(M, Cn))
        torch.cuda.synchronize()
        assert torch.equal(buf[31:31 + M * Cn].view(M, Cn).cpu(), c["want"])
        assert bool((buf[:31] == 0x5A).all()) and bool((buf[31 + M * Cn:] == 0x5A).all())


def test_a_call_in_a_graph():
    c = C.case(*CASES[11])
    args = C.args_of(c, DEV)                        # nothing is copied to the device during the capture
    eager = _entered_once(args)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _entered_once(args, out)                    # warm-up: the LDS opt-in is not captured
        out.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            held = _entered_once(args, out)         # the capture enters the library once
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(held.cpu(), c["want"]) and torch.equal(out, eager)


@pytest.mark.parametrize("which", [3, 13], ids=["gate", "up"])
def test_a_weight_at_an_odd_byte_offset_takes_the_two_launches(which):
    """the control of `entered`: dense weight levels that start at an odd byte of a larger buffer are not served, so the call runs
    the ops it composes -- no entry into this library -- and its bytes are the reference's all the same, also in an `out` at an odd
    byte offset, whose guard bytes stay as they were"""
    c = C.case(*CASES[4])
    M, Cn = c["want"].shape
    ybuf = torch.full((M * Cn + 64,), 0x5A, dtype=c["want"].dtype, device=DEV)
    out = ybuf[31:31 + M * Cn].view(M, Cn)
    a = list(C.args_of(c, DEV))
    buf = torch.zeros(a[which].numel() + 32, dtype=a[which].dtype, device=DEV)
    a[which] = buf[17:17 + a[which].numel()].view(a[which].shape).copy_(a[which])
    assert a[which].is_contiguous() and a[which].data_ptr() % 16 == 1
    with entered(HOST) as names:
        got = E.linglu_w8_q(*a)
        held = E.linglu_w8_q(*a, out=out)
    torch.cuda.synchronize()
    assert names == [] and torch.equal(got.cpu(), c["want"])
    assert held.data_ptr() == out.data_ptr() and torch.equal(out.cpu(), c["want"])
    assert bool((ybuf[:31] == 0x5A).all()) and bool((ybuf[31 + M * Cn:] == 0x5A).all())


def test_decode_steps_of_the_llama_layer():
    """tests/decoder_glu_w8_cases.py's layer, prompt then single-token steps.  Its `run` calls the MLP's children one by one, so at
    every call the layer's MLP with glu_epilogue=True is run on that call's n2 and add1: the product it hands to the down projection
    and its output hold the bytes of the stages h and out of the glu_epilogue=False run, which holds the CPU run's"""
    import decoder_glu_w8_cases as L
    from torchlsq.functional import LevelsTensor
    mid, name = torch.bfloat16, "short"
    xl = L.input_levels(name)
    xg = LevelsTensor(xl.levels.to(DEV), xl.scale.to(DEV), xl.zero_point.to(DEV), xl.quant_min, xl.quant_max)
    layer = copy.deepcopy(L.chain(name, mid)).to(DEV)
    layer.mlp.glu_epilogue = False
    mlp, seen, taken = copy.deepcopy(layer.mlp), [], []
    mlp.glu_epilogue = True
    mlp.down.register_forward_pre_hook(lambda mod, a: seen.append(a[0].levels))
    mlp._product_in_epilogue = lambda x, f=mlp._product_in_epilogue: taken.append(1) or f(x)

    def each(T, start, mids):
        out = mlp(mids["n2"], mids["add1"])
        assert torch.equal(seen[-1], mids["h"].levels) and torch.equal(out.levels, mids["out"].levels), (T, start)

    with torch.no_grad():
        got = L.sequence(layer, xg, L.make_cache(name, "dense", DEV), L.chunks_of(name, "steps"), each=each)
    assert L.CASES[name]["B"] <= 16 and len(taken) >= L.CASES[name]["steps"] >= 1
    assert L.differing(got, L.cpu_run(name, mid, "steps")) == []
