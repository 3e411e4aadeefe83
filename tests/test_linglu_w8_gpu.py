"""liblsq_hip_linglu_w8.so on the GPU: every byte against the plain reference of tests/test_linglu_w8_cpu.py, against the two-launch
route on the same operands and against a second launch.  No tolerance anywhere."""
import copy

import pytest
import torch

import test_linglu_w8_cpu as C
from test_linglu_w8_cpu import BF16, F16, F32, I8, U8
from torchlsq import extension as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS = torch.ops.torchlsq


def _big_c():
    return 16 * (torch.cuda.get_device_properties(0).multi_processor_count + 1)     # the persistent loop's second pass


# (M, C, K, x, weight, gate / up / product levels unsigned, mid_dtype, bias, function, activation quantizer, fused); C = 0 stands for
# 16 (CUs + 1).  K: 16 less than one wave's step, 272 a partial step and idle waves, 4096 resident, 4112 restaged per tile; C: 16 one
# tile, 40 a tail tile, clamped rows, byte stores and an up strip that starts at weight row 40.  (A case needs some hundred outputs
# to meet requant_w8_cases' condition: M = 1 goes with the widest C.)
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
         (1, 0, 64, U8, I8, True, True, True, F32, "f32", "gelu_tanh", True, False)]


def _case(spec):
    spec = list(spec)
    spec[1] = spec[1] or _big_c()
    return C.case(*spec)


def _run(c, out=None, rows=None):
    """the one-launch route on the case's operands (`rows`: on those rows of x alone)"""
    a = list(C.args_of(c, DEV))
    if rows is not None:
        a[0] = a[0][rows].contiguous()
    return E.linglu_w8_q(*a, out=out)


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "-".join(str(v).replace("torch.", "") for v in s))
def test_bytes_equal_the_reference_and_the_two_launches(spec):
    c = _case(spec)
    M, Cn = c["want"].shape
    assert E.linglu_w8_plan(M, Cn, spec[2])["served"]
    got, old, again = _run(c), C.two_launches(C.args_of(c, DEV)), _run(c)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), c["want"]) and torch.equal(got, old) and torch.equal(got, again)
    if M > 1:           # a row's bytes depend on that row alone
        assert torch.equal(_run(c, rows=slice(1, 2)).cpu(), c["want"][1:2])


def test_odd_byte_offset_and_guard_bytes():
    """y at an odd byte offset inside a larger buffer (byte stores); the guard bytes stay as they were"""
    c = C.case(*CASES[3])
    M, Cn = c["want"].shape
    buf = torch.full((M * Cn + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    _run(c, out=buf[31:31 + M * Cn].view(M, Cn))
    torch.cuda.synchronize()
    assert torch.equal(buf[31:31 + M * Cn].view(M, Cn).cpu(), c["want"])
    assert bool((buf[:31] == 0x5A).all()) and bool((buf[31 + M * Cn:] == 0x5A).all())


def test_a_call_in_a_graph():
    c = C.case(*CASES[11])
    args = C.args_of(c, DEV)                        # nothing is copied to the device during the capture
    eager = E.linglu_w8_q(*args)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        E.linglu_w8_q(*args, out=out)               # warm-up: the LDS opt-in is not captured
        out.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            held = E.linglu_w8_q(*args, out=out)
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(held.cpu(), c["want"]) and torch.equal(out, eager)


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
