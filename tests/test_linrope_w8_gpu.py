"""liblsq_hip_linrope_w8.so on the GPU: every byte against the plain reference of tests/test_linrope_w8_cpu.py, against the four-launch
composition on the same operands and against a second launch.  No tolerance anywhere."""
import copy

import pytest
import torch

import test_linrope_w8_cpu as C
from test_linrope_w8_cpu import BF16, F16, F32, FILL, I8, U8
from torchlsq import _linrope_w8_host as HOST
from torchlsq import extension as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, T, H, Hkv, D, R, K, x, weight, qkv / rot levels unsigned, mid_dtype, bias, paged, shift); H = 0 stands for CUs - 1: CUs + 1 items,
# the persistent loop's second pass.  K: 16 less than one wave's step, 272 a partial step and idle waves, 4096 resident, 4112 restaged
# per item.  (H, Hkv, D, R): (2, 1, 32, 32) one ROTATE item per head, (2, 2, 64, 32) ROTATE + PASS items and v strips that start
# mid-weight, (4, 1, 128, 128).  (A case needs some hundred rotated outputs to meet requant_w8_cases' condition: M = 1 goes with the
# widest shapes.)  paged: (page size, page_major); rows 5 and 6 of a 16-row paged case have the entries -1 and Np + 1.
CASES = [(16, 1, 2, 1, 32, 32, 16, U8, I8, True, True, BF16, "f32", None, 0),
         (3, 1, 2, 2, 64, 32, 16, I8, U8, False, True, F32, None, None, 1),
         (2, 3, 2, 2, 64, 32, 272, U8, I8, True, True, F32, "f32", None, 1),
         (16, 1, 4, 1, 128, 128, 272, I8, U8, False, False, BF16, "f32", None, 0),
         (3, 1, 2, 1, 32, 32, 272, U8, I8, True, False, F16, None, None, 2),
         (1, 1, 4, 1, 128, 128, 4096, U8, I8, True, True, BF16, "f32", None, 0),
         (2, 3, 2, 2, 64, 32, 4096, U8, U8, False, True, F16, "f32", None, 3),
         (16, 1, 2, 1, 32, 32, 4096, U8, I8, True, True, BF16, None, None, 0),
         (16, 1, 2, 2, 64, 32, 4112, U8, I8, True, False, F16, "f32", None, 0),
         (3, 1, 4, 1, 128, 128, 4112, I8, I8, False, True, F32, None, None, 1),
         (2, 3, 2, 1, 32, 32, 4112, U8, I8, True, True, BF16, "f32", None, 1),
         (1, 1, 0, 1, 32, 32, 64, U8, I8, True, True, BF16, "f32", None, 0),
         (16, 1, 0, 1, 32, 32, 64, U8, I8, True, False, BF16, None, None, 0),
         (3, 1, 0, 1, 32, 32, 64, I8, U8, False, True, F16, "f32", None, 1),
         (16, 1, 2, 1, 32, 32, 272, U8, I8, True, True, BF16, "f32", (16, True), 0),
         (16, 1, 2, 2, 64, 32, 4096, I8, U8, False, False, F16, None, (16, False), 0),
         (16, 1, 2, 2, 64, 32, 16, U8, I8, True, True, F32, "f32", (1, True), 0),
         (2, 3, 4, 1, 128, 128, 4112, U8, I8, True, False, BF16, "f32", (1, False), 1)]


def _case(spec):
    spec = list(spec)
    spec[2] = spec[2] or torch.cuda.get_device_properties(0).multi_processor_count - 1
    return C.case(*spec)


def _four_launches(*a, out):
    """the route of before: lsq_linear_w8_q8_dec_q, lsq_rope_w8 on q, and the dense or the paged append of k and v"""
    return HOST._composed(*a[:3], a[3:7], a[7:13], *a[13:17], a[17:23], a[23], a[24], a[25], int(a[26].shape[3]), *a[26:30], out)


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "-".join(str(v).replace("torch.", "") for v in s))
def test_bytes_equal_the_reference_and_the_four_launches(spec):
    c = _case(spec)
    B, T, H, Hkv, D = c["dims"]
    kw = dict(pages=(c["want"][1].shape[0], spec[13][0], C.TMAX // spec[13][0])) if spec[13] else dict(Tmax=C.TMAX)
    assert E.linrope_w8_plan(B, T, H, Hkv, D, spec[6], R=spec[5], P=C.P, **kw)["served"]
    got, old, again = C.call(c, DEV), C.call(c, DEV, fn=_four_launches), C.call(c, DEV)
    torch.cuda.synchronize()
    for g, o, a, w in zip(got[:3], old[:3], again[:3], c["want"]):
        assert torch.equal(g.cpu(), w) and torch.equal(g, o) and torch.equal(g, a)      # skipped rows and untouched pages keep FILL
    assert all(bool((t == FILL).all()) for t in got[3])
    if B * T > 1:           # a row's bytes depend on that row alone
        C.assert_row(c, DEV, 1 // T, 1 % T)


def test_a_call_in_a_graph():
    c = _case(CASES[8])
    made = C.call(c, DEV)[4]                        # the warm-up: the LDS opt-in is not captured, nothing is copied during the capture
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            C.call(c, DEV, made=made)
        for _ in range(3):
            for t in made[2]:
                t.fill_(FILL)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(g.cpu(), w) for g, w in zip(made[1], c["want"]))


@pytest.mark.parametrize("route", ["dense", "paged"])
def test_decode_steps_of_the_llama_layer(route):
    """tests/decoder_glu_w8_cases.py's layer, prompt then single-token steps.  At every call a QKVRotaryW8Q of the layer's own qkv and
    rot with rope_epilogue=True runs on that call's n1 and a copy of the cache from before the call: its rq and its cache hold the
    bytes of the unfused run, which holds the CPU run's"""
    import decoder_glu_w8_cases as L
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import QKVRotaryW8Q
    mid, name = torch.bfloat16, "short"
    xl = L.input_levels(name)
    xg = LevelsTensor(xl.levels.to(DEV), xl.scale.to(DEV), xl.zero_point.to(DEV), xl.quant_min, xl.quant_max)
    layer = copy.deepcopy(L.chain(name, mid)).to(DEV)
    mod, taken = QKVRotaryW8Q(layer.qkv, layer.rot, layer.H, layer.Hkv, rope_epilogue=True), []
    mod._in_epilogue = lambda x, cache, f=mod._in_epilogue: taken.append(int(x.shape[1])) or f(x, cache)
    cache = L.make_cache(name, route, DEV)
    before = [copy.deepcopy(cache)]

    def each(T, start, mids):
        rq, kl, vl, lens = mod(mids["n1"], before[0])
        assert torch.equal(rq.levels, mids["rq"].levels) and torch.equal(kl.levels, mids["k_cache"].levels), (T, start)
        assert torch.equal(vl.levels, mids["v_cache"].levels) and torch.equal(lens, cache.lengths), (T, start)
        before[0] = copy.deepcopy(cache)

    with torch.no_grad():
        got = L.sequence(layer, xg, cache, L.chunks_of(name, "steps"), route, each=each)
    assert taken == [1] * L.CASES[name]["steps"] and L.CASES[name]["steps"] >= 1
    assert L.differing(got, L.cpu_run(name, mid, "steps", route)) == []
