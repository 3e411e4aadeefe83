"""liblsq_hip_linrope_w8.so on the GPU: every byte against the plain reference of tests/test_linrope_w8_cpu.py, against the four-launch
composition on the same operands and against a second launch.  No tolerance anywhere."""
import copy

import pytest
import torch

import test_linrope_w8_cpu as C
from test_linrope_w8_cpu import BF16, F16, F32, FILL, I8, U8
from torchlsq import _linrope_w8_host as HOST
from torchlsq import extension as E
from w8_routes import entered

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SYMBOL = "lsq_linrope_w8"                   # the library's one launch

# (B, T, H, Hkv, D, R, K, x, weight, qkv / rot levels unsigned, mid_dtype, bias, paged, shift); H = 0 stands for CUs - 1: CUs + 1 items,
# the persistent loop's second pass.  K: 16 less than one wave's step, 272 a partial step and idle waves, 4096 resident, 4112 restaged
# per item.  (H, Hkv, D, R): (2, 1, 32, 32) one ROTATE item per head, (2, 2, 64, 32) ROTATE + PASS items and v strips that start
# mid-weight, (4, 1, 128, 128).  (A case needs some hundred rotated outputs to meet requant_w8_cases' condition: M = 1 goes with the
# widest shapes.)  paged: (page size, page_major); rows 5 and 6 of a 16-row paged case have the entries -1 and Np + 1.
# The last six rows: K = 8208 is a first, a middle and a last chunk of 16 k with 15 idle waves, K = 12288 three full chunks, (3, 1, 0)
# at K = 4112 has a workgroup's second item restage x chunk by chunk, and B = 6 and 7 at K = 4096 lie on either side of the 64 KB of
# LDS a kernel has without the opt-in.  Behind them tests/test_linrope_w8_cpu.py's LAYOUT_CASES, which have a 16th entry, the layout.
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
         (2, 3, 4, 1, 128, 128, 4112, U8, I8, True, False, BF16, "f32", (1, False), 1),
         (2, 3, 2, 2, 64, 32, 8208, U8, I8, True, True, BF16, "f32", None, 1),
         (2, 3, 2, 2, 64, 32, 8208, U8, I8, True, False, F32, None, (1, False), 1),
         (16, 1, 2, 1, 32, 32, 12288, U8, I8, True, True, BF16, "f32", None, 0),
         (3, 1, 0, 1, 32, 32, 4112, U8, I8, True, True, BF16, "f32", None, 1),
         (6, 1, 2, 2, 64, 32, 4096, U8, I8, True, True, BF16, "f32", None, 0),
         (7, 1, 2, 2, 64, 32, 4096, U8, I8, True, True, BF16, "f32", None, 0)] + C.LAYOUT_CASES


def _case(spec):
    spec = list(spec)
    spec[2] = spec[2] or torch.cuda.get_device_properties(0).multi_processor_count - 1
    return C.case(*spec)


def _four_launches(*a, out):
    """the route of before: lsq_linear_w8_q8_dec_q, lsq_rope_w8 on q, and the dense or the paged append of k and v; it never enters
    liblsq_hip_linrope_w8.so"""
    with entered(HOST) as names:
        rq = HOST._composed(*a[:3], a[3:7], a[7:13], *a[13:17], a[17:23], a[23], a[24], a[25], int(a[26].shape[3]), *a[26:30], out)
    assert names == [], names
    return rq


def _one_launch(*a, out):
    """the op, held to ONE entry into liblsq_hip_linrope_w8.so: the comparison below it is on that kernel's bytes"""
    with entered(HOST) as names:
        rq = E.linrope_w8_q(*a, out=out)
    assert names == [SYMBOL], names
    return rq


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "-".join(str(v).replace("torch.", "") for v in s))
def test_bytes_equal_the_reference_and_the_four_launches(spec):
    _assert_bytes(_case(spec), spec[6], spec[5])


def _assert_bytes(c, K, Rd):
    B, T, H, Hkv, D = c["dims"]
    kw = dict(pages=(c["want"][1].shape[0], c["paged"][0], C.TMAX // c["paged"][0])) if c["paged"] else dict(Tmax=C.TMAX)
    assert E.linrope_w8_plan(B, T, H, Hkv, D, K, R=Rd, P=C.P, **kw)["served"]
    got, old, again = C.call(c, DEV, fn=_one_launch), C.call(c, DEV, fn=_four_launches), C.call(c, DEV, fn=_one_launch)
    torch.cuda.synchronize()
    rq, kc, vc = got[4][1]              # the plan of the call that was made: the destinations' own strides and alignment
    own = dict(q_strides=HOST._strides(rq, (0, 1, 2)), k_strides=HOST._strides(kc, (0, 2, 1)), v_strides=HOST._strides(vc, (0, 2, 1)),
               aligned=all(t.data_ptr() % 16 == 0 for t in (rq, kc, vc)))
    assert E.linrope_w8_plan(B, T, H, Hkv, D, K, R=Rd, P=C.P, **kw, **own)["served"]
    if c["layout"] == "rq_padded":
        assert own["q_strides"][2] == D + 16
    if c["layout"] == "token_major":
        assert own["k_strides"] == (C.TMAX * Hkv * D, Hkv * D, D)
    for g, o, a, w in zip(got[:3], old[:3], again[:3], c["want"]):
        assert torch.equal(g.cpu(), w) and torch.equal(g, o) and torch.equal(g, a)      # skipped rows and untouched pages keep FILL
    assert all(bool((t == FILL).all()) for run in (got, old, again) for t in run[3])
    if B * T > 1:           # a row's bytes depend on that row alone
        C.assert_row(c, DEV, 1 // T, 1 % T, fn=_one_launch)


def test_lds_on_either_side_of_the_opt_in():
    """the rows B = 6 and B = 7 of CASES are what they are said to be"""
    assert E.linrope_w8_plan(6, 1, 2, 2, 64, 4096, R=32, P=C.P, Tmax=C.TMAX)["lds_bytes"] == 37376 + 6 * 4112 <= 65536
    assert E.linrope_w8_plan(7, 1, 2, 2, 64, 4096, R=32, P=C.P, Tmax=C.TMAX)["lds_bytes"] == 37376 + 7 * 4112 > 65536


@pytest.mark.parametrize("paged", [None, (16, True)], ids=["dense", "paged"])
def test_longest_k_with_border_levels(paged):
    """K = 65536: tests/test_linrope_w8_cpu.py's `extreme_case`, 16 chunks on a [96, 65536] weight"""
    assert E.linrope_w8_plan(16, 1, 1, 1, 32, 65536, P=C.P, Tmax=C.TMAX)["chunks"] == 16
    _assert_bytes(C.extreme_case(paged), 65536, 32)


def test_a_call_in_a_graph():
    c = _case(CASES[8])
    made = C.call(c, DEV, fn=_one_launch)[4]        # the warm-up: the LDS opt-in is not captured, nothing is copied during the capture
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            C.call(c, DEV, fn=_one_launch, made=made)       # the capture enters the library once
        for _ in range(3):
            for t in made[2]:
                t.fill_(FILL)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(g.cpu(), w) for g, w in zip(made[1], c["want"]))


def test_a_weight_at_an_odd_byte_offset_takes_the_four_launches():
    """the control of `entered`: dense weight levels that start at an odd byte of a larger buffer are not served, so the call runs
    the ops it composes -- no entry into this library -- and the bytes of rq and of the caches are the reference's all the same"""
    c = _case(CASES[2])

    def shifted(*a, out):
        buf = torch.zeros(a[3].numel() + 32, dtype=a[3].dtype, device=DEV)
        odd = buf[17:17 + a[3].numel()].view(a[3].shape).copy_(a[3])
        assert odd.is_contiguous() and odd.data_ptr() % 16 == 1
        with entered(HOST) as names:
            rq = E.linrope_w8_q(*a[:3], odd, *a[4:], out=out)
        assert names == [], names
        return rq

    got = C.call(c, DEV, fn=shifted)
    torch.cuda.synchronize()
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got[:3], c["want"])) and all(bool((t == FILL).all()) for t in got[3])


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
