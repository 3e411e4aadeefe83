"""A whole decoder layer on 8-bit levels on the CPU path (tests/decoder_w8_cases.py): the ops fed each other's outputs -- a norm's levels
into the fused qkv projection, its strided q, k and v views into rope, the cache append and attention, the [B, T, H D] context into a
projection that adds the residual levels --, the layer run as one prompt, as a prompt and steps and token by token on the dense, the
split and the paged cache routes, bit for bit, and the `mid_dtype=float32` layer held to a plain float64 model of it: no level further
than 1, at most 0.1 % of a stage's levels different.  Runs without a GPU.
"""
import copy

import pytest
import torch

import decoder_w8_cases as L

NAMES = tuple(L.CASES)


def _mid_id(mid):
    return str(mid).replace("torch.", "")


@pytest.mark.parametrize("name", NAMES)
def test_every_stage_holds_more_than_64_distinct_levels(name):
    """a calibration that left a stage a handful of levels would make every comparison below vacuous"""
    for mid in L.MIDS:
        got = L.cpu_run(name, mid)
        c = L.CASES[name]
        assert got["out"].shape == (c["B"], L.total(c), c["d"]) and got["k"].shape == (c["B"], c["Hkv"], L.total(c), c["D"])
        for s in L.STAGES + L.CACHED:
            assert len(got[s].unique()) > 64, (name, _mid_id(mid), s, len(got[s].unique()))


def test_the_heads_are_views_of_the_qkv_bytes():
    from torchlsq.functional import LevelsTensor
    lv = torch.arange(2 * 3 * 8 * 16, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(2, 3, 8 * 16)
    qkv = LevelsTensor(lv, torch.tensor([0.1]), torch.tensor([7], dtype=torch.int32), 0, 255)
    q, k, v = L.heads(qkv, 4, 2, 16)
    assert q.shape == (2, 3, 4, 16) and k.shape == v.shape == (2, 3, 2, 16) and q.levels.stride() == (3 * 128, 128, 16, 1)
    assert all(t.levels.untyped_storage().data_ptr() == lv.untyped_storage().data_ptr() for t in (q, k, v))
    assert torch.equal(torch.cat([t.levels.reshape(2, 3, -1) for t in (q, k, v)], -1), lv)
    assert v.zero_point.data_ptr() == qkv.zero_point.data_ptr() and v.scale.data_ptr() == qkv.scale.data_ptr()


# (the whole prompt on the dense cache is the run every other one is compared with)
HOW_ROUTE = [(how, route) for how in ("whole", "steps", "tokens") for route in L.ROUTES if (how, route) != ("whole", "dense")]


@pytest.mark.parametrize("mid", L.MIDS, ids=_mid_id)
@pytest.mark.parametrize("how,route", HOW_ROUTE)
@pytest.mark.parametrize("name", NAMES)
def test_one_prompt_equals_prompt_and_steps_equals_token_by_token(name, how, route, mid):
    """every stage of every call, and the cache (a paged pool gathered through its table), against the rows of the whole prompt on the
    dense cache.  A prompt runs the linears at B T rows and a step at B rows, a prompt runs the prefill route and a step the decode,
    split or paged one: the per-row ops promise row independence and the attention routes equal bytes."""
    want, got = L.cpu_run(name, mid), L.cpu_run(name, mid, how, route)
    assert L.differing(got, want) == [], (name, how, route, _mid_id(mid))


@pytest.mark.parametrize("name", NAMES)
def test_a_batch_entry_alone(name):
    """B = 1: the linears at T rows and at one row"""
    c = L.CASES[name]
    want = L.cpu_run(name, L.BF16)
    xl = L.input_levels(name)
    one = L.with_levels(xl, xl.levels[1:2].contiguous())
    got = L.sequence(copy.deepcopy(L.chain(name, L.BF16)), one, L.make_cache(name, "paged", B=1), L.chunks_of(name, "steps"), "paged")
    assert all(torch.equal(got[s], want[s][1:2]) for s in L.STAGES + L.CACHED)
    assert got["out"].shape == (1, L.total(c), c["d"])


@pytest.mark.parametrize("name", NAMES)
def test_float32_against_the_float64_reference(name):
    """free running, every stage: the measured shares stand in decoder_w8_cases.py's docstring"""
    L.assert_close_to_reference(L.cpu_run(name, L.F32), name, "float32, CPU path")


@pytest.mark.parametrize("mid", (L.BF16, L.F16), ids=_mid_id)
@pytest.mark.parametrize("name", NAMES)
def test_bfloat16_and_float16_against_the_float64_reference_are_printed(name, mid):
    """between two quantizers the definition rounds to `mid_dtype`, which is not real arithmetic: the shares are printed (pytest -s),
    nothing is asserted about them"""
    res = L.distance(L.cpu_run(name, mid), name)
    print("%s %s, CPU path, against float64: %s" % (name, _mid_id(mid), L.distance_line(res)))
    assert set(res) == set(L.STAGES + L.CACHED)


def test_the_reference_notices_a_level():
    """the comparison is not blind: one level added to one row of one stage is a distance of 1 and a share above the cap"""
    got = dict(L.cpu_run("short", L.F32))
    got["fc1"] = got["fc1"].clone()
    got["fc1"][0, 3] += 1
    with pytest.raises(AssertionError, match="fc1"):
        L.assert_close_to_reference(got, "short", "one row off by one")
