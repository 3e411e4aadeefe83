"""A whole LLAMA layer on 8-bit levels on the CPU path (tests/decoder_glu_w8_cases.py): the decoder layer of
tests/decoder_w8_cases.py with the gated MLP -- ONE fused gate_up linear, SiLU(gate) * up on its halves in place, the down projection
with the residual -- run as one prompt, as a prompt and steps and token by token on the dense, the split and the paged cache routes,
bit for bit, and the `mid_dtype=float32` layer held to a plain float64 model of it under decoder_w8_cases' own condition: no level
further than 1, at most 0.1 % of a stage's levels different.  Runs without a GPU.
"""
import copy

import pytest
import torch

import decoder_glu_w8_cases as L

NAMES = tuple(L.CASES)


def _mid_id(mid):
    return str(mid).replace("torch.", "")


@pytest.mark.parametrize("name", NAMES)
def test_every_stage_holds_more_than_64_distinct_levels(name):
    """a calibration that left a stage a handful of levels would make every comparison below vacuous"""
    for mid in L.MIDS:
        got = L.cpu_run(name, mid)
        c = L.CASES[name]
        assert got["out"].shape == (c["B"], L.total(c), c["d"]) and got["gu"].shape == (c["B"], L.total(c), 2 * c["hidden"])
        assert got["h"].shape == (c["B"], L.total(c), c["hidden"])
        for s in L.STAGES + L.CACHED:
            assert len(got[s].unique()) > 64, (name, _mid_id(mid), s, len(got[s].unique()))
        # the gates reach both bends of the SiLU: a good share of them below -1 and above 1
        _, qs, _ = L.fitted(name)
        scale, zero, _, _ = L.D.site(qs["gu"])
        gate = (got["gu"][..., :c["hidden"]].double() - zero) * scale
        assert float((gate < -1).double().mean()) > 0.05 and float((gate > 1).double().mean()) > 0.05, name


def test_the_product_reads_the_halves_of_the_fused_output_in_place():
    from torchlsq import extension as E
    name = "short"
    c = L.CASES[name]
    layer = copy.deepcopy(L.chain(name, L.F32))
    xl = L.input_levels(name)
    seen = []
    L.sequence(layer, xl, L.make_cache(name, "dense"), L.chunks_of(name, "whole"), each=lambda T, start, mids: seen.append(mids))
    m = seen[0]
    gu, h = m["gu"], m["h"]
    B, T, hidden = c["B"], L.total(c), c["hidden"]
    assert gu.levels.shape == (B, T, 2 * hidden) and gu.levels.is_contiguous() and h.levels.shape == (B, T, hidden)
    gate, up = gu.levels[..., :hidden], gu.levels[..., hidden:]
    assert up.data_ptr() == gate.data_ptr() + hidden and gate.stride() == (T * 2 * hidden, 2 * hidden, 1)
    assert E.glu_w8_plan(B * T, hidden, 2 * hidden, 2 * hidden)["family"] == "packets"
    # the module on the fused output, on the two views and on dense copies: the same bytes; and the whole MLP in one call
    glu = layer.mlp.glu
    assert torch.equal(glu(gu).levels, h.levels)
    assert torch.equal(glu(L.with_levels(gu, gate), L.with_levels(gu, up)).levels, h.levels)
    assert torch.equal(glu(L.with_levels(gu, gate.contiguous()), L.with_levels(gu, up.contiguous())).levels, h.levels)
    assert torch.equal(layer.mlp(m["n2"], m["add1"]).levels, m["out"].levels)
    # the existing ops composed, with no quantizer between the SiLU and the product
    t = torch.nn.functional.silu(L.with_levels(gu, gate).dequantize(L.F32)) * L.with_levels(gu, up).dequantize(L.F32)
    want = torch.ops.torchlsq.lsq_levels_per_tensor(t, glu.output_scale, glu.output_shift, *glu.output_range, 0).view(torch.uint8)
    assert torch.equal(h.levels, want)


# (the whole prompt on the dense cache is the run every other one is compared with)
HOW_ROUTE = [(how, route) for how in ("whole", "steps", "tokens") for route in L.ROUTES if (how, route) != ("whole", "dense")]


@pytest.mark.parametrize("mid", L.MIDS, ids=_mid_id)
@pytest.mark.parametrize("how,route", HOW_ROUTE)
@pytest.mark.parametrize("name", NAMES)
def test_one_prompt_equals_prompt_and_steps_equals_token_by_token(name, how, route, mid):
    """every stage of every call, and the cache, against the rows of the whole prompt on the dense cache: the gated product at B T
    rows and at B rows (a step) promises row independence like the other per-row ops"""
    want, got = L.cpu_run(name, mid), L.cpu_run(name, mid, how, route)
    assert L.differing(got, want) == [], (name, how, route, _mid_id(mid))


@pytest.mark.parametrize("name", NAMES)
def test_float32_against_the_float64_reference(name):
    """free running, every stage: the measured shares stand in decoder_glu_w8_cases.py's docstring"""
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
    """the comparison is not blind: one level added to one row of the product is a distance of 1 and a share above the cap"""
    got = dict(L.cpu_run("short", L.F32))
    got["h"] = got["h"].clone()
    got["h"][0, 3] += 1
    with pytest.raises(AssertionError, match="'h'"):
        L.assert_close_to_reference(got, "short", "one row off by one")
