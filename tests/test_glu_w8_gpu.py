"""The gated product act(gate) * up on 8-bit levels on the GPU (liblsq_hip_glu_w8.so), bit for bit against the CPU path of the same
op for the SAME table (tests/test_glu_w8_cpu.py holds that path to the two compositions of existing ops and to a numpy restatement;
the table is built once on the CPU and moved): both kernel families, every layout, both sides of every threshold of the plan with
this device's compute units, guard bytes, repeatability, a captured graph, and the whole Llama layer of
tests/decoder_glu_w8_cases.py on the dense, split and paged routes.  No tolerance anywhere.
"""
import copy

import pytest
import torch

import glu_w8_cases as C

pytestmark = pytest.mark.gpu
OPS = torch.ops.torchlsq
DEV = "cuda:0"
one = C.one
OUTS = [(True, torch.float32), (False, torch.bfloat16), (None, torch.float16), (None, torch.float32), (True, torch.float16)]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _check(case, family, note=""):
    """the GPU's result of a case against the CPU path's; the plan's family for the pointers the device sees"""
    gate, up = C.operands(case, DEV)
    aligned = gate.levels.data_ptr() % 16 == 0 and up.levels.data_ptr() % 16 == 0
    pl = C.plan_of(case, aligned)
    assert pl == C.expected_plan(case["rows"], case["C"], case["gate"][2], case["up"][2], aligned, cus=_cus()), (note, pl)
    assert pl["family"] == family, (note, pl)
    want = C.run(case)
    got = C.run(case, DEV, ops=(gate, up))
    assert got.is_contiguous() and C.same(got, want), note
    return got, want


@pytest.mark.parametrize("Cn", (16, 48, 272))
@pytest.mark.parametrize("rows", (1, 3, 17))
def test_packets_family(rows, Cn):
    """C % 16 == 0 with row strides C (dense), 2 C (the halves of a fused buffer) and 2 C + 16 (a padded one)"""
    k = 0
    for layout in C.LAYOUTS:
        for pair in C.DTYPE_PAIRS:
            out = OUTS[k % len(OUTS)]
            case = C.glu_case(rows, Cn, pair, out, ("silu", "gelu", "sigmoid", "relu")[k % 4], k % 3 == 0, layout, (128, 3)[k % 2], seed=k)
            _check(case, "packets", (layout, pair, out))
            k += 1


@pytest.mark.parametrize("Cn", (1, 15, 17))
def test_generic_family(Cn):
    k = 0
    for rows in (1, 3, 17):
        for layout in ("dense", "halves", "odd_stride"):
            case = C.glu_case(rows, Cn, C.DTYPE_PAIRS[k % 4], OUTS[k % len(OUTS)], "silu", k % 2 == 0, layout, seed=k)
            _check(case, "generic", (rows, layout))
            k += 1


@pytest.mark.parametrize("layout", ("off_by_one", "odd_stride"))
def test_generic_family_serves_what_the_packets_cannot(layout):
    """C % 16 == 0, but a base one byte off a 16-byte boundary, or row strides that are no multiple of 16"""
    for k, (pair, out) in enumerate(zip(C.DTYPE_PAIRS, OUTS)):
        case = C.glu_case(17, 48, pair, out, "silu", k % 2 == 1, layout, seed=k)
        gate, up = C.operands(case, DEV)
        assert (gate.levels.data_ptr() % 16 == 1) == (layout == "off_by_one")
        _check(case, "generic", (layout, pair))


def test_thresholds_with_this_devices_compute_units():
    """one size on each side of the packets-per-lane threshold (2 workgroups per compute unit at 2 packets per lane) and of the family
    thresholds (C % 16, the alignment of a base, a row stride % 16), the reported plan asserted in each"""
    from torchlsq import extension as E
    edge = 2 * _cus() * 256 * 2 - 2 * 256 + 1            # the fewest packets with 2 * CUs workgroups at 2 packets per lane
    seen = set()
    for rows in (edge - 1, edge):
        case = C.glu_case(rows, 16, C.DTYPE_PAIRS[1], (True, torch.bfloat16), "silu", False, "halves", seed=rows % 7)
        pl = C.plan_of(case)
        assert pl["packets"] == rows and pl["grid"] == -(-rows // (256 * pl["packets_per_lane"]))
        seen.add(pl["packets_per_lane"])
        _check(case, "packets", rows)
    assert seen == {1, 2}
    for Cn, family in ((15, "generic"), (16, "packets"), (17, "generic"), (32, "packets")):
        _check(C.glu_case(33, Cn, layout="dense", seed=Cn), family, Cn)
    assert E.glu_w8_plan(33, 32, 64, 64, aligned=False)["family"] == "generic" and E.glu_w8_plan(33, 32, 64, 72)["family"] == "generic"
    assert E.glu_w8_plan(33, 32, 64, 80)["family"] == "packets"


@pytest.mark.parametrize("mid", C.MIDS, ids=C.name)
def test_all_65536_byte_pairs(mid):
    for k, pair in enumerate(C.DTYPE_PAIRS):
        for unsigned in (True, None):
            case = C.glu_case(256, 256, pair, (unsigned, mid), "silu", k % 2 == 1, "dense", exhaustive=True)
            got, _ = _check(case, "packets", (pair, unsigned))
            assert len(got.float().unique()) > 64


def test_special_values_of_the_table():
    case = C.glu_case(16, 16, (torch.uint8, torch.uint8), (True, torch.float32), "silu")
    case["table"] = case["table"].clone()
    case["table"][7], case["table"][8], case["table"][9] = float("nan"), float("inf"), float("-inf")
    gate, up = C.operands(case)
    for r, b in enumerate((7, 8, 9)):
        gate.levels[r, :] = b
    up.levels[:3, 0:4] = torch.tensor([130, 120, 128, 255], dtype=torch.uint8)
    for out in ((True, torch.float32), (False, torch.bfloat16), (None, torch.float32), (None, torch.float16)):
        c = dict(case, mid=out[1])
        if out[0] is None:
            c["rng"] = None
        elif not out[0]:
            c["rng"] = (-128, 127, -128, 127)
        got, want = _check(c, "packets", out)
        if out[0] is not None:
            assert got[0].tolist() == [c["rng"][0]] * 16                 # a NaN goes to quant_min
        else:
            assert bool(got[0].isnan().all())


@pytest.mark.parametrize("family", ("packets", "generic"))
def test_guard_bytes_and_padding(family):
    """bytes around y stay as they were; the bytes between the halves' rows never influence the result; the operands are only read"""
    from torchlsq._glu_w8_host import glu_w8, glu_w8_q
    rows, Cn = 17, (48 if family == "packets" else 47)
    for out, layout in (((True, torch.float32), "padded"), ((None, torch.bfloat16), "padded"), ((False, torch.float16), "halves")):
        case = C.glu_case(rows, Cn, C.DTYPE_PAIRS[2], out, "gelu", False, layout, seed=9)
        want = C.run(case)
        gate, up = C.operands(case, DEV)
        table = case["table"].to(DEV)
        size = want.element_size()
        for yo in ((0, 16) if family == "packets" else (0, size)):
            ybuf = torch.full((rows * Cn * size + 96,), 77, dtype=torch.uint8, device=DEV)
            yv = ybuf[32 + yo:32 + yo + rows * Cn * size].view(want.dtype).reshape(rows, Cn)
            before = [b.clone() for b in (gate.levels, up.levels)]
            if case["rng"] is None:
                got = glu_w8(gate.levels, up.levels, up.scale, up.zero_point, table, case["mid"], out=yv)
            else:
                got = glu_w8_q(gate.levels, up.levels, up.scale, up.zero_point, table, case["osc"].to(DEV), case["osh"].to(DEV), *case["rng"],
                               case["mid"], out=yv)
            assert got.data_ptr() == yv.data_ptr() and C.same(got, want), (out, layout, yo)
            guard = torch.cat([ybuf[:32 + yo], ybuf[32 + yo + rows * Cn * size:]])
            assert bool((guard == 77).all()), (out, layout, yo)
            assert torch.equal(before[0], gate.levels) and torch.equal(before[1], up.levels)
        # other bytes in the padding, the same result
        other = dict(case, bufs=[b.clone() for b in case["bufs"]])
        keep = torch.zeros_like(other["bufs"][0], dtype=torch.bool)
        for side in ("gate", "up"):
            C.view(keep, case[side], rows, Cn, torch.bool).fill_(True)
        other["bufs"][0][~keep] ^= 0xff
        assert C.same(C.run(other, DEV), want)


def test_row_offsets_beyond_32_bits():
    """the halves of a buffer whose row stride is 2^30 + 16: the third row lies beyond 2^31 bytes"""
    rows, Cn, ld = 3, 48, (1 << 30) + 16
    case = C.glu_case(rows, Cn, C.DTYPE_PAIRS[0], (True, torch.float32), "silu", False, "halves", seed=11)
    want = C.run(case)
    gate, up = C.operands(case)
    big = torch.empty((rows - 1) * ld + 2 * Cn, dtype=torch.uint8, device=DEV)
    bg, bu = big.as_strided((rows, Cn), (ld, 1), 0), big.as_strided((rows, Cn), (ld, 1), Cn)
    bg.copy_(gate.levels)
    bu.copy_(up.levels)
    from torchlsq import extension as E
    assert E.glu_w8_plan(rows, Cn, ld, ld)["family"] == "packets"
    got = OPS.lsq_glu_w8_q8_q(bg, bu, up.scale.to(DEV), up.zero_point.to(DEV), case["table"].to(DEV), case["osc"].to(DEV), case["osh"].to(DEV),
                              *case["rng"], case["mid"])
    assert C.same(got, want)


def test_equals_the_existing_gpu_ops_composed():
    """`lsq_lut_w8` + `lsq_mul_gate_w8_q` on dense copies, on the GPU, with the byte table built where the float table was"""
    for k, pair in enumerate(C.DTYPE_PAIRS):
        for out in ((True, torch.float32), (False, torch.bfloat16), (None, torch.float16)):
            case = C.glu_case(33, 272, pair, out, ("silu", "gelu_tanh")[k % 2], True, "halves", seed=k)
            got = C.run(case, DEV)
            assert C.same(got, C.composed_with_act_quantizer(case, DEV)), (pair, out)
            assert C.same(got, C.run(case)), (pair, out)


def test_launches_repeat_and_rows_are_independent():
    case = C.glu_case(257, 272, C.DTYPE_PAIRS[3], (True, torch.bfloat16), "silu", False, "padded", seed=4)
    gate, up = C.operands(case, DEV)
    first = C.run(case, DEV, ops=(gate, up))
    for _ in range(3):
        assert torch.equal(C.run(case, DEV, ops=(gate, up)), first)
    assert C.same(first, C.run(case))
    # a row of the result is the result of that row alone; a row changed changes that row alone
    from torchlsq.functional import LevelsTensor
    for r in (0, 100, 256):
        g1, u1 = (LevelsTensor(t.levels[r:r + 1], t.scale, t.zero_point, t.quant_min, t.quant_max) for t in (gate, up))
        assert torch.equal(C.run(case, DEV, ops=(g1, u1)), first[r:r + 1]), r
    gate.levels[100] = gate.levels[100].roll(1, 0)
    again = C.run(case, DEV, ops=(gate, up))
    assert not torch.equal(again[100], first[100])
    keep = torch.arange(257, device=DEV) != 100
    assert torch.equal(again[keep], first[keep])


@pytest.mark.parametrize("shared", (True, False), ids=("fused", "two_linears"))
def test_a_gated_mlp_in_a_graph(shared):
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import convert_w8a8_glu
    net, qs, x = C.mlp_block(shared=shared, d=64, hidden=96, rows=40)
    mlp = convert_w8a8_glu(net, {"mlp": C.mlp_quantizers(qs)}, mid_dtype=torch.bfloat16).mlp       # tables built on the CPU
    assert mlp.fused == shared
    xl = LevelsTensor.from_quantized(qs["in"].quantize(x))
    other = LevelsTensor.from_quantized(qs["in"].quantize(x.flip(0) * 0.5 + 0.1))
    want, want_other = mlp(xl, xl).levels, mlp(other, other).levels
    assert not torch.equal(want, want_other) and len(want.unique()) > 16
    gm = copy.deepcopy(mlp).to(DEV)
    static = LevelsTensor(xl.levels.to(DEV), xl.scale.to(DEV), xl.zero_point.to(DEV), xl.quant_min, xl.quant_max, xl.type_min, xl.type_max)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        assert torch.equal(gm(static, static).levels.cpu(), want)       # eager, and the warm-up of the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = gm(static, static).levels
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    static.levels.copy_(other.levels)                                   # new input bytes, the same graph
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want_other)
    if shared:                                                          # the product read the halves of the fused output in place
        gu = gm.gate_up(static)
        assert gu.levels.shape == (40, 192) and gm.glu(gu).levels.shape == (40, 96)


# ---------------------------------------------------------------------------------------------------
# the whole Llama layer (tests/decoder_glu_w8_cases.py) on the dense, split and paged routes against the CPU run's bytes
# ---------------------------------------------------------------------------------------------------
def _layer_sequence(name, mid, how, route):
    """(the GPU's levels of the sequence by stage, the plan families the gated product took by rows): the CPU-built layer moved, so its
    constants, tables and weights are those of the CPU run"""
    import decoder_glu_w8_cases as L
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor
    c = L.CASES[name]
    layer = copy.deepcopy(L.chain(name, mid)).to(DEV)
    xl = L.input_levels(name)
    xg = LevelsTensor(xl.levels.to(DEV), xl.scale.to(DEV), xl.zero_point.to(DEV), xl.quant_min, xl.quant_max)
    seen = set()

    def each(T, start, mids):
        gu, hidden = mids["gu"].levels, c["hidden"]
        assert gu.is_cuda and gu.shape == (c["B"], T, 2 * hidden) and gu.is_contiguous() and gu.data_ptr() % 16 == 0
        pl = E.glu_w8_plan(c["B"] * T, hidden, 2 * hidden, 2 * hidden, aligned=mids["h"].levels.data_ptr() % 16 == 0)
        assert pl["family"] == "packets", pl                    # the halves of the fused output, read in place
        seen.add(("step" if T == 1 else "prompt", pl["family"]))

    with torch.no_grad():
        got = L.sequence(layer, xg, L.make_cache(name, route, DEV), L.chunks_of(name, how), route, each=each)
    return got, seen


@pytest.mark.parametrize("mid", C.MIDS, ids=C.name)
@pytest.mark.parametrize("name", ("short", "long"))
def test_the_llama_layer_whole_prompt_against_the_cpu_run_and_float64(name, mid):
    import decoder_glu_w8_cases as L
    got, seen = _layer_sequence(name, mid, "whole", "dense")
    assert seen == {("prompt", "packets")}
    assert L.differing(got, L.cpu_run(name, mid)) == [], (name, mid)
    if mid == torch.float32:
        # a reference that is not the package: no level further than 1, at most 0.1 % of a stage's levels different
        L.assert_close_to_reference(got, name, "float32, GPU")


@pytest.mark.parametrize("route", ("dense", "split", "paged"))
@pytest.mark.parametrize("name", ("short", "long"))
def test_the_llama_layer_prompt_then_steps(name, route):
    import decoder_glu_w8_cases as L
    got, seen = _layer_sequence(name, torch.bfloat16, "steps", route)
    assert seen == {("prompt", "packets"), ("step", "packets")}
    assert L.differing(got, L.cpu_run(name, torch.bfloat16)) == [], (name, route)


@pytest.mark.parametrize("route", ("dense", "split", "paged"))
def test_the_llama_layer_token_by_token(route):
    import decoder_glu_w8_cases as L
    got, _ = _layer_sequence("short", torch.float16, "tokens", route)
    assert L.differing(got, L.cpu_run("short", torch.float16)) == [], route
