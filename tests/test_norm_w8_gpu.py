"""LayerNorm and RMSNorm on 8-bit levels on the GPU (liblsq_hip_norm_w8.so): bit for bit against the CPU path of the same ops
(tests/test_norm_w8_cpu.py holds that path to a numpy restatement and to float64), in both kernel families, at every (L, P) the
plan can emit, in both placements of w and bias, and on both sides of every threshold of the plan.  No tolerance anywhere.
"""
import pytest
import torch

import norm_w8_cases as N

pytestmark = pytest.mark.gpu
CL = torch.channels_last
DEV = "cuda:0"
one = N.one
LP = N.every_lp()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _same(got, want, note=""):
    assert got.shape == want.shape and got.dtype == want.dtype and got.is_contiguous(), note
    assert torch.equal(N.bits(got.cpu()), N.bits(want)), note


def _case(kind, R_, C, x_dtype, z_u8, unsigned, mid, seed=0, pdt=torch.float32, has_w=True, has_b=True):
    """(the op's arguments on the CPU, the CPU path's result); the non-vacuity conditions are asserted on that result"""
    x, s, z = N.rows(R_, C, seed, x_dtype), one(N.S_X), N.zero_for(x_dtype, z_u8)
    w, b = N.params(C, seed, pdt)
    w, b = (w if has_w else None), (b if has_b else None)
    q = None if unsigned is None else N.quantizer_for(kind, x, s, z, w, b, N.EPS[kind], unsigned, N.one_sided(kind, z_u8))
    want = N.run(kind, x, s, z, w, b, N.EPS[kind], q, mid)
    if q is not None:
        N.assert_conditions(kind, x, s, z, w, b, N.EPS[kind], q, mid, want, (kind, R_, C))
    return (kind, x, s, z, w, b, N.EPS[kind], q, mid), want


def _check(args, want, note=""):
    got = N.run_on(DEV, *args)
    _same(got, want, note)
    return got


# ---------------------------------------------------------------------------------------------------
# the packets family: a row in the registers of L lanes, P packets each
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 32, 48, 96, 768, 1024, 1040, 4096, 8192])
@pytest.mark.parametrize("kind", N.KINDS)
def test_packets_family_equals_the_cpu_path(kind, C):
    from torchlsq import extension as E
    R_ = N.rows_for(C)
    pl = E.norm_w8_plan(R_, C)
    assert pl == N.expected_plan(R_, C, cus=_cus()) and pl["family"] == "packets"
    assert pl["params"] == ("registers" if pl["packets_per_lane"] == 1 else "lds")
    assert pl["lds_bytes"] == (0 if pl["packets_per_lane"] == 1 else 8 * C)
    for x_dtype, unsigned, mid in ((torch.uint8, True, torch.float32), (torch.int8, False, torch.bfloat16), (torch.uint8, False, torch.float16)):
        _check(*_case(kind, R_, C, x_dtype, 128, unsigned, mid), (kind, C, x_dtype, mid))
    # RMSNorm with the zero point at the low end; weight or bias alone, and neither.  Without w an RMSNorm's values end near
    # sqrt(10) (a 3 sigma value of the row whose mean is a third of its spread) while its bulk sits on +-1, so the output
    # quantizer's borders lie out of reach: those two give floats (LayerNorm's give levels)
    no_w = (False, True) if kind == "layer" else (None, None)
    _check(*_case(kind, R_, C, torch.uint8, 3, True, torch.bfloat16, 1), (kind, C, "z3"))
    _check(*_case(kind, R_, C, torch.int8, 0, True, torch.float32, 2, has_b=False), (kind, C, "no bias"))
    _check(*_case(kind, R_, C, torch.uint8, 128, no_w[0], torch.float32, 3, has_w=False), (kind, C, "no weight"))
    _check(*_case(kind, R_, C, torch.uint8, 128, no_w[1], torch.float32, 4, has_w=False, has_b=False), (kind, C, "plain"))


def test_the_pairs_of_lanes_and_packets_the_plan_can_emit():
    assert len(LP) == 39 and {p for _, p in LP} == set(range(1, 9)) and {l for l, _ in LP} == {4, 8, 16, 32, 64}
    assert sum(L * P > C // 16 for (L, P), C in LP.items()) >= 30          # rows that leave packet slots of their last lanes empty


@pytest.mark.parametrize("LP_", sorted(LP), ids=lambda v: "L%d_P%d" % v)
def test_every_lanes_and_packets_pair(LP_):
    """the smallest C for each (L, P) the plan can emit: both placements of w and bias and masked packet slots among them"""
    from torchlsq import extension as E
    C = LP[LP_]
    pl = E.norm_w8_plan(N.rows_for(C), C)
    assert (pl["lanes_per_row"], pl["packets_per_lane"]) == LP_, (C, pl)
    for kind, x_dtype, pdt in (("layer", torch.uint8, torch.float32), ("rms", torch.int8, torch.bfloat16)):
        _check(*_case(kind, N.rows_for(C), C, x_dtype, 128, True, torch.bfloat16, pdt=pdt), (LP_, C, kind))


def _rows_cases():
    """R on each side of every threshold: the rows a workgroup takes (C = 16: 64 groups a workgroup), and the rows-per-group rule
    (8 rows a group from 2 * 256 workgroups on)"""
    edge = (512 - 1) * 64 * 8 + 1                    # the smallest R with 512 workgroups at 8 rows a group
    return [1, 2, 63, 64, 65, edge - 1, edge]


@pytest.mark.parametrize("R_", _rows_cases())
def test_rows_on_each_side_of_the_plan_thresholds(R_):
    from torchlsq import extension as E
    pl = E.norm_w8_plan(R_, 16)
    assert pl == N.expected_plan(R_, 16, cus=_cus())
    _check(*_case("layer", R_, 16, torch.uint8, 128, True, torch.bfloat16), R_)


def test_rows_per_group_on_this_gpu():
    """both sides of the rows-per-group rule with the compute units of THIS device, at C = 16 (64 groups a workgroup)"""
    from torchlsq import extension as E
    fill, seen = 2 * _cus(), set()
    for K in (2, 8):
        edge = (fill - 1) * 64 * K + 1
        for R_ in (edge - 1, edge):
            pl = E.norm_w8_plan(R_, 16)
            assert pl == N.expected_plan(R_, 16, cus=_cus())
            seen.add(pl["rows_per_workgroup"])
            _check(*_case("rms", R_, 16, torch.int8, 128, False, torch.float32), R_)
    assert seen == {64 * 8, 64 * 4, 64 * 2, 64}


# ---------------------------------------------------------------------------------------------------
# the generic family
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 20, 24, 8208, 65536])
@pytest.mark.parametrize("kind", N.KINDS)
def test_generic_family_equals_the_cpu_path(kind, C):
    from torchlsq import extension as E
    # (a LayerNorm value of C = 3 elements cannot exceed sqrt(C - 1) = 1.41, less than the two bulk deviations at which the output
    #  quantizer's borders lie: that case stays small, 72 outputs, and only the larger ones are held to the conditions)
    R_ = N.rows_for(C) if C >= 16 else 24
    assert E.norm_w8_plan(R_, C)["family"] == "generic" and E.norm_w8_plan(R_, C) == N.expected_plan(R_, C)
    for x_dtype, z, unsigned, mid, pdt in ((torch.uint8, 128, True, torch.float32, torch.float32), (torch.int8, 3, False, torch.bfloat16, torch.float16),
                                           (torch.uint8, 0, None, torch.float16, torch.bfloat16)):
        _check(*_case(kind, R_, C, x_dtype, z, unsigned, mid, pdt=pdt), (kind, C, x_dtype, mid))


@pytest.mark.parametrize("which", ["x", "y"])
def test_a_misaligned_buffer_takes_the_generic_family_and_writes_its_bytes_only(which):
    from torchlsq import extension as E
    args, want = _case("layer", 7, 16, torch.uint8, 128, True, torch.float32)
    kind, x, s, z, w, b, eps, q, mid = args
    assert E.norm_w8_plan(7, 16, aligned=False)["family"] == "generic"
    buf = torch.full((7 * 16 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    s, z, w, b, osc, osh = N.to(DEV, s, z, w, b, q[0], q[1])
    if which == "x":
        buf[1:1 + 112] = x.to(DEV).reshape(-1)
        xg = buf[1:1 + 112].view(7, 16)
        assert xg.data_ptr() % 16 == 1
        got = E.norm_w8_layer_q(xg, s, z, w, b, eps, osc, osh, *q[2], mid)
    else:
        out = buf[1:1 + 112].view(7, 16)
        assert out.data_ptr() % 16 == 1
        got = E.norm_w8_layer_q(x.to(DEV), s, z, w, b, eps, osc, osh, *q[2], mid, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert bool((buf[:1] == 0xA5).all()) and bool((buf[113:] == 0xA5).all())          # the guard bytes
    assert torch.equal(got.cpu(), want)


# ---------------------------------------------------------------------------------------------------
# exact integer statistics, the roundings, independence of rows
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8192, 65536])
def test_planted_integer_statistics_rows(C):
    for x_dtype in N.LEVEL_DTYPES:
        x, at = N.planted(C, x_dtype)
        w, b = N.params(C)
        s = one(N.S_X)
        q = (one(0.02), one(-128 * 0.02), (0, 255, 0, 255))
        args = ("layer", x, s, N.zero_for(x_dtype, 128), w, b, 1e-5, q, torch.float32)
        want = N.run(*args)
        _check(args, want, (C, x_dtype))
        assert len(want[at["one_zero_in_255s"]].unique()) >= 2 and len(want[at["one_8_in_7s"]].unique()) >= 2
        for z in (0, 3, 128):
            args = ("rms", x, s, N.zero_for(x_dtype, z), w, b, 1e-6, q, torch.float32)
            _check(args, N.run(*args), (C, x_dtype, z))


def test_product_and_add_are_rounded_apart_and_a_nan_goes_to_quant_min():
    q = (one(N.NO_FMA_SCALE), one(0.0), (0, 255, 0, 255))
    for seed in N.NO_FMA_SEEDS:
        x, w, b, at, fused = N.no_fma_case(seed)
        args = ("layer", x, one(N.S_X), one(128, torch.int32), w, b, 1e-5, q, torch.float32)
        want = N.run(*args)
        assert len(at) >= 8 and bool((want[0, at].numpy() != fused).all())
        _check(args, want, seed)
    for kind in N.KINDS:
        args, want = _case(kind, 70, 48, torch.uint8, 128, True, torch.bfloat16)
        w = args[4].clone()
        w[5] = float("nan")
        q = (args[7][0], args[7][1], (3, 200, 0, 255))
        args = args[:4] + (w,) + args[5:7] + (q, args[8])
        want = N.run(*args)
        assert bool((want[:, 5] == 3).all()) and len(want[:, 4].unique()) > 4
        _check(args, want, kind)


def test_rows_are_independent_and_launches_repeat():
    for kind, C in (("layer", 768), ("rms", 1040), ("layer", 20)):
        args, want = _case(kind, 67, C, torch.uint8, 128, True, torch.bfloat16)
        got = _check(args, want)
        assert torch.equal(N.run_on(DEV, *args), got)
        perm = torch.randperm(67, generator=torch.Generator().manual_seed(5))
        assert torch.equal(N.run_on(DEV, args[0], args[1][perm], *args[2:]), got[perm.to(DEV)])


@pytest.mark.parametrize("mid", N.MIDS, ids=N.name)
def test_floats_out(mid):
    for kind, C in (("layer", 96), ("rms", 768), ("layer", 4096), ("rms", 24)):
        args, want = _case(kind, 11, C, torch.int8, 128, None, mid)
        assert want.dtype == mid
        _check(args, want, (kind, C))


def test_dim_1_on_channels_last_levels():
    from torchlsq.functional import LevelsTensor, lsq_layer_norm_w8, lsq_layer_norm_w8_q, lsq_rms_norm_w8_q
    x = N.rows(2 * 5 * 7, 96).reshape(2, 5, 7, 96).permute(0, 3, 1, 2)
    assert x.is_contiguous(memory_format=CL)
    w, b = N.params(96)
    s, z = one(N.S_X), one(128, torch.int32)
    q = N.quantizer_for("layer", x.permute(0, 2, 3, 1), s, z, w, b, 1e-6, True)
    X, Xg = LevelsTensor(x, s, z, 0, 255), LevelsTensor(x.to(DEV), s.to(DEV), z.to(DEV), 0, 255)
    for fn in (lsq_layer_norm_w8_q, lsq_rms_norm_w8_q):
        want = fn(X, w, b, 1e-6, q[0], q[1], 0, 255, mid_dtype=torch.bfloat16, dim=1)
        got = fn(Xg, w.to(DEV), b.to(DEV), 1e-6, q[0].to(DEV), q[1].to(DEV), 0, 255, mid_dtype=torch.bfloat16, dim=1)
        assert got.levels.shape == (2, 96, 5, 7) and got.levels.is_contiguous(memory_format=CL)
        assert torch.equal(got.levels.cpu(), want.levels) and torch.equal(got.zero_point.cpu(), want.zero_point)
    v = lsq_layer_norm_w8(Xg, w.to(DEV), b.to(DEV), 1e-6, torch.float16, dim=1)
    assert v.is_contiguous(memory_format=CL) and torch.equal(N.bits(v.cpu()), N.bits(lsq_layer_norm_w8(X, w, b, 1e-6, torch.float16, dim=1)))


# ---------------------------------------------------------------------------------------------------
# the converted blocks, captured in a graph
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", ["convnext", "token"])
def test_converted_block_in_a_graph_replayed_on_new_bytes(block):
    from torchlsq.functional import LevelsTensor
    mid = torch.bfloat16
    net, qs, x = N.cn_block() if block == "convnext" else N.token_block()
    new = (N.convert_cn_block if block == "convnext" else N.convert_token_block)(net, qs, mid)
    xl = LevelsTensor.from_quantized(qs["in"].quantize(x))
    x2 = LevelsTensor.from_quantized(qs["in"].quantize(torch.roll(x, 1, -1) * 0.7))
    want, want2 = new(xl).levels, new(x2).levels
    assert not torch.equal(want, want2) and len(want.unique()) > 32
    gpu = new.to(DEV)
    static = LevelsTensor(xl.levels.to(DEV), xl.scale.to(DEV), xl.zero_point.to(DEV), 0, 255)
    eager = gpu(static).levels
    assert torch.equal(eager.cpu(), want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gpu(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gpu(static).levels
    graph.replay()
    assert torch.equal(out.cpu(), want)
    static.levels.copy_(x2.levels)
    graph.replay()
    assert torch.equal(out.cpu(), want2)
