"""Pooling on 8-bit levels on the GPU (liblsq_hip_pool_w8.so): every result bit for bit against the CPU path of the same op
(tests/test_pool_w8_cpu.py holds that path to torch's pooling and to a numpy restatement), in every kernel family and on both
sides of every threshold of the plans.
"""
import pytest
import torch
import torch.nn.functional as F

import pool_w8_cases as P
import requant_w8_cases as R

pytestmark = pytest.mark.gpu
CL = torch.channels_last
OPS = torch.ops.torchlsq
DEV = "cuda:0"


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same(got, want, note=""):
    assert got.shape == want.shape and got.dtype == want.dtype and got.is_contiguous(memory_format=CL), note
    assert torch.equal(_bits(got.cpu()), _bits(want)), note


def _max(lx, geom):
    H, W, k, s, p, d, ceil_mode = geom
    return OPS.lsq_max_pool2d_q8(lx, list(k), list(s), list(p), list(d), ceil_mode)


@pytest.mark.parametrize("dtype", P.LEVEL_DTYPES, ids=("u8", "i8"))
@pytest.mark.parametrize("geom", P.MAX_GEOMS, ids=P.geom_id)
def test_max_pool_packets(geom, dtype):
    from torchlsq import extension as E
    for C in (16, 48):
        lx, _, _ = P.x_levels(2, C, geom[0], geom[1], dtype, C)
        lx = P.negative_corner(lx) if dtype == torch.int8 else lx
        assert E.pool_w8_plan_max(2, C, *geom[:7])["family"] == "packets"
        want = _max(lx, geom)
        _same(_max(lx.to(DEV), geom), want, (geom, C))
        assert len(want.unique()) > 32
        if dtype == torch.int8 and max(geom[4]) > 0:
            assert bool((want[:, :, 0, 0] < 0).all())            # a padded tap taken for the byte 0 would show here


@pytest.mark.parametrize("C", (3, 20, 24, 16))
def test_max_pool_generic_and_misaligned_buffers_leave_the_guard_bytes(C):
    from torchlsq import extension as E
    from torchlsq._pool_w8_host import pool_w8_max
    geom = P.MAX_GEOMS[0]
    lx, _, _ = P.x_levels(2, C, 9, 7, torch.int8, 2)
    want = _max(lx, geom)
    assert E.pool_w8_plan_max(2, C, *geom[:7], aligned=False)["family"] == "generic"
    offsets = ((0, 0), (1, 0), (0, 1), (1, 1)) if C == 16 else ((0, 0),)
    for xo, yo in offsets:
        xbuf = torch.zeros(lx.numel() + 32, dtype=torch.int8, device=DEV)
        xv = xbuf[xo:xo + lx.numel()].view(2, 9, 7, C).permute(0, 3, 1, 2)
        xv.copy_(lx)
        ybuf = torch.full((want.numel() + 32,), 77, dtype=torch.int8, device=DEV)
        yv = ybuf[16 + yo:16 + yo + want.numel()].view(2, 5, 4, C).permute(0, 3, 1, 2)
        assert xv.data_ptr() % 16 == xo and yv.data_ptr() % 16 == yo
        got = pool_w8_max(xv, [3, 3], [2, 2], [1, 1], [1, 1], False, out=yv)
        assert got.data_ptr() == yv.data_ptr()
        _same(got, want, (C, xo, yo))
        guard = torch.cat([ybuf[:16 + yo], ybuf[16 + yo + want.numel():]])
        assert bool((guard == 77).all()), (C, xo, yo)


def test_max_pool_is_the_existing_gpu_ops_composed():
    from torchlsq.functional import LevelsTensor
    for dtype in P.LEVEL_DTYPES:
        lx, s_x, zx = P.x_levels(2, 32, 9, 7, dtype, 4)
        lo, hi = R.W.LEVEL_RANGE[dtype]
        x = LevelsTensor(lx.to(DEV), s_x.to(DEV), zx.to(DEV), lo, hi)
        got = _max(x.levels, P.MAX_GEOMS[0])
        for mid in P.MIDS:
            pooled = F.max_pool2d(x.dequantize(mid), 3, 2, 1)
            back = OPS.lsq_levels_per_tensor(pooled, x.scale, -x.zero_point.float() * x.scale, lo, hi, lo, hi, 0)
            assert torch.equal(back.view(dtype), got), (dtype, mid)


@pytest.mark.parametrize("variant", P.AVG_VARIANTS, ids=P.avg_id)
@pytest.mark.parametrize("case", P.AVG_LANE_CASES, ids=P.geom_id)
def test_avg_pool_window_per_lane(case, variant):
    from torchlsq import extension as E
    unsigned, mid = variant
    assert E.pool_w8_plan_avg(2, 32, case[0], case[1], case[2], case[3], case[4], case[5])["family"] == "packets"
    for x_dtype in P.LEVEL_DTYPES:
        c = P.avg_case(2, 32, case, x_dtype, bool(unsigned), 9)
        lx, s_x, zx, args, osc, osh, rng = c
        dev = R.to(DEV, lx, s_x, zx)
        if unsigned is None:
            _same(P.avg_float(*dev, args, mid), P.avg_float(lx, s_x, zx, args, mid), (case, variant, x_dtype))
        else:
            want = P.avg_q(*c, mid)
            P.assert_conditions(want, c, mid, (case, variant, x_dtype))
            _same(P.avg_q(*dev, args, *R.to(DEV, osc, osh), rng, mid), want, (case, variant, x_dtype))


# (B, C, H, W, kernel = stride): global pooling and adaptive sizes, on both sides of every threshold of the split
SHARED_CASES = [
    (3, 32, 7, 7, (7, 7)),              # global 7 x 7: 32 lanes
    (1, 16, 33, 31, (33, 31)),          # 1023 taps: 256 lanes, not a multiple of any split
    (2, 16, 8, 6, (4, 3)),              # adaptive 2 x 2 from 8 x 6: 12 taps, 8 lanes
    (2, 16, 6, 6, (2, 3)),              # 6 taps, not a square window: a window per lane, the kernel with the tap loops
    (2, 16, 6, 6, (3, 3)),              # 9 taps: a window per lane ...
    (2, 16, 4, 10, (2, 5)),             # ... 10 taps: shared
    (1, 16, 3, 5, (3, 5)),              # 15 taps: 8 lanes at most ...
    (1, 16, 4, 4, (4, 4)),              # ... 16 taps: 16
    (1, 16, 15, 17, (15, 17)),          # 255 taps: 128 lanes at most ...
    (1, 16, 16, 16, (16, 16)),          # ... 256 taps: 256
]


@pytest.mark.parametrize("case", SHARED_CASES, ids=P.geom_id)
def test_avg_pool_window_per_workgroup(case):
    from torchlsq import extension as E
    B, C, H, W, k = case
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    family, lanes, grid = P.expected_avg_plan(B, C, H // k[0], W // k[1], k[0] * k[1], True, cus)
    pl = E.pool_w8_plan_avg(B, C, H, W, k)
    assert (pl["family"], pl["lanes_per_window"], pl["grid"]) == (family, lanes, grid), pl
    assert (family == "packets_shared") == (k[0] * k[1] >= 10)
    args = (list(k), list(k), [0, 0], False, True, None)
    for x_dtype, (unsigned, mid) in zip(P.LEVEL_DTYPES * 5, P.AVG_VARIANTS):
        lx, s_x, zx = P.x_levels(B, C, H, W, x_dtype, 13)
        dev = R.to(DEV, lx, s_x, zx)
        if unsigned is None:
            _same(P.avg_float(*dev, args, mid), P.avg_float(lx, s_x, zx, args, mid), (case, mid))
        else:
            osc, osh, rng = R.out_quantizer(P.avg_float(lx, s_x, zx, args), unsigned, False)
            want = P.avg_q(lx, s_x, zx, args, osc, osh, rng, mid)
            assert len(want.unique()) > min(16, want.numel() // 4)
            if want.numel() >= 336:
                P.assert_conditions(want, (lx, s_x, zx, args, osc, osh, rng), mid, (case, unsigned, mid))
            _same(P.avg_q(*dev, args, *R.to(DEV, osc, osh), rng, mid), want, (case, unsigned, mid))


def test_avg_pool_on_both_sides_of_the_grid_that_fills_the_chip():
    from torchlsq import extension as E
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 2 * cus * 256 // (8 * 128)                     # 8 images of rows x 128 windows of 10 taps: 2 cus workgroups of lanes
    seen = set()
    for OH, x_dtype, unsigned in ((rows - 1, torch.uint8, True), (rows, torch.int8, False)):
        case = (2 * OH, 640, (2, 5), (2, 5), (0, 0), False, True, None)
        c = P.avg_case(8, 16, case, x_dtype, unsigned, 5)     # the output quantizer from the float32 averages, as everywhere
        lx, s_x, zx, args, osc, osh, rng = c
        pl = E.pool_w8_plan_avg(8, 16, 2 * OH, 640, (2, 5))
        assert (pl["family"], pl["lanes_per_window"], pl["grid"]) == P.expected_avg_plan(8, 16, OH, 128, 10, True, cus)
        seen.add(pl["lanes_per_window"])
        want = P.avg_q(*c, torch.float32)
        P.assert_conditions(want, c, torch.float32, OH)
        _same(P.avg_q(*R.to(DEV, lx, s_x, zx), args, *R.to(DEV, osc, osh), rng, torch.float32), want, OH)
    assert seen == {1, 2}


def test_the_32_bit_sum_and_the_one_rounding_of_a_sum_beyond_24_bits():
    k = [260, 260]
    args = (k, k, [0, 0], False, True, None)
    zero = torch.zeros(1, dtype=torch.int32)
    full = torch.full((1, 16, 260, 260), 255, dtype=torch.uint8).contiguous(memory_format=CL)
    full[0, 1::2, 7, 5:8] = 254                          # S = 17 238 000 and 17 237 997: beyond 2^24, the odd one no float32
    rand, s_x, zx = P.x_levels(1, 16, 260, 260, torch.int8, 6)
    assert len(P.avg_float(rand, s_x, zx, args).unique()) > 8 and len(P.avg_float(full, s_x, zero, args).unique()) == 2
    for lx, z in ((full, zero), (rand, zx), (rand, torch.tensor([-128], dtype=torch.int32))):
        for mid in P.MIDS:
            want = P.avg_float(lx, s_x, z, args, mid)
            _same(P.avg_float(*R.to(DEV, lx, s_x, z), args, mid), want, mid)


@pytest.mark.parametrize("C", (3, 20, 24, 16))
def test_avg_pool_generic_and_misaligned_buffers_leave_the_guard_bytes(C):
    from torchlsq import extension as E
    from torchlsq._pool_w8_host import pool_w8_avg, pool_w8_avg_q
    case = P.AVG_LANE_CASES[2]
    assert E.pool_w8_plan_avg(2, C, 12, 10, 3, 2, 1, aligned=False)["family"] == "generic"
    c = P.avg_case(2, C, case, torch.uint8, False, 3)
    lx, s_x, zx, args, osc, osh, rng = c
    want = P.avg_q(*c, torch.bfloat16)
    wantf = P.avg_float(lx, s_x, zx, args, torch.bfloat16)
    if want.numel() >= 336:
        P.assert_conditions(want, c, torch.bfloat16, C)
    offsets = ((0, 0), (1, 0), (0, 1), (1, 1)) if C == 16 else ((0, 0),)
    for xo, yo in offsets:
        xbuf = torch.zeros(lx.numel() + 32, dtype=torch.uint8, device=DEV)
        xv = xbuf[xo:xo + lx.numel()].view(2, 12, 10, C).permute(0, 3, 1, 2)
        xv.copy_(lx)
        ybuf = torch.full((want.numel() + 32,), 77, dtype=torch.int8, device=DEV)
        yv = ybuf[16 + yo:16 + yo + want.numel()].view(2, 6, 5, C).permute(0, 3, 1, 2)
        got = pool_w8_avg_q(xv, s_x.to(DEV), zx.to(DEV), *args, osc.to(DEV), osh.to(DEV), *rng, torch.bfloat16, out=yv)
        _same(got, want, (C, xo, yo))
        guard = torch.cat([ybuf[:16 + yo], ybuf[16 + yo + want.numel():]])
        assert bool((guard == 77).all()), (C, xo, yo)
        # floats out: y at an offset of one element (2 bytes), x at `xo`
        fbuf = torch.full((wantf.numel() + 16,), 3.0, dtype=torch.bfloat16, device=DEV)
        fv = fbuf[8 + yo:8 + yo + wantf.numel()].view(2, 6, 5, C).permute(0, 3, 1, 2)
        _same(pool_w8_avg(xv, s_x.to(DEV), zx.to(DEV), *args, torch.bfloat16, out=fv), wantf, (C, xo, yo))
        assert bool((torch.cat([fbuf[:8 + yo], fbuf[8 + yo + wantf.numel():]]) == 3.0).all()), (C, xo, yo)


def test_launches_repeat_and_an_output_depends_on_its_own_image_alone():
    lx, s_x, zx = P.x_levels(3, 32, 14, 14, torch.uint8, 8)
    dev = R.to(DEV, lx, s_x, zx)
    runs = {"max": lambda x: _max(x, P.MAX_GEOMS[0])}
    for name, args in (("lane", ([3, 3], [2, 2], [1, 1], False, True, None)), ("shared", ([7, 7], [7, 7], [0, 0], False, True, None))):
        osc, osh, rng = R.out_quantizer(P.avg_float(lx, s_x, zx, args), True, False)
        c = (lx, s_x, zx, args, osc, osh, rng)
        P.assert_conditions(P.avg_q(*c, torch.float32), c, torch.float32, name)
        runs[name] = lambda x, args=args, q=R.to(DEV, osc, osh), rng=rng: P.avg_q(x, dev[1], dev[2], args, *q, rng, torch.float32)
    other = dev[0].clone()
    other[0] = 255 - other[0]
    other[2] = 0
    for name, run in runs.items():
        first = run(dev[0])
        for _ in range(3):
            assert torch.equal(run(dev[0]), first), name
        assert torch.equal(run(other)[1], first[1]) and not torch.equal(run(other)[0], first[0]), name
        assert torch.equal(run(dev[0][1:2])[0], first[1]), name


@pytest.mark.parametrize("mid", R.MIDS, ids=lambda v: str(v).replace("torch.", ""))
def test_the_converted_small_network_in_a_graph(mid):
    from torchlsq.functional import LevelsTensor
    net, qs, x = P.small_net()
    new = P.convert_small_net(net, qs, mid)
    xq = qs["x"].quantize(x)
    xl = LevelsTensor.from_quantized(xq)
    want = new(xl).levels
    other = LevelsTensor.from_quantized(qs["x"].quantize(x.flip(0) * 0.5 + 0.1))
    want_other = new(other).levels
    assert not torch.equal(want, want_other) and len(want.unique()) > 16
    gnew = new.to(DEV)
    static = LevelsTensor(xl.levels.to(DEV), xl.scale.to(DEV), xl.zero_point.to(DEV), xl.quant_min, xl.quant_max, xl.type_min, xl.type_max)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert torch.equal(gnew(static).levels.cpu(), want)            # eager, and the warm-up of the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gnew(static).levels
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    static.levels.copy_(other.levels)                                   # new input bytes, the same graph
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want_other)
