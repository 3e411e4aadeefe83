"""The elementwise ops on 8-bit levels on the GPU (liblsq_hip_eltwise_w8.so): the table op bit for bit against `table[x.long()]`,
the gate multiply bit for bit against the CPU path of the same op (tests/test_eltwise_w8_cpu.py holds that path to the existing
ops composed and to a numpy restatement), in every kernel family and on both sides of every threshold of the plans.  The table op's
plan has no cap on its grid, so there is no size at which one would be reached.  No tolerance anywhere.
"""
import pytest
import torch
import torch.nn.functional as F

import eltwise_w8_cases as C
import requant_w8_cases as R

pytestmark = pytest.mark.gpu
CL = torch.channels_last
OPS = torch.ops.torchlsq
DEV = "cuda:0"
one = C.one


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _same(got, want, note=""):
    assert got.shape == want.shape and got.dtype == want.dtype, note
    assert got.is_contiguous(memory_format=CL) if got.dim() == 4 else got.is_contiguous(), note
    assert torch.equal(C.bits(got.cpu()), C.bits(want)), note


# ---------------------------------------------------------------------------------------------------
# the table op
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    """(a random permutation of 0..255, a real hardswish table built on the GPU), on the GPU and on the CPU"""
    perm = C.perm_table()
    hsw = C.hardswish_table(DEV)
    assert sorted(perm.tolist()) == list(range(256)) and len(hsw.unique()) > 32
    return [(perm.to(DEV), perm), (hsw, hsw.cpu())]


def _lut_sizes():
    """the sizes of the issue, and one n on each side of every threshold of the plan at 256 compute units, n % 16 != 0 among
    them: 15 | 16 (the family), and 512 workgroups at 2 packets per lane"""
    edge = 512 * 256 * 2 * 16 - 2 * 256 * 16 + 16
    return list(C.LUT_SIZES) + [31, 4111, edge - 16, edge - 1, edge, edge + 5, 4 * edge + 7]


@pytest.mark.parametrize("n", _lut_sizes())
def test_table_op_is_table_of_x(n, tables):
    from torchlsq import extension as E
    x = C.lut_x(n)
    assert n < 256 or len(x.unique()) == 256
    pl = E.eltwise_w8_plan_lut(n)
    assert pl == C.expected_plan_lut(n, cus=_cus()) and pl["family"] == ("packets" if n >= 16 else "generic")
    xg = x.to(DEV)
    for tg, tc in tables:
        want = tc[x.long()]
        got = OPS.lsq_lut_w8(xg, tg, torch.uint8)
        assert got.dtype == torch.uint8 and got.shape == (n,) and torch.equal(got.cpu(), want), n
        assert torch.equal(got, tg[xg.long()])                         # torch's indexing on the GPU is the same expectation
    # int8 views of x, the table and y: the same bytes; and a second launch repeats the first bit for bit
    tg, tc = tables[0]
    got8 = OPS.lsq_lut_w8(xg.view(torch.int8), tg.view(torch.int8), torch.int8)
    assert got8.dtype == torch.int8 and torch.equal(got8.view(torch.uint8).cpu(), tc[x.long()])
    assert torch.equal(OPS.lsq_lut_w8(xg.view(torch.int8), tg.view(torch.int8), torch.int8), got8)


def test_table_op_packets_per_lane_on_this_gpu():
    """both sides of the packets-per-lane threshold with the compute units of THIS device (the sizes above assume 256)"""
    from torchlsq import extension as E
    tg, tc = C.perm_table(3).to(DEV), C.perm_table(3)
    seen = set()
    edge = 2 * _cus() * 256 * 2 * 16 - 2 * 256 * 16 + 16
    for n in (edge - 16, edge + 3):
        pl = E.eltwise_w8_plan_lut(n)
        assert pl == C.expected_plan_lut(n, cus=_cus())
        seen.add(pl["packets_per_lane"])
        x = C.lut_x(n, 1)
        assert torch.equal(OPS.lsq_lut_w8(x.to(DEV), tg, torch.uint8).cpu(), tc[x.long()]), n
    assert seen == {1, 2}


@pytest.mark.parametrize("n", (1, 17, 255, 4096 + 7))
def test_table_op_at_byte_offsets_leaves_the_guard_bytes(n, tables):
    from torchlsq import extension as E
    from torchlsq._eltwise_w8_host import eltwise_w8_lut
    x = C.lut_x(n, 2)
    tg, tc = tables[0]
    want = tc[x.long()]
    assert E.eltwise_w8_plan_lut(n, aligned=False)["family"] == "generic"
    for xo, yo in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xbuf = torch.zeros(n + 32, dtype=torch.uint8, device=DEV)
        xv = xbuf[xo:xo + n]
        xv.copy_(x)
        ybuf = torch.full((n + 48,), 77, dtype=torch.uint8, device=DEV)
        yv = ybuf[16 + yo:16 + yo + n]
        assert xv.data_ptr() % 16 == xo and yv.data_ptr() % 16 == yo
        got = eltwise_w8_lut(xv, tg, torch.uint8, out=yv)
        assert got.data_ptr() == yv.data_ptr() and torch.equal(got.cpu(), want), (n, xo, yo)
        guard = torch.cat([ybuf[:16 + yo], ybuf[16 + yo + n:]])
        assert bool((guard == 77).all()), (n, xo, yo)


def test_table_op_keeps_a_channels_last_layout_and_is_the_unfused_gpu_chain():
    """`lsq_act_w8_q` against dequantize -> hardswish -> lsq_levels_per_tensor on the same device, for channels-last levels"""
    from torchlsq.functional import LevelsTensor, lsq_act_w8_q
    lx = C.lut_x(2 * 48 * 7 * 7, 5).reshape(2, 48, 7, 7).contiguous(memory_format=CL).to(DEV)
    x = LevelsTensor(lx, one(0.05).to(DEV), one(128, torch.int32).to(DEV), 0, 255)
    o_s, o_b = one(0.03).to(DEV), one(-0.4).to(DEV)
    for mid in C.MIDS:
        got = lsq_act_w8_q(x, "hardswish", o_s, o_b, -128, 127, mid_dtype=mid)
        chain = OPS.lsq_levels_per_tensor(F.hardswish(x.dequantize(mid)), o_s, o_b, -128, 127, -128, 127, 0)
        assert got.levels.dtype == torch.int8 and got.levels.stride() == lx.stride() and torch.equal(got.levels, chain), mid
        assert len(chain.unique()) > 32


# ---------------------------------------------------------------------------------------------------
# the gate multiply
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", C.VARIANTS, ids=C.variant_id)
@pytest.mark.parametrize("geometry", C.GEOMETRIES, ids=C.geom_id)
def test_gate_multiply_packets(geometry, variant):
    """every geometry x level dtypes x zero points, every mid, levels out (both types) and floats out, against the CPU path"""
    from torchlsq import extension as E
    assert E.eltwise_w8_plan_mul(*geometry)["family"] == "packets"
    for out_variant in C.OUT_VARIANTS:
        c = C.mul_case(geometry, variant, out_variant, 11)
        want = C.run(c)
        if out_variant[0] is not None and want.numel() >= 1000:
            C.assert_conditions(want, c, (geometry, variant, out_variant))
        _same(C.run(c, DEV), want, (geometry, variant, out_variant))


def _threshold_geometries():
    """one geometry on each side of each threshold of the plan at 256 compute units: pixels per lane 1 | 2 | 4 by the size of the
    grid (4 B / P workgroups at 64 channels and 16 x 16 pixels), pixels per lane capped by H W (1 x 2, 1 x 3: the second
    pixel of the last lane lies beyond the image), and 4 pixels per lane on 15 x 15 = 225 pixels, which 4 does not divide"""
    return [(255, 64, 16, 16, 1), (256, 64, 16, 16, 2), (511, 64, 16, 16, 2), (512, 64, 16, 16, 4), (1 << 15, 64, 1, 2, 2),
            (1 << 15, 64, 1, 3, 2), (1 << 16, 64, 1, 1, 1), (576, 64, 15, 15, 4), (573, 64, 15, 15, 2)]


@pytest.mark.parametrize("geometry", _threshold_geometries(), ids=lambda g: C.geom_id(g[:4]))
def test_gate_multiply_on_both_sides_of_the_plan_thresholds(geometry):
    from torchlsq import extension as E
    *g, pix = geometry
    pl = E.eltwise_w8_plan_mul(*g)
    assert pl == C.expected_plan_mul(*g, cus=_cus())
    if _cus() == 256:
        assert pl["pixels_per_lane"] == pix and pl["family"] == "packets", pl
    for variant, out_variant in ((C.VARIANTS[2], (True, torch.bfloat16)), (C.VARIANTS[-1], (None, torch.float16))):
        c = C.mul_case(tuple(g), variant, out_variant, 17)
        _same(C.run(c, DEV), C.run(c), (g, out_variant))


@pytest.mark.parametrize("Cn", (3, 20, 24, 16))
def test_gate_multiply_generic_and_misaligned_buffers_leave_the_guard_bytes(Cn):
    from torchlsq import extension as E
    from torchlsq._eltwise_w8_host import eltwise_w8_mul_gate, eltwise_w8_mul_gate_q
    assert E.eltwise_w8_plan_mul(2, Cn, 3, 5, aligned=False)["family"] == "generic"
    assert E.eltwise_w8_plan_mul(2, Cn, 3, 5)["family"] == ("packets" if Cn == 16 else "generic")
    offsets = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)) if Cn == 16 else ((0, 0, 0),)
    for variant, (unsigned, mid) in ((C.VARIANTS[3], (False, torch.bfloat16)), (C.VARIANTS[-2], (True, torch.float32)),
                                     (C.VARIANTS[0], (None, torch.bfloat16))):
        c = C.mul_case((2, Cn, 3, 5), variant, (unsigned, mid), 19)
        lx, s_x, zx, lg, s_g, zg, osc, osh, rng, _ = c
        want = C.run(c)
        esize = want.element_size()
        consts = [t.to(DEV) for t in (s_x, zx, s_g, zg)]
        for xo, go, yo in offsets:
            xbuf = torch.zeros(lx.numel() + 32, dtype=lx.dtype, device=DEV)
            xv = xbuf[xo:xo + lx.numel()].view(2, 3, 5, Cn).permute(0, 3, 1, 2)
            xv.copy_(lx)
            gbuf = torch.zeros(lg.numel() + 32, dtype=lg.dtype, device=DEV)
            gv = gbuf[go:go + lg.numel()].view(2, Cn, 1, 1)
            gv.copy_(lg)
            ybuf = torch.full((want.numel() + 32,), 77, dtype=want.dtype, device=DEV)
            at = 16 // esize + yo                                           # a floating y stays element-aligned: yo elements on
            yv = ybuf[at:at + want.numel()].view(2, 3, 5, Cn).permute(0, 3, 1, 2)
            assert xv.data_ptr() % 16 == xo and gv.data_ptr() % 16 == go and yv.data_ptr() % 16 == yo * esize
            if rng is None:
                got = eltwise_w8_mul_gate(xv, consts[0], consts[1], gv, consts[2], consts[3], mid, out=yv)
            else:
                got = eltwise_w8_mul_gate_q(xv, consts[0], consts[1], gv, consts[2], consts[3], osc.to(DEV), osh.to(DEV), *rng, mid, out=yv)
            assert got.data_ptr() == yv.data_ptr()
            _same(got, want, (Cn, xo, go, yo, unsigned))
            guard = torch.cat([ybuf[:at], ybuf[at + want.numel():]])
            assert bool((guard == 77).all()), (Cn, xo, go, yo, unsigned)


def test_gate_multiply_images_are_independent_and_launches_repeat():
    c = C.mul_case((2, 48, 7, 7), C.VARIANTS[2], (True, torch.bfloat16), 23)
    lx, s_x, zx, lg, s_g, zg, osc, osh, rng, mid = c
    got = C.run(c, DEV)
    assert torch.equal(C.run(c, DEV), got)
    lg2, lx2 = lg.clone(), lx.clone()
    lg2[1] = lg2[1].roll(1, 0)
    lx2[1] = lx2[1].flip(0)
    moved_gate = C.run((lx, s_x, zx, lg2, s_g, zg, osc, osh, rng, mid), DEV)
    moved_bytes = C.run((lx2, s_x, zx, lg, s_g, zg, osc, osh, rng, mid), DEV)
    for moved in (moved_gate, moved_bytes):
        assert torch.equal(moved[0], got[0]) and C.differ(moved[1].cpu(), got[1].cpu()) > 0.4


@pytest.mark.parametrize("geometry", ((2, 48, 7, 7), (3, 32, 1, 1), (2, 20, 3, 5)), ids=C.geom_id)
def test_gate_multiply_is_the_existing_gpu_ops_composed(geometry):
    """the definition on the device: `dequantize`, `torch.mul` and `lsq_levels_per_tensor` on the GPU"""
    for variant in (C.VARIANTS[0], C.VARIANTS[9], C.VARIANTS[-1]):
        for out_variant in C.OUT_VARIANTS:
            c = C.mul_case(geometry, variant, out_variant, 29)
            got, want = C.run(c, DEV), C.composed(c, DEV)
            assert got.dtype == want.dtype and torch.equal(C.bits(got), C.bits(want)), (geometry, variant, out_variant)


# ---------------------------------------------------------------------------------------------------
# the tables across devices, the modules
# ---------------------------------------------------------------------------------------------------
def test_clamp_type_tables_are_the_same_on_both_devices():
    """asserted for identity, relu, relu6 and hardtanh; for the other named functions ATen's CPU and GPU kernels may round
    differently, so the number of entries that differ is printed (DESIGN.md 9.13 reports it) and nothing is asserted"""
    from torchlsq.functional import lsq_act_table
    report = []
    for fn in C.NAMED:
        worst = 0
        for mid, in_dtype, unsigned in ((m, d, u) for m in C.MIDS for d in C.LEVEL_DTYPES for u in (True, False)):
            s, z = one(0.047), one(131 if in_dtype == torch.uint8 else 3, torch.int32)
            rng = (0, 255) if unsigned else (-128, 127)
            osc, osh = one(0.021), one(-2.0 if unsigned else 0.4)
            cpu = lsq_act_table(fn, s, z, in_dtype, osc, osh, *rng, mid_dtype=mid)
            gpu = lsq_act_table(fn, s.to(DEV), z.to(DEV), in_dtype, osc.to(DEV), osh.to(DEV), *rng, mid_dtype=mid)
            assert gpu.is_cuda and gpu.dtype == torch.uint8
            n = int((gpu.cpu() != cpu).sum())
            if fn in C.CLAMP_TYPE:
                assert n == 0, (fn, mid, in_dtype, unsigned)
            worst = max(worst, n)
        report.append("%s %d" % (fn, worst))
    print("entries of 256 that differ between a table built on the CPU and on the GPU, the most over 12 cases: " + ", ".join(report))


@pytest.mark.parametrize("fn", ("silu", "gelu"))
def test_activation_module_with_a_gpu_built_table_is_the_unfused_gpu_chain(fn):
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import ActivationW8Q
    lx = C.lut_x(2 * 32 * 9 * 7, 7).reshape(2, 32, 9, 7).contiguous(memory_format=CL)
    sample = (lx.float() - 120) * 0.04
    q_in = R.trained_quantizer(sample)
    call = {"silu": F.silu, "gelu": F.gelu}[fn]
    q_out = R.trained_quantizer(call(sample))
    for mid in C.MIDS:
        m = ActivationW8Q.from_float(fn, q_in, q_out, mid_dtype=mid, device=DEV)
        assert m.table.is_cuda and m.output_scale.is_cuda
        xc = LevelsTensor.from_quantized(q_in.quantize(sample))
        xl = LevelsTensor(xc.levels.to(DEV), xc.scale.to(DEV), xc.zero_point.to(DEV), xc.quant_min, xc.quant_max, xc.type_min, xc.type_max)
        got = m(xl)
        q_gpu = q_out.to(DEV)
        with torch.no_grad():
            chain = q_gpu.quantize(call(xl.dequantize(mid))).int_repr()
        q_out.to("cpu")
        assert torch.equal(got.levels, chain) and len(chain.unique()) > 32, (fn, mid)


@pytest.mark.parametrize("mid", R.MIDS, ids=C.name)
def test_the_converted_mobilenet_v3_block_in_a_graph(mid):
    from torchlsq.functional import LevelsTensor
    net, qs, x = C.v3_block()
    new = C.convert_v3_block(net, qs, mid)
    xl = LevelsTensor.from_quantized(qs["in"].quantize(x))
    want = new(xl).levels
    other = LevelsTensor.from_quantized(qs["in"].quantize(x.flip(0) * 0.5 + 0.1))
    want_other = new(other).levels
    assert not torch.equal(want, want_other) and len(want.unique()) > 16
    gnew = new.to(DEV)                                                      # the tables were built on the CPU: the CPU modules' bytes
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
