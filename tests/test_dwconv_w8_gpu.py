"""The W8A8 depthwise conv2d on 8-bit levels on the GPU (liblsq_hip_dwconv_w8.so): every result bit for bit against the CPU path
of the same op (tests/test_dwconv_w8_cpu.py holds that path to the existing dense op and to a numpy restatement), in every kernel
family, at every border, and against the existing GPU ops composed through the dense embedding.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dwconv_w8_cases as D
import qconv_w8_cases as V
import qlinear_w8_cases as W
import requant_w8_cases as R

pytestmark = pytest.mark.gpu
CL = torch.channels_last
OPS = torch.ops.torchlsq
DEV = "cuda:0"


def _same(got, want, note=""):
    assert got.shape == want.shape and got.dtype == want.dtype and got.is_contiguous(memory_format=CL), note
    assert torch.equal(D.bits(got.cpu()), D.bits(want)), note


def _plan(g, **kw):
    from torchlsq import extension as E
    return E.dwconv_w8_plan(*g[:4], g[4], g[5], g[6], g[7], **kw)


@pytest.mark.parametrize("variant", D.VARIANTS, ids=range(len(D.VARIANTS)))
@pytest.mark.parametrize("geometry", D.GEOMETRIES, ids=D.geom_id)
def test_gpu_is_the_cpu_path_bit_for_bit(geometry, variant):
    """five operand variants x u8, i8 and float outputs x three mid x three act"""
    pl = _plan(geometry)
    assert pl["family"] == "packets"
    assert pl["unrolled_window"] == (3 if geometry[4] == (3, 3) and geometry[7] == (1, 1) else 0)
    for out_variant in D.OUT_VARIANTS:
        c = D.case(geometry, variant, out_variant, 5)
        want = D.run(c)
        _same(D.run(c, DEV), want, (geometry, variant, out_variant))
        if out_variant[0] is not None and want.numel() >= 1000:
            D.assert_conditions(want, c, (geometry, variant, out_variant))


@pytest.mark.parametrize("stride", (1, 2))
def test_every_output_width_around_the_pixels_of_a_lane(stride):
    # OW = 1 .. 9 covers both sides of every tail of P = 1, 2 and 4 output pixels per lane
    seen = set()
    for Wd in range(1, 19):
        g = (2, 32, 5, Wd, (3, 3), (stride, stride), (1, 1), (1, 1))
        OW = D.out_hw(g)[1]
        if OW in seen or OW > 9:
            continue
        seen.add(OW)
        for out_variant in ((True, torch.bfloat16, 2), (None, torch.float32, 0)):
            c = D.case(g, D.VARIANTS[1], out_variant, Wd)
            _same(D.run(c, DEV), D.run(c), (g, out_variant))
    assert seen == set(range(1, 10))


@pytest.mark.parametrize("C", (3, 20, 24, 16))
def test_generic_and_misaligned_buffers_leave_the_guard_bytes(C):
    from torchlsq._dwconv_w8_host import dwconv_w8_levels, dwconv_w8_levels_q
    g = (2, C, 9, 7, (3, 3), (2, 2), (1, 1), (1, 1))
    assert _plan(g, aligned=False)["family"] == "generic" and _plan(g, y_aligned=False)["family"] == "generic"
    assert _plan(g)["family"] == ("packets" if C == 16 else "generic")
    offsets = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)) if C == 16 else ((0, 0, 0),)
    for variant, out_variant in ((D.VARIANTS[0], (False, torch.float32, 1)), (D.VARIANTS[2], (True, torch.float16, 2))):
        c = D.case(g, variant, out_variant, 3)
        lx, s, z, lw, s_w, zw, bias, geo, osc, osh, rng, act, mid = c
        want = D.run(c)
        wantf = D.run(c[:8] + (None, None, None, act, mid))
        if want.numel() >= 1000:
            D.assert_conditions(want, c, (C, out_variant))
        dev = R.to(DEV, s, z, s_w, zw, bias, osc, osh)
        for xo, wo, yo in offsets:
            xbuf = torch.zeros(lx.numel() + 32, dtype=lx.dtype, device=DEV)
            xv = xbuf[xo:xo + lx.numel()].view(2, 9, 7, C).permute(0, 3, 1, 2)
            xv.copy_(lx)
            wbuf = torch.zeros(lw.numel() + 32, dtype=lw.dtype, device=DEV)
            wv = wbuf[wo:wo + lw.numel()].view(3, 3, C)
            wv.copy_(lw)
            ybuf = torch.full((want.numel() + 32,), 77, dtype=want.dtype, device=DEV)
            yv = ybuf[16 + yo:16 + yo + want.numel()].view(2, 5, 4, C).permute(0, 3, 1, 2)
            assert xv.data_ptr() % 16 == xo and wv.data_ptr() % 16 == wo and yv.data_ptr() % 16 == yo
            got = dwconv_w8_levels_q(xv, dev[0], dev[1], wv, dev[2], dev[3], dev[4], *geo, dev[5], dev[6], *rng, act, mid, out=yv)
            assert got.data_ptr() == yv.data_ptr()
            _same(got, want, (C, xo, wo, yo))
            guard = torch.cat([ybuf[:16 + yo], ybuf[16 + yo + want.numel():]])
            assert bool((guard == 77).all()), (C, xo, wo, yo)
            # floats out: y at an element offset that is no multiple of 16 bytes
            fbuf = torch.full((wantf.numel() + 16,), 3.0, dtype=mid, device=DEV)
            fv = fbuf[8 + yo:8 + yo + wantf.numel()].view(2, 5, 4, C).permute(0, 3, 1, 2)
            _same(dwconv_w8_levels(xv, dev[0], dev[1], wv, dev[2], dev[3], dev[4], *geo, act, mid, out=fv), wantf, (C, xo, wo, yo))
            assert bool((torch.cat([fbuf[:8 + yo], fbuf[8 + yo + wantf.numel():]]) == 3.0).all()), (C, xo, wo, yo)


@pytest.mark.parametrize("geometry", D.GEOMETRIES, ids=D.geom_id)
def test_the_padding_byte_independently_of_the_cpu_path(geometry):
    B, C, H, Wd, k, st, p, d = geometry
    geo = (list(st), list(p), list(d))
    OH, OW = D.out_hw(geometry)
    for x_dt, zx, w_dt in ((torch.uint8, 200, torch.int8), (torch.int8, -100, torch.uint8), (torch.uint8, 0, torch.uint8), (torch.int8, 126, torch.int8)):
        lw, s_w, zw = D.dw_weight(C, k, w_dt, 4)
        s, z = W.act(0.0371, zx)
        bias = W.random_bias(C, torch.float32, 2)
        # x all zx: I = 0 inside and in the padding alike, v = bias exactly, whatever the weights
        lx = torch.full((B, C, H, Wd), zx, dtype=x_dt).contiguous(memory_format=CL)
        osc, osh, rng = torch.tensor([0.01]), torch.tensor([-1.28]), (0, 255, 0, 255)
        got = OPS.lsq_dwconv2d_w8_q8_q(*R.to(DEV, lx, s, z, lw, s_w, zw, bias), *geo, *R.to(DEV, osc, osh), *rng, 0, torch.float32).cpu()
        want = torch.from_numpy(D.numpy_levels(bias.numpy(), osc, osh, rng)).reshape(1, C, 1, 1).expand(B, C, OH, OW)
        assert torch.equal(got.to(torch.int64), want) and len(got.unique()) > 8, (geometry, x_dt, zx)
        # x all zx + 1 on weights all zw + 1, scales powers of two: v is the number of taps inside x, exactly
        zw1 = torch.randint(W.LEVEL_RANGE[w_dt][0], W.LEVEL_RANGE[w_dt][1], (C,), generator=torch.Generator().manual_seed(3)).to(torch.int32)
        lw1 = (zw1 + 1).to(w_dt).reshape(1, 1, C).expand(k[0], k[1], C).contiguous()
        lx1 = torch.full((B, C, H, Wd), zx + 1, dtype=x_dt).contiguous(memory_format=CL)
        s1, _ = W.act(0.25, zx)
        f = OPS.lsq_dwconv2d_w8_q8(*R.to(DEV, lx1, s1, z, lw1, torch.full((C,), 4.0), zw1, None), *geo, 0, torch.float32).cpu()
        count = F.conv2d(torch.ones(1, 1, H, Wd), torch.ones(1, 1, *k), None, st, p, d)
        assert torch.equal(f, count.expand(B, C, OH, OW)) and (max(p) == 0 or count.min() < count.max()), (geometry, x_dt, zx)


@pytest.mark.parametrize("geometry", D.GEOMETRIES[:4], ids=D.geom_id)
def test_gpu_is_the_existing_gpu_ops_composed_through_the_dense_embedding(geometry):
    for variant, out_variant in zip(D.VARIANTS, ((True, torch.bfloat16, 2), (False, torch.float32, 1), (None, torch.float16, 2), (True, torch.float16, 0),
                                                 (None, torch.bfloat16, 1))):
        c = D.case(geometry, variant, out_variant, 11)
        got, want = D.run(c, DEV), D.composed(c, DEV)
        assert got.dtype == want.dtype and torch.equal(D.bits(got), D.bits(want)), (geometry, variant, out_variant)


def test_launches_repeat_and_an_output_depends_on_its_own_image_alone():
    for g in ((3, 32, 14, 14, (3, 3), (1, 1), (1, 1), (1, 1)), (3, 32, 14, 14, (3, 3), (2, 2), (1, 1), (1, 1)), (3, 32, 14, 14, (5, 5), (1, 1), (2, 2), (1, 1)),
              (3, 20, 14, 14, (3, 3), (1, 1), (1, 1), (1, 1))):
        c = D.case(g, D.VARIANTS[0], (True, torch.bfloat16, 2), 8)
        D.assert_conditions(D.run(c), c, g)
        dev = R.to(DEV, *c[:7]) + list(c[7:8]) + R.to(DEV, c[8], c[9]) + list(c[10:])
        first = D.run(tuple(dev))
        for _ in range(3):
            assert torch.equal(D.run(tuple(dev)), first), g
        other = dev[0].clone()
        other[0] = 255 - other[0]
        other[2] = 0
        again = D.run((other,) + tuple(dev[1:]))
        assert torch.equal(again[1], first[1]) and not torch.equal(again[0], first[0]), g
        assert torch.equal(D.run((dev[0][1:2],) + tuple(dev[1:]))[0], first[1]), g


def test_a_grid_of_many_workgroups():
    g = (8, 64, 34, 34, (3, 3), (1, 1), (1, 1), (1, 1))
    pl = _plan(g)
    assert pl["family"] == "packets" and pl["grid"] == -(-(8 * 34 * -(-34 // pl["pixels_per_lane"]) * 4) // 256) and pl["grid"] > 128
    c = D.case(g, D.VARIANTS[1], (True, torch.bfloat16, 2), 13)
    want = D.run(c)
    D.assert_conditions(want, c, g)
    _same(D.run(c, DEV), want, g)


@pytest.mark.parametrize("mid", R.MIDS, ids=lambda v: str(v).replace("torch.", ""))
def test_the_converted_inverted_residual_block_in_a_graph(mid):
    from torchlsq.functional import LevelsTensor
    net, qs, x = D.inverted_residual()
    new = D.convert_inverted_residual(net, qs, mid)
    xl = LevelsTensor.from_quantized(qs["in"].quantize(x))
    want = new(xl).levels
    other = LevelsTensor.from_quantized(qs["in"].quantize(x.flip(0) * 0.5 + 0.1))
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
