"""GPU: the W8A8 conv2d op on channels-last 8-bit levels (include/lsq_hip_qconv_w8.h, liblsq_hip_qconv_w8.so,
torch.ops.torchlsq.lsq_conv2d_w8_q8 / lsq_conv2d_w8_a8, torchlsq.quantized.Conv2dW8A8 / convert_w8a8) on the MI355X.

The contract defines the result bit for bit (an exact integer, then four rounded fp32 steps), so every comparison here is
`torch.equal` on the bits against the package's CPU path -- which tests/test_qconv_w8_cpu.py holds to the float64 reference
within the derived bound and to an independent restatement of the integers -- or against a known integer.  No tolerance
appears in this file.
"""
import pytest
import torch

import qconv_w8_cases as V
import qlinear_cases as C
import qlinear_w8_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last


def bits(t):
    return t.detach().cpu().contiguous().view(C.INT[t.dtype])


def dev(*tensors):
    return [None if t is None else t.to(DEV) for t in tensors]


def q8(lx, s_x, zx, lw, s_w, zw, bias, stride, padding, dilation, dtype):
    s, z = W.act(s_x, zx, lx.device)
    return torch.ops.torchlsq.lsq_conv2d_w8_q8(lx, s, z, lw, s_w, zw, bias, list(stride), list(padding), list(dilation), dtype)


def both(lx, s_x, zx, lw, s_w, zw, bias, s, p, d, dtype, note):
    """the op on the CPU and on the GPU: equal bits, the right shape, channels-last; returns the GPU result"""
    want = q8(lx, s_x, zx, lw, s_w, zw, bias, s, p, d, dtype)
    got = q8(*dev(lx), s_x, zx, *dev(lw, s_w, zw, bias), s, p, d, dtype)
    assert got.is_cuda and got.shape == want.shape and got.dtype == dtype and got.is_contiguous(memory_format=CL), note
    assert torch.equal(bits(got), bits(want)), note
    return got


def plan_of(geometry, aligned=True):
    from torchlsq import extension as E
    B, Cin, H, Wd, N, k, s, p, d = geometry
    return E.qconv_w8_plan(B, Cin, H, Wd, N, k, s, p, d, aligned)


@pytest.mark.parametrize("geometry", V.GEOMETRIES, ids=V.geom_id)
def test_levels_form_equals_the_cpu_path_bit_for_bit(geometry):
    """both level types on both sides, zero points at and off the borders, three output types, bias none / float32 / y's type"""
    B, Cin, H, Wd, N, k, s, p, d = geometry
    assert plan_of(geometry)["form"] == "mfma"
    for i, (x_dt, zx, w_dt, zeros, y_dt, bias_kind) in enumerate(V.VARIANTS):
        lw, s_w, zw = V.conv_weight(N, Cin, k, w_dt, B + Cin + i, zeros)
        bias = None if bias_kind is None else W.random_bias(N, torch.float32 if bias_kind == "f32" else y_dt, i)
        lx = V.x_levels(B, Cin, H, Wd, x_dt, seed=H + i)
        both(lx, 0.0371, zx, lw, s_w, zw, bias, s, p, d, y_dt, (V.geom_id(geometry), i))


def test_row_counts_on_both_sides_of_every_plan_threshold():
    """a padded 3 x 3 convolution on images of M = 1, 15, 16, 17 pixels and of both sides of every M at which the plan changes,
    each over every variant"""
    from torchlsq import extension as E
    Cin, N = 16, 17
    ms = V.plan_row_counts(lambda M: E.qconv_w8_plan(1, Cin, 1, M, N, 3, 1, 1))
    assert {32, 33, 64, 65} <= set(ms)
    subs = set()
    for M in ms:
        B, H, Wd = V.image_of(M)
        pl = E.qconv_w8_plan(B, Cin, H, Wd, N, 3, 1, 1)
        assert pl["M"] == M and pl["form"] == "mfma"
        subs.add(pl["rows_per_tile"])
        for i, (x_dt, zx, w_dt, zeros, y_dt, bias_kind) in enumerate(V.VARIANTS):
            lw, s_w, zw = V.conv_weight(N, Cin, (3, 3), w_dt, M + i, zeros)
            bias = None if bias_kind is None else W.random_bias(N, torch.float32 if bias_kind == "f32" else y_dt, M)
            both(V.x_levels(B, Cin, H, Wd, x_dt, seed=M), 0.0371, zx, lw, s_w, zw, bias, (1, 1), (1, 1), (1, 1), y_dt, (M, i))
    assert subs == {32, 64, 128}


def test_wide_tiles_equal_the_cpu_path_bit_for_bit():
    """the 64-column tiles, which the plan takes once they give every compute unit one, at 8, 2 and 4 sub-tiles: many pixels on
    a 3 x 3 convolution (K = 144), few pixels on a very wide 1 x 1 one; the sizes are read from the plan"""
    from torchlsq import extension as E
    plan = E.qconv_w8_plan
    cases = []
    B, H, Wd = 1, 41, 47                                                    # M = 1927: 16 row tiles of 128, the last one short
    col_tiles = next(t for t in range(1, 4097) if plan(B, 16, H, Wd, 64 * t, 3, 1, 1)["shape"] == "tiles")
    assert plan(B, 16, H, Wd, 64 * (col_tiles - 1), 3, 1, 1)["shape"] == "tiles_split_k"
    cases.append(((B, 16, H, Wd, 64 * (col_tiles - 1) + 1, (3, 3), (1, 1), (1, 1), (1, 1)), 128))
    col_tiles = next(t for t in range(1, 4097) if plan(1, 16, 4, 5, 64 * t, 1)["shape"] == "tiles")
    cases.append(((1, 16, 4, 5, 64 * (col_tiles - 1) + 1, (1, 1), (1, 1), (0, 0), (1, 1)), 32))
    cases.append(((2, 16, 5, 5, 64 * (col_tiles - 1) + 1, (1, 1), (1, 1), (0, 0), (1, 1)), 64))
    for geometry, rows in cases:
        B, Cin, H, Wd, N, k, s, p, d = geometry
        pl = plan_of(geometry)
        assert pl["shape"] == "tiles" and pl["cols_per_tile"] == 64 and pl["k_split"] == 1 and pl["rows_per_tile"] == rows, (geometry, pl)
        lw, s_w, zw = V.conv_weight(N, Cin, k, torch.uint8, H, (0, 255, 131))
        bias = W.random_bias(N, torch.float32, H)
        both(V.x_levels(B, Cin, H, Wd, torch.int8, seed=H), 0.0371, -3, lw, s_w, zw, bias, s, p, d, torch.bfloat16, geometry)


@pytest.mark.parametrize("x_dt,zx", [(torch.uint8, 131), (torch.int8, -5)], ids=["uint8_zx131", "int8_zxm5"])
def test_the_padding_byte_independent_of_the_cpu_path(x_dt, zx):
    """pad 2 on a 3 x 3 convolution.  x levels all zx: every real value is 0 like the padding, so y == bias exactly (+0.0 without
    one).  x levels all zx + 1 and weight levels all zw + 1 with scales 2^-4 and 2^-6: y == Cin * (in-bounds taps of that output
    pixel) * 2^-10 exactly -- a padded tap staged as anything but the level zx shows in either"""
    B, Cin, H, Wd, N = 2, 16, 4, 5, 20
    k, s, p, d = (3, 3), (1, 1), (2, 2), (1, 1)
    oh, ow = V.out_hw(H, Wd, k, s, p, d)
    for w_dt in (torch.int8, torch.uint8):
        lw, s_w, zw = V.conv_weight(N, Cin, k, w_dt, 7, (5, 100))
        bias = W.random_bias(N, torch.float32, 3)
        lx = torch.full((B, Cin, H, Wd), zx, dtype=x_dt).contiguous(memory_format=CL)
        for b in (None, bias):
            got = q8(*dev(lx), 0.0371, zx, *dev(lw, s_w, zw, b), s, p, d, torch.float32).cpu()
            want = torch.zeros(B, N, oh, ow) if b is None else bias.reshape(1, N, 1, 1).expand(B, N, oh, ow)
            assert torch.equal(bits(got), bits(want.contiguous())), (w_dt, b is None)
        ones_w = (zw.reshape(N, 1, 1, 1) + 1).expand(N, Cin, 3, 3).to(w_dt).contiguous(memory_format=CL)
        got = q8(*dev(lx + 1), 2.0 ** -4, zx, *dev(ones_w, torch.full((N,), 2.0 ** -6), zw), None, s, p, d, torch.float32).cpu()
        taps = torch.zeros(oh, ow, dtype=torch.int64)                       # in-bounds taps per output pixel, integer arithmetic
        for y0 in range(oh):
            for x0 in range(ow):
                taps[y0, x0] = (sum(0 <= y0 * s[0] - p[0] + i * d[0] < H for i in range(3)) *
                                sum(0 <= x0 * s[1] - p[1] + j * d[1] < Wd for j in range(3)))
        assert int(taps.min()) == 1 and int(taps.max()) == 9
        want = (Cin * taps).double().mul(2.0 ** -10).float().reshape(1, 1, oh, ow).expand(B, N, oh, ow)
        assert torch.equal(bits(got), bits(want.contiguous())), w_dt


def test_one_hot_weights_pin_the_tap_order_and_the_lane_maps():
    """one nonzero weight level per output channel, at a distinct (c, i, j), on asymmetric integer x with scales 1 and zero
    points 0: y[b, n, oh, ow] is exactly the level x[b, c_n, oh s - p + i_n d, ow s - p + j_n d] (0 in the padding)"""
    B, Cin, H, Wd = 2, 32, 6, 7
    k, s, p, d = (3, 3), (2, 1), (1, 2), (1, 2)
    N = Cin * 9
    oh, ow = V.out_hw(H, Wd, k, s, p, d)
    idx = torch.arange(B * Cin * H * Wd).reshape(B, Cin, H, Wd)
    lx = ((idx * 7 + idx // 13) % 256).to(torch.uint8).contiguous(memory_format=CL)
    lw = torch.zeros(N, Cin, 3, 3, dtype=torch.int8)
    want = torch.zeros(B, N, oh, ow)
    for n in range(N):
        c, i, j = n // 9, (n % 9) // 3, n % 3
        lw[n, c, i, j] = 1
        for y0 in range(oh):
            for x0 in range(ow):
                ih, iw = y0 * s[0] - p[0] + i * d[0], x0 * s[1] - p[1] + j * d[1]
                if 0 <= ih < H and 0 <= iw < Wd:
                    want[:, n, y0, x0] = lx[:, c, ih, iw].float()
    lw = lw.contiguous(memory_format=CL)
    got = q8(*dev(lx), 1.0, 0, *dev(lw, torch.ones(N), torch.zeros(N, dtype=torch.int32)), None, s, p, d, torch.float32)
    assert torch.equal(got.cpu(), want) and len(want.unique()) > 200


def test_the_integer_sum_beyond_32_bits():
    """a 1 x 1 convolution with Cin = 33040 on a 1 x 2 image, all x levels 255 with zx = 0, all w levels -128 with zw = 127:
    I = -255 * 255 * 33040 < -2^31; with power-of-two scales y is exact.  And a random case at that K."""
    N, Cin = 16, 33040
    g = (1, Cin, 1, 2, N, (1, 1), (1, 1), (0, 0), (1, 1))
    assert plan_of(g)["form"] == "mfma" and plan_of(g)["K"] == Cin
    lw = torch.full((N, Cin, 1, 1), -128, dtype=torch.int8)
    lx = torch.full((1, Cin, 1, 2), 255, dtype=torch.uint8)
    I = -255 * 255 * 33040
    assert I < -2 ** 31
    got = q8(*dev(lx), 2.0 ** -7, 0, *dev(lw, torch.full((N,), 2.0 ** -9), torch.full((N,), 127, dtype=torch.int32)), None,
             (1, 1), (0, 0), (1, 1), torch.float32)
    want = torch.full((1, N, 1, 2), float(torch.tensor(I, dtype=torch.int64).float()) * 2.0 ** -16)     # one rounding: float(I)
    assert torch.equal(bits(got), bits(want))
    lwr, swr, zwr = V.conv_weight(N, Cin, (1, 1), torch.uint8, 5, (0, 255))
    both(V.x_levels(1, Cin, 1, 2, torch.int8, 6), 0.02, -128, lwr, swr, zwr, None, (1, 1), (0, 0), (1, 1), torch.float32, "random")


def test_generic_form_equals_the_cpu_path_bit_for_bit():
    """Cin = 3 (a 7 x 7 stride-2 stem), Cin = 24 with a 3 x 3 kernel (K = 216) and with a 2 x 2 one (K = 96: K % 16 == 0 but
    Cin % 16 != 0, so a 16-byte packet would straddle two taps), and a weight and an x at a byte offset of 1"""
    stem = (2, 3, 9, 11, 5, (7, 7), (2, 2), (3, 3), (1, 1))
    c24 = (1, 24, 5, 4, 6, (3, 3), (1, 1), (1, 1), (1, 1))
    c24k96 = (2, 24, 4, 5, 6, (2, 2), (1, 2), (1, 0), (1, 1))
    off = (2, 16, 5, 7, 17, (3, 3), (1, 1), (1, 1), (1, 1))
    assert plan_of(stem)["form"] == "generic" and plan_of(c24)["form"] == "generic"
    assert plan_of(c24k96)["form"] == "generic" and plan_of(c24k96)["K"] == 96
    assert plan_of(off)["form"] == "mfma" and plan_of(off, aligned=False)["shape"] == "generic"
    for geometry in (stem, c24, c24k96):
        B, Cin, H, Wd, N, k, s, p, d = geometry
        for i, (x_dt, zx, w_dt, zeros, y_dt, bias_kind) in enumerate(V.VARIANTS):
            lw, s_w, zw = V.conv_weight(N, Cin, k, w_dt, i, zeros)
            bias = None if bias_kind is None else W.random_bias(N, torch.float32 if bias_kind == "f32" else y_dt, i)
            both(V.x_levels(B, Cin, H, Wd, x_dt, seed=i), 0.04, zx, lw, s_w, zw, bias, s, p, d, y_dt, (geometry, i))
    B, Cin, H, Wd, N, k, s, p, d = off
    lw, s_w, zw = V.conv_weight(N, Cin, k, torch.int8, 1, (-7, 127))
    lx = V.x_levels(B, Cin, H, Wd, torch.uint8, seed=2)
    want = q8(lx, 0.04, 125, lw, s_w, zw, None, s, p, d, torch.float32)

    def at_offset(t, offset):
        """`t` (channels-last) on the GPU at a storage byte offset"""
        flat = torch.zeros(t.numel() + 16, dtype=t.dtype, device=DEV)
        view = flat[offset:offset + t.numel()].view(t.shape[0], t.shape[2], t.shape[3], t.shape[1]).permute(0, 3, 1, 2)
        view.copy_(t)
        assert view.data_ptr() % 16 == offset and view.is_contiguous(memory_format=CL)
        return view
    for wo, xo in ((1, 0), (0, 1), (1, 1)):
        got = q8(at_offset(lx, xo), 0.04, 125, at_offset(lw, wo), *dev(s_w, zw), None, s, p, d, torch.float32)
        assert torch.equal(bits(got), bits(want)), (wo, xo)
    sc, sh = torch.tensor([0.05]), torch.tensor([-3.0])                      # the fused form through the generic kernel
    B, Cin, H, Wd, N, k, s, p, d = stem
    lw, s_w, zw = V.conv_weight(N, Cin, k, torch.int8, 9, (-7, 127))
    x = W.special_x(1, B * H * Wd * Cin, torch.float16, 0.05, -3.0, 0, 127).reshape(B, H, Wd, Cin).permute(0, 3, 1, 2)     # one row: 3 columns cannot hold its 8 special values
    geo = (list(s), list(p), list(d))
    want = torch.ops.torchlsq.lsq_conv2d_w8_a8(x, sc, sh, 0, 127, 0, 255, lw, s_w, zw, None, *geo)
    got = torch.ops.torchlsq.lsq_conv2d_w8_a8(*dev(x, sc, sh), 0, 127, 0, 255, *dev(lw, s_w, zw), None, *geo)
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda v: str(v).replace("torch.", ""))
def test_fused_form_equals_the_cpu_path_and_the_levels_form_bit_for_bit(dtype):
    """floating x of three types with NaN, +-inf, -0.0, both borders and a tie; an unsigned and a signed activation range;
    channels-last and NCHW x give equal bits"""
    B, Cin, H, Wd, N = 2, 16, 5, 7, 17
    geo = ([2, 1], [1, 2], [1, 2])
    for rng, scale, shift in (((0, 127, 0, 255), 0.05, -3.0), ((-128, 127, -128, 127), 0.03, 0.4)):
        qmin, qmax, tmin, tmax = rng
        lw, s_w, zw = V.conv_weight(N, Cin, (3, 3), torch.int8, 5, (-7, 127))
        bias = W.random_bias(N, dtype, 5)
        x = W.special_x(B * H * Wd, Cin, dtype, scale, shift, qmin, qmax, seed=3).reshape(B, H, Wd, Cin).permute(0, 3, 1, 2)
        sc, sh = torch.tensor([scale]), torch.tensor([shift])
        want = torch.ops.torchlsq.lsq_conv2d_w8_a8(x, sc, sh, qmin, qmax, tmin, tmax, lw, s_w, zw, bias, *geo)
        gx, gsc, gsh, glw, gs, gz, gb = dev(x, sc, sh, lw, s_w, zw, bias)
        got = torch.ops.torchlsq.lsq_conv2d_w8_a8(gx, gsc, gsh, qmin, qmax, tmin, tmax, glw, gs, gz, gb, *geo)
        assert got.dtype == dtype and got.is_contiguous(memory_format=CL) and torch.equal(bits(got), bits(want)), rng
        lv = torch.ops.torchlsq.lsq_levels_per_tensor(gx, gsc, gsh, qmin, qmax, tmin, tmax, 0)
        lv = lv.view(torch.uint8) if tmax > 127 else lv
        s_x = gsc.abs().clamp_min(torch.finfo(torch.float32).eps)
        zx = torch.fmin(torch.full_like(s_x, tmax), torch.fmax(torch.full_like(s_x, tmin), -gsh * (1.0 / s_x))).round().to(torch.int32)
        by_levels = torch.ops.torchlsq.lsq_conv2d_w8_q8(lv, s_x, zx, glw, gs, gz, gb, *geo, dtype)
        assert torch.equal(bits(got), bits(by_levels)), rng
        nchw = gx.contiguous()
        assert not nchw.is_contiguous(memory_format=CL)
        assert torch.equal(bits(torch.ops.torchlsq.lsq_conv2d_w8_a8(nchw, gsc, gsh, qmin, qmax, tmin, tmax, glw.contiguous(), gs, gz, gb, *geo)),
                           bits(got)), rng


def test_image_independence_and_repeatability():
    B, Cin, H, Wd, N = 5, 16, 6, 7, 67
    k, s, p, d = (3, 3), (1, 2), (1, 1), (2, 1)
    lw, s_w, zw = V.conv_weight(N, Cin, k, torch.int8, 11, (-7, 127))
    bias = W.random_bias(N, torch.bfloat16, 11)
    glw, gs, gz, gb = dev(lw, s_w, zw, bias)
    lx = V.x_levels(B, Cin, H, Wd, torch.uint8, 12).to(DEV)
    big = q8(lx, 0.0371, 125, glw, gs, gz, gb, s, p, d, torch.bfloat16)
    again = q8(lx, 0.0371, 125, glw, gs, gz, gb, s, p, d, torch.bfloat16)
    assert torch.equal(bits(big), bits(again))                                  # two launches, the same bits
    for b in range(B):                                                         # image b alone == its slice of the batched call
        one = q8(lx[b:b + 1], 0.0371, 125, glw, gs, gz, gb, s, p, d, torch.bfloat16)
        assert torch.equal(bits(one), bits(big[b:b + 1])), b
    nchw = lx.contiguous()                                                      # an NCHW x: copied channels-last by the host layer
    assert torch.equal(bits(q8(nchw, 0.0371, 125, glw.contiguous(), gs, gz, gb, s, p, d, torch.bfloat16)), bits(big))


def test_graph_capture_and_replay():
    B, Cin, H, Wd, N = 2, 16, 5, 7, 17
    k, s, p, d = (3, 3), (1, 1), (1, 1), (1, 1)
    geo = (list(s), list(p), list(d))
    lw, s_w, zw = V.conv_weight(N, Cin, k, torch.int8, 21, (-7, 127))
    glw, gs, gz = dev(lw, s_w, zw)
    sx, z = W.act(0.0371, 125, DEV)
    static_lx = V.x_levels(B, Cin, H, Wd, torch.uint8, 22).to(DEV)
    static_x = torch.randn(B, Cin, H, Wd, device=DEV, dtype=torch.bfloat16).contiguous(memory_format=CL)
    sc, sh = torch.tensor([0.05], device=DEV), torch.tensor([-3.0], device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                              # warm-up outside the capture
        torch.ops.torchlsq.lsq_conv2d_w8_q8(static_lx, sx, z, glw, gs, gz, None, *geo, torch.float32)
        torch.ops.torchlsq.lsq_conv2d_w8_a8(static_x, sc, sh, 0, 127, 0, 255, glw, gs, gz, None, *geo)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y1 = torch.ops.torchlsq.lsq_conv2d_w8_q8(static_lx, sx, z, glw, gs, gz, None, *geo, torch.float32)
        y2 = torch.ops.torchlsq.lsq_conv2d_w8_a8(static_x, sc, sh, 0, 127, 0, 255, glw, gs, gz, None, *geo)
    new_lx = V.x_levels(B, Cin, H, Wd, torch.uint8, 23)
    new_x = torch.randn(B, Cin, H, Wd).to(torch.bfloat16).contiguous(memory_format=CL)
    static_lx.copy_(new_lx)
    static_x.copy_(new_x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(y1), bits(q8(new_lx, 0.0371, 125, lw, s_w, zw, None, s, p, d, torch.float32)))
    want = torch.ops.torchlsq.lsq_conv2d_w8_a8(new_x, sc.cpu(), sh.cpu(), 0, 127, 0, 255, lw, s_w, zw, None, *geo)
    assert torch.equal(bits(y2), bits(want))


def test_module_and_convert_on_the_gpu_equal_the_cpu_module_bit_for_bit():
    from torchlsq.quantized import Conv2dW8A8, convert_w8a8
    model, in_q, mid_q = V.qat_conv_model()
    conv = convert_w8a8(model, {"0": in_q, "2": mid_q})
    assert [type(m).__name__ for m in conv] == ["Conv2dW8A8", "ReLU", "Conv2dW8A8"]
    gconv = convert_w8a8(model, {"0": in_q, "2": mid_q}).to(DEV)
    assert gconv[0].weight_levels.is_cuda and gconv[0].weight_levels.is_contiguous(memory_format=CL)
    for B in (1, 6):
        x = torch.randn(B, 16, 7, 7)
        with torch.no_grad():
            want, got = conv(x), gconv(x.to(DEV))
        assert got.is_cuda and got.shape == (B, 4, 3, 3) and torch.equal(bits(got), bits(want)), B
    layer = Conv2dW8A8.from_float(model[0], in_q)
    glayer = Conv2dW8A8.from_float(model[0], in_q).to(DEV)
    x = torch.randn(3, 16, 7, 7)
    with torch.no_grad():
        assert torch.equal(bits(glayer(x.to(DEV))), bits(layer(x)))
        xq = in_q.quantize(x)                                                   # a quantized tensor in: the levels form
        gq = torch._make_per_tensor_quantized_tensor(xq.int_repr().to(DEV), xq.q_scale(), xq.q_zero_point())
        assert torch.equal(bits(glayer(gq)), bits(layer(xq)))
        assert torch.equal(bits(layer(xq)), bits(layer(x)))
