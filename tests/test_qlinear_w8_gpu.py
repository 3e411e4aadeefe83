"""GPU: the W8A8 linear op on per-channel 8-bit weight levels (include/lsq_hip_qlinear_w8.h, liblsq_hip_qlinear_w8.so,
torch.ops.torchlsq.lsq_linear_w8_q8 / lsq_linear_w8_a8, torchlsq.quantized.LinearW8A8 / convert_w8a8) on the MI355X.

The contract defines the result bit for bit (an exact integer, then four rounded fp32 steps), so every comparison here is
`torch.equal` on the bits against the package's CPU path -- which tests/test_qlinear_w8_cpu.py holds to the float64
reference within the derived bound -- or against the exact integer itself.  No tolerance appears in this file.
"""
import pytest
import torch

import qlinear_cases as C
import qlinear_w8_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (5, 17, 67)
KS = (64, 80, 4160)
_id = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))


def bits(t):
    return t.detach().cpu().contiguous().view(C.INT[t.dtype])


def dev(*tensors):
    return [None if t is None else t.to(DEV) for t in tensors]


def q8(lx, s_x, zx, lw, s_w, zw, bias, dtype):
    s, z = W.act(s_x, zx, lx.device)
    return torch.ops.torchlsq.lsq_linear_w8_q8(lx, s, z, lw, s_w, zw, bias, dtype)


def row_counts(N, K):
    """1, 2, 15, 16, 17, 33, 129 and both sides of every M at which the plan changes its launch shape"""
    from torchlsq import extension as E
    ms = {1, 2, 15, 16, 17, 33, 129}
    for t in W.plan_row_thresholds(E.qlinear_w8_plan, N, K):
        ms |= {t - 1, t}
    return sorted(ms)


def test_the_plan_changes_its_launch_shape_where_the_cases_expect_it():
    from torchlsq import extension as E
    for N in NS:
        for K in KS:
            ts = W.plan_row_thresholds(E.qlinear_w8_plan, N, K)
            assert 17 in ts and len(ts) >= 2, (N, K, ts)
            shapes = {E.qlinear_w8_plan(M, N, K)["shape"] for M in row_counts(N, K)}
            assert {"decode", "tiles_split_k"} <= shapes and "generic" not in shapes


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_levels_form_equals_the_cpu_path_bit_for_bit(N, K):
    """every row count of row_counts(), both level types on both sides, zero points at and off the borders, three output
    types, bias none / float32 / y's type"""
    variants = [(torch.uint8, 3, torch.int8, (-7, 127), torch.float32, "f32"),
                (torch.uint8, 125, torch.uint8, (0, 255, 131), torch.bfloat16, "y"),
                (torch.int8, -128, torch.int8, (-128, 5), torch.float16, None),
                (torch.int8, 127, torch.uint8, (7, 200), torch.float32, None)]
    seed = N * 7 + K
    for x_dt, zx, w_dt, zeros, y_dt, bias_kind in variants:
        lw, s_w, zw = W.weight(N, K, w_dt, seed, zeros)
        bias = None if bias_kind is None else W.random_bias(N, torch.float32 if bias_kind == "f32" else y_dt, seed)
        lo, hi = W.LEVEL_RANGE[x_dt]
        lx_all = W.levels((129, K), lo, hi, seed)
        want_all = q8(lx_all, 0.0371, zx, lw, s_w, zw, bias, y_dt)               # the CPU path, once: rows are independent
        r, E = W.reference(lx_all, torch.tensor(0.0371, dtype=torch.float32).item(), zx, lw, s_w, zw, bias)
        C.assert_within_bound(want_all, r, E, y_dt, "cpu path N=%d K=%d" % (N, K))
        glw, gs, gz, gb = dev(lw, s_w, zw, bias)
        for M in row_counts(N, K):
            got = q8(lx_all[:M].to(DEV), 0.0371, zx, glw, gs, gz, gb, y_dt)
            assert got.shape == (M, N) and torch.equal(bits(got), bits(want_all[:M])), (M, x_dt, w_dt, y_dt)
        seed += 1


@pytest.mark.parametrize("dtype", C.DTYPES, **_id)
@pytest.mark.parametrize("K", KS)
def test_fused_form_equals_the_cpu_path_and_the_levels_form_bit_for_bit(dtype, K):
    """floating x of three types with NaN, +-inf, -0.0, both borders and a tie; an unsigned and a signed activation range"""
    N = 17
    for rng, scale, shift in (((0, 127, 0, 255), 0.05, -3.0), ((-128, 127, -128, 127), 0.03, 0.4)):
        qmin, qmax, tmin, tmax = rng
        lw, s_w, zw = W.weight(N, K, torch.int8, K, (-7, 127))
        bias = W.random_bias(N, dtype, K)
        x = W.special_x(129, K, dtype, scale, shift, qmin, qmax, seed=K)
        sc, sh = torch.tensor([scale]), torch.tensor([shift])
        want = torch.ops.torchlsq.lsq_linear_w8_a8(x, sc, sh, qmin, qmax, tmin, tmax, lw, s_w, zw, bias)
        gx, gsc, gsh, glw, gs, gz, gb = dev(x, sc, sh, lw, s_w, zw, bias)
        lv = torch.ops.torchlsq.lsq_levels_per_tensor(gx, gsc, gsh, qmin, qmax, tmin, tmax, 0)
        lv = lv.view(torch.uint8) if tmax > 127 else lv
        s_x = gsc.abs().clamp_min(torch.finfo(torch.float32).eps)
        zx = torch.fmin(torch.full_like(s_x, tmax), torch.fmax(torch.full_like(s_x, tmin), -gsh * (1.0 / s_x))).round().to(torch.int32)
        for M in row_counts(N, K):
            got = torch.ops.torchlsq.lsq_linear_w8_a8(gx[:M], gsc, gsh, qmin, qmax, tmin, tmax, glw, gs, gz, gb)
            assert torch.equal(bits(got), bits(want[:M])), (M, rng)
            if M in (1, 16, 17, 129):
                by_levels = torch.ops.torchlsq.lsq_linear_w8_q8(lv[:M], s_x, zx, glw, gs, gz, gb, dtype)
                assert torch.equal(bits(got), bits(by_levels)), (M, rng)


def test_wide_tiles_equal_the_cpu_path_bit_for_bit():
    """the 64-column tiles, which the plan takes once they give every compute unit one: many rows on a narrow weight (8
    sub-tiles) and few rows on a very wide, very short one (2 and 4 sub-tiles); the sizes are read from the plan"""
    from torchlsq import extension as E
    plan = E.qlinear_w8_plan
    cases = []
    row_tiles = next(t for t in range(1, 4097) if plan(128 * t, 67, 80)["shape"] == "tiles")
    assert plan(128 * (row_tiles - 1), 67, 80)["shape"] == "tiles_split_k"
    cases.append((128 * (row_tiles - 1) + 1, 67, 80))
    col_tiles = next(t for t in range(1, 4097) if plan(20, 64 * t, 16)["shape"] == "tiles")
    cases += [(20, 64 * (col_tiles - 1) + 1, 16), (50, 64 * (col_tiles - 1) + 1, 16)]
    for M, N, K in cases:
        pl = plan(M, N, K)
        assert pl["shape"] == "tiles" and pl["cols_per_tile"] == 64 and pl["k_split"] == 1, (M, N, K, pl)
        lw, s_w, zw = W.weight(N, K, torch.uint8, M, (0, 255, 131))
        bias = W.random_bias(N, torch.float32, M)
        lx = W.levels((M, K), -128, 127, M)
        want = q8(lx, 0.0371, -3, lw, s_w, zw, bias, torch.bfloat16)
        got = q8(lx.to(DEV), 0.0371, -3, *dev(lw, s_w, zw, bias), torch.bfloat16)
        assert torch.equal(bits(got), bits(want)), (M, N, K)


def test_the_integer_sum_beyond_32_bits():
    """N = 16, K = 33040, all x levels 255 with zx = 0, all w levels -128 with zw = 127: I = -255 * 255 * 33040 < -2^31; with
    power-of-two scales y is exact.  And a random case at that K."""
    from torchlsq import extension as E
    N, K = 16, 33040
    assert E.qlinear_w8_plan(3, N, K)["form"] == "mfma"
    lw = torch.full((N, K), -128, dtype=torch.int8)
    s_w = torch.full((N,), 2.0 ** -9)
    zw = torch.full((N,), 127, dtype=torch.int32)
    for M in (3, 40):
        lx = torch.full((M, K), 255, dtype=torch.uint8)
        I = W.exact_I(lx, 0, lw, zw)
        assert int(I[0, 0]) == -255 * 255 * 33040 < -2 ** 31
        got = q8(lx.to(DEV), 2.0 ** -7, 0, *dev(lw, s_w, zw), None, torch.float32)
        want = (I.double() * 2.0 ** -16).float()                               # one rounding: that of float(I)
        assert torch.equal(bits(got), bits(want)), M
        lwr, swr, zwr = W.weight(N, K, torch.uint8, 5, (0, 255))
        lxr = W.levels((M, K), -128, 127, 6)
        want = q8(lxr, 0.02, -128, lwr, swr, zwr, None, torch.float32)
        got = q8(lxr.to(DEV), 0.02, -128, *dev(lwr, swr, zwr), None, torch.float32)
        assert torch.equal(bits(got), bits(want)), M


def test_generic_form_equals_the_cpu_path_bit_for_bit():
    """K = 72 (no multiple of 16), and a weight view at a byte offset of 1"""
    from torchlsq import extension as E
    assert E.qlinear_w8_plan(5, 17, 72)["form"] == "generic" and E.qlinear_w8_plan(5, 17, 80, w_aligned=False)["form"] == "generic"
    for K, offset in ((72, 0), (80, 1)):
        for M in (1, 5, 19):
            for w_dt, x_dt, zx, y_dt in ((torch.int8, torch.uint8, 125, torch.float32), (torch.uint8, torch.int8, -3, torch.bfloat16)):
                lw, s_w, zw = W.weight(17, K, w_dt, K + M, (-7 if w_dt == torch.int8 else 7, 127))
                bias = W.random_bias(17, torch.float32, K)
                lx = W.levels((M, K), *W.LEVEL_RANGE[x_dt], seed=M)
                want = q8(lx, 0.04, zx, lw, s_w, zw, bias, y_dt)
                flat = torch.zeros(17 * K + 16, dtype=w_dt, device=DEV)
                view = flat[offset:offset + 17 * K].view(17, K)
                view.copy_(lw)
                assert view.data_ptr() % 16 == offset and view.is_contiguous()
                got = q8(lx.to(DEV), 0.04, zx, view, *dev(s_w, zw, bias), y_dt)
                assert torch.equal(bits(got), bits(want)), (K, offset, M)
                sc, sh = torch.tensor([0.05]), torch.tensor([-3.0])
                x = W.special_x(M, K, torch.float16, 0.05, -3.0, 0, 127, seed=M)
                want = torch.ops.torchlsq.lsq_linear_w8_a8(x, sc, sh, 0, 127, 0, 255, lw, s_w, zw, None)
                got = torch.ops.torchlsq.lsq_linear_w8_a8(*dev(x, sc, sh), 0, 127, 0, 255, view, *dev(s_w, zw), None)
                assert torch.equal(bits(got), bits(want)), (K, offset, M, "fused")


def test_row_invariance_and_repeatability():
    N, K = 67, 4160
    lw, s_w, zw = W.weight(N, K, torch.int8, 11, (-7, 127))
    bias = W.random_bias(N, torch.bfloat16, 11)
    glw, gs, gz, gb = dev(lw, s_w, zw, bias)
    lx = W.levels((129, K), 0, 255, 12).to(DEV)
    big = q8(lx, 0.0371, 125, glw, gs, gz, gb, torch.bfloat16)
    again = q8(lx, 0.0371, 125, glw, gs, gz, gb, torch.bfloat16)
    assert torch.equal(bits(big), bits(again))                                  # two launches, the same bits
    for m in (0, 15, 16, 77, 128):                                             # row m of the 129-row call == the 1-row call
        one = q8(lx[m:m + 1], 0.0371, 125, glw, gs, gz, gb, torch.bfloat16)
        assert torch.equal(bits(one), bits(big[m:m + 1])), m
    same = lx.clone()
    same[0], same[16], same[128] = lx[5], lx[5], lx[5]                          # one row at positions 0, 16 and 128
    y = q8(same, 0.0371, 125, glw, gs, gz, gb, torch.bfloat16)
    assert torch.equal(bits(y[0]), bits(y[16])) and torch.equal(bits(y[0]), bits(y[128])) and torch.equal(bits(y[0]), bits(big[5]))
    wide = torch.zeros(129, 2 * K, dtype=torch.uint8, device=DEV)               # a non-contiguous view of x
    wide[:, ::2] = lx
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert torch.equal(bits(q8(view, 0.0371, 125, glw, gs, gz, gb, torch.bfloat16)), bits(big))
    assert torch.equal(bits(q8(view[:3], 0.0371, 125, glw, gs, gz, gb, torch.bfloat16)), bits(big[:3]))


@pytest.mark.parametrize("K", (64, 80))
def test_asymmetric_integer_data_pins_the_mfma_lane_maps(K):
    """lw[n, k] = (3 n + 5 k) mod 251 - 125, lx[m, k] = (7 m + 11 k) mod 256, scales 1, zero points 0, fp32 y: |I| < 2^24, so y is
    the exact integer matrix -- any wrong pairing of a lane's k with another's, or a wrong row / column of D, shows"""
    for N, M in ((16, 16), (67, 129), (17, 3), (67, 40)):
        n, k, m = torch.arange(N).reshape(-1, 1), torch.arange(K).reshape(1, -1), torch.arange(M).reshape(-1, 1)
        lw = ((3 * n + 5 * k) % 251 - 125).to(torch.int8)
        lx = ((7 * m + 11 * k) % 256).to(torch.uint8)
        I = lx.to(torch.int64) @ lw.to(torch.int64).t()
        assert int(I.abs().max()) < 2 ** 24
        got = q8(lx.to(DEV), 1.0, 0, *dev(lw, torch.ones(N), torch.zeros(N, dtype=torch.int32)), None, torch.float32)
        assert torch.equal(got.cpu(), I.float()), (N, M)


def test_graph_capture_and_replay():
    N, K = 67, 80
    lw, s_w, zw = W.weight(N, K, torch.int8, 21, (-7, 127))
    glw, gs, gz = dev(lw, s_w, zw)
    s, z = W.act(0.0371, 125, DEV)
    static_lx = W.levels((33, K), 0, 255, 22).to(DEV)
    static_x = torch.randn(3, K, device=DEV, dtype=torch.bfloat16)
    sc, sh = torch.tensor([0.05], device=DEV), torch.tensor([-3.0], device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                              # warm-up outside the capture
        torch.ops.torchlsq.lsq_linear_w8_q8(static_lx, s, z, glw, gs, gz, None, torch.float32)
        torch.ops.torchlsq.lsq_linear_w8_a8(static_x, sc, sh, 0, 127, 0, 255, glw, gs, gz, None)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y1 = torch.ops.torchlsq.lsq_linear_w8_q8(static_lx, s, z, glw, gs, gz, None, torch.float32)
        y2 = torch.ops.torchlsq.lsq_linear_w8_a8(static_x, sc, sh, 0, 127, 0, 255, glw, gs, gz, None)
    new_lx = W.levels((33, K), 0, 255, 23)
    new_x = torch.randn(3, K).to(torch.bfloat16)
    static_lx.copy_(new_lx)
    static_x.copy_(new_x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(y1), bits(q8(new_lx, 0.0371, 125, lw, s_w, zw, None, torch.float32)))
    want = torch.ops.torchlsq.lsq_linear_w8_a8(new_x, sc.cpu(), sh.cpu(), 0, 127, 0, 255, lw, s_w, zw, None)
    assert torch.equal(bits(y2), bits(want))


def test_module_and_convert_on_the_gpu_equal_the_cpu_module_bit_for_bit():
    from torchlsq.quantized import LinearW8A8, convert_w8a8
    model, in_q, mid_q = W.qat_model()
    conv = convert_w8a8(model, {"0": in_q, "2": mid_q})
    assert [type(m).__name__ for m in conv] == ["LinearW8A8", "ReLU", "LinearW8A8"]
    gconv = convert_w8a8(model, {"0": in_q, "2": mid_q}).to(DEV)
    for M in (5, 40):
        x = torch.randn(M, 64)
        with torch.no_grad():
            want, got = conv(x), gconv(x.to(DEV))
        assert got.is_cuda and torch.equal(bits(got), bits(want)), M
    layer = LinearW8A8.from_float(model[0], in_q)
    glayer = LinearW8A8.from_float(model[0], in_q).to(DEV)
    x = torch.randn(19, 64)
    with torch.no_grad():
        assert torch.equal(bits(glayer(x.to(DEV))), bits(layer(x)))
        xq = in_q.quantize(x)                                                   # a quantized tensor in: the levels form
        gq = torch._make_per_tensor_quantized_tensor(xq.int_repr().to(DEV), xq.q_scale(), xq.q_zero_point())
        assert torch.equal(bits(glayer(gq)), bits(layer(xq)))
        assert torch.equal(bits(layer(xq)), bits(layer(x)))
