"""GPU: the W8A8 layers with an 8-bit output (include/lsq_hip_requant_w8.h, liblsq_hip_requant_w8.so,
torch.ops.torchlsq.lsq_linear_w8_q8_q / _a8_q, lsq_conv2d_w8_q8_q / _a8_q, torchlsq.quantized.convert_w8a8_q) on the MI355X.

The contract defines every output byte (three existing ops composed), so every comparison here is `torch.equal` on the levels:
against the package's CPU path -- which IS that composition and which tests/test_requant_w8_cpu.py holds to integers at the
rounding ties -- and against the three existing GPU ops composed.  No tolerance appears in this file.  Output quantizers come
from requant_w8_cases.out_quantizer; every random case of 336 outputs or more is held to `assert_not_vacuous` on the CPU
result, and the sweeps over small M on the union of their results per output variant.
"""
import pytest
import torch

import qconv_w8_cases as V
import qlinear_w8_cases as W
import requant_w8_cases as R
from torchlsq.functional import _act_constants

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
OPS = torch.ops.torchlsq


def dev(case):
    return [t.to(DEV) if isinstance(t, torch.Tensor) else t for t in case]


def both_linear(case, note, seen=None):
    """the op on the CPU and on the GPU: equal levels; returns the GPU result"""
    want = R.linear_q(*case)
    got = R.linear_q(*dev(case))
    assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape, note
    assert torch.equal(got.cpu(), want), note
    if want.numel() >= 336:
        R.assert_not_vacuous(want, case[9], note)
    if seen is not None:
        seen.setdefault(case[9], []).append(want.flatten())
    return got


def both_conv(case, note):
    want = R.conv_q(*case)
    got = R.conv_q(*dev(case))
    assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape and got.is_contiguous(memory_format=CL), note
    assert torch.equal(got.cpu(), want), note
    if want.numel() >= 336:
        R.assert_not_vacuous(want, case[10], note)
    return got


def union_not_vacuous(seen):
    for rng, parts in seen.items():
        R.assert_not_vacuous(torch.cat(parts), rng, rng)


@pytest.mark.parametrize("K", [144, 288])
@pytest.mark.parametrize("N", [16, 17, 64, 80])
def test_linear_tiles_equal_the_cpu_path_bit_for_bit(N, K):
    """K = 144: a tail step, 288: two steps.  N = 16 / 64: packets on full tiles, 17: bytes and a tail column tile, 80: packets and
    a partial column tile.  M = 1, 15, 16, 17 and both sides of every plan threshold; every variant of the operands; the output
    variants (level type, relu, mid_dtype) taken in turn, so that each M and each variant meets several"""
    from torchlsq import extension as E
    ms = sorted({1, 15, 16, 17} | {m for t in W.plan_row_thresholds(lambda M, n, k: E.requant_w8_plan_linear(M, n, k), N, K)
                                   for m in (t - 1, t)})
    assert ms == [1, 15, 16, 17, 32, 33, 64, 65]
    pl = E.requant_w8_plan_linear(33, N, K)
    assert pl["form"] == "mfma" and pl["store"] == ("packets" if N % 16 == 0 else "bytes")
    seen, used = {}, set()
    for j, M in enumerate(ms):
        for i, variant in enumerate(V.VARIANTS):
            ov = R.OUT_VARIANTS[(5 * j + 7 * i + N + K // 144) % len(R.OUT_VARIANTS)]
            used.add(ov)
            both_linear(R.linear_case(M, N, K, variant, ov, i), (M, i, R.out_id(ov)), seen)
    assert len(used) == len(R.OUT_VARIANTS)
    union_not_vacuous(seen)


@pytest.mark.parametrize("out_variant", R.OUT_VARIANTS, ids=R.out_id)
def test_every_output_variant_on_one_linear_and_one_conv_shape(out_variant):
    """both output level types, relu on and off, every mid_dtype: split-K tiles with packets (N = 48) and with bytes (N = 37)"""
    for N in (48, 37):
        both_linear(R.linear_case(40, N, 144, V.VARIANTS[1], out_variant, N), N)
    both_conv(R.conv_case(V.GEOMETRIES[0], V.VARIANTS[0], out_variant, 3), "conv")


def test_wide_tiles_equal_the_cpu_path_bit_for_bit():
    """the 64-column tiles at 8, 2 and 4 sub-tiles, N read from the plan: once N % 16 != 0 (bytes, a tail column tile) and once
    N % 16 == 0 with a partial last column tile (packets: the tile's tail holds whole packets only)"""
    from torchlsq import extension as E
    plan = E.requant_w8_plan_linear
    K = 144
    for M, rows in ((1927, 128), (20, 32), (50, 64)):
        col_tiles = next(t for t in range(1, 4097) if plan(M, 64 * t, K)["shape"] == "tiles")
        assert plan(M, 64 * (col_tiles - 1), K)["shape"] == "tiles_split_k"
        for N, store in ((64 * (col_tiles - 1) + 1, "bytes"), (64 * (col_tiles - 1) + 16, "packets")):
            N = N if plan(M, N, K)["shape"] == "tiles" else N + 64
            pl = plan(M, N, K)
            assert pl["shape"] == "tiles" and pl["cols_per_tile"] == 64 and pl["k_split"] == 1 and pl["rows_per_tile"] == rows, (M, N, pl)
            assert pl["store"] == store and N % 64 != 0
            ov = R.OUT_VARIANTS[(rows // 32 + (store == "packets") * 5) % len(R.OUT_VARIANTS)]
            both_linear(R.linear_case(M, N, K, V.VARIANTS[1 + (store == "packets")], ov, rows), (M, N, store))


def test_a_misaligned_output_takes_the_byte_store_and_leaves_its_surroundings_alone():
    from torchlsq import extension as E
    M, N, K = 40, 16, 144
    assert E.requant_w8_plan_linear(M, N, K, True, True)["store"] == "packets"
    assert E.requant_w8_plan_linear(M, N, K, True, False)["store"] == "bytes"
    for ov in (R.OUT_VARIANTS[0], R.OUT_VARIANTS[7]):                   # uint8 and int8 levels
        case = R.linear_case(M, N, K, V.VARIANTS[0], ov, 2)
        want = R.linear_q(*case)
        buf = torch.full((M * N + 64,), 0x5A, dtype=want.dtype, device=DEV)
        first = 17 + (-buf.data_ptr()) % 16                                 # byte offset 1 past a 16-byte boundary
        out = buf[first:first + M * N].view(M, N)
        assert out.data_ptr() % 16 == 1
        got = E.requant_w8_linear_levels(*dev(case[:9]), *case[9], case[10], case[11], out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and torch.equal(out.cpu(), want)
        assert bool((buf[first - 16:first] == 0x5A).all()) and bool((buf[first + M * N:first + M * N + 16] == 0x5A).all())
        R.assert_not_vacuous(want, case[9])
    # the aligned twin: packets, the same bytes, the same surroundings
    buf = torch.full((M * N + 64,), 0x5A, dtype=want.dtype, device=DEV)
    first = 16 + (-buf.data_ptr()) % 16
    out = buf[first:first + M * N].view(M, N)
    E.requant_w8_linear_levels(*dev(case[:9]), *case[9], case[10], case[11], out=out)
    assert torch.equal(out.cpu(), want)
    assert bool((buf[first - 16:first] == 0x5A).all()) and bool((buf[first + M * N:first + M * N + 16] == 0x5A).all())


@pytest.mark.parametrize("geometry", V.GEOMETRIES, ids=V.geom_id)
def test_conv_levels_form_equals_the_cpu_path_bit_for_bit(geometry):
    from torchlsq import extension as E
    B, Cin, H, Wd, N, k, s, p, d = geometry
    assert E.requant_w8_plan_conv(B, Cin, H, Wd, N, k, s, p, d)["form"] == "mfma"
    for i, variant in enumerate(V.VARIANTS):
        ov = R.OUT_VARIANTS[(5 * i + B + Cin + N) % len(R.OUT_VARIANTS)]
        both_conv(R.conv_case(geometry, variant, ov, i), (V.geom_id(geometry), i, R.out_id(ov)))


def test_a_conv_output_is_the_next_conv_operand_as_it_lies():
    """Cout = 16, padded 3 x 3: channels-last bytes stored as packets, read by a second convolution as its A operand"""
    from torchlsq import extension as E
    geometry = (2, 16, 7, 9, 16, (3, 3), (1, 1), (1, 1), (1, 1))
    assert E.requant_w8_plan_conv(*geometry[:5], 3, 1, 1)["store"] == "packets"
    for ov1, ov2 in ((R.OUT_VARIANTS[3], R.OUT_VARIANTS[1]), (R.OUT_VARIANTS[8], R.OUT_VARIANTS[5])):
        c1 = R.conv_case(geometry, V.VARIANTS[0], ov1, 1)
        y1 = both_conv(c1, "first")
        s1, z1 = _act_constants(c1[8], c1[9], c1[10][2], c1[10][3])
        # the second convolution's operands, with its quantizer taken from the float result on the first one's CPU levels
        lw, s_w, zw = V.conv_weight(24, 16, (3, 3), torch.int8, 9)
        geo = ([2, 2], [1, 1], [1, 1])
        ref = OPS.lsq_conv2d_w8_q8(y1.cpu(), s1, z1, lw, s_w, zw, None, *geo, torch.float32)
        osc, osh, rng = R.out_quantizer(ref, ov2[0], ov2[1])
        c2 = (y1.cpu(), s1, z1, lw, s_w, zw, None, geo, osc, osh, rng, ov2[1], ov2[2])
        want = R.conv_q(*c2)
        got = R.conv_q(y1, *dev(c2[1:]))                                   # y1 as the GPU wrote it: no copy, no relayout
        assert y1.is_contiguous(memory_format=CL) and torch.equal(got.cpu(), want)
        R.assert_not_vacuous(want, rng, "second")


def test_generic_form_equals_the_cpu_path_bit_for_bit():
    """Cin = 3 (a stem), K % 16 != 0, and a weight at byte offset 1"""
    from torchlsq import extension as E
    stem = (2, 3, 12, 12, 24, (7, 7), (2, 2), (3, 3), (1, 1))
    assert E.requant_w8_plan_conv(*stem[:5], 7, 2, 3)["form"] == "generic"
    for i, ov in enumerate((R.OUT_VARIANTS[0], R.OUT_VARIANTS[4], R.OUT_VARIANTS[11])):
        both_conv(R.conv_case(stem, V.VARIANTS[i], ov, i), ("stem", i))
        assert E.requant_w8_plan_linear(21, 37, 40)["form"] == "generic"
        both_linear(R.linear_case(21, 37, 40, V.VARIANTS[i + 1], ov, i), ("K = 40", i))
    case = R.linear_case(40, 16, 144, V.VARIANTS[0], R.OUT_VARIANTS[2], 4)
    want = R.linear_q(*case)
    d = dev(case)
    buf = torch.zeros(16 * 144 + 32, dtype=torch.int8, device=DEV)
    first = 1 + (-buf.data_ptr()) % 16
    buf[first:first + 16 * 144] = d[3].flatten()
    d[3] = buf[first:first + 16 * 144].view(16, 144)
    assert d[3].data_ptr() % 16 == 1
    assert torch.equal(R.linear_q(*d).cpu(), want)
    R.assert_not_vacuous(want, case[9])


@pytest.mark.parametrize("dtype", R.MIDS, ids=lambda v: str(v).replace("torch.", ""))
def test_fused_forms_equal_the_levels_forms_on_the_levels_forward_bytes(dtype):
    gen = torch.Generator().manual_seed(5)
    a_s, a_b, ir = torch.tensor([0.02]), torch.tensor([-2.5]), (0, 255, 0, 255)
    for relu, unsigned in ((False, True), (True, False)):
        lw, s_w, zw = W.weight(37, 144, torch.int8, 3)
        x = torch.randn(40, 144, generator=gen).to(dtype)
        osc, osh, rng = R.out_quantizer(OPS.lsq_linear_w8_a8(x.float(), a_s, a_b, *ir, lw, s_w, zw, None), unsigned, relu)
        want = OPS.lsq_linear_w8_a8_q(x, a_s, a_b, *ir, lw, s_w, zw, None, osc, osh, *rng, relu)
        xg, a_sg, a_bg, lwg, s_wg, zwg, oscg, oshg = R.to(DEV, x, a_s, a_b, lw, s_w, zw, osc, osh)
        got = OPS.lsq_linear_w8_a8_q(xg, a_sg, a_bg, *ir, lwg, s_wg, zwg, None, oscg, oshg, *rng, relu)
        lv = OPS.lsq_levels_per_tensor(xg, a_sg, a_bg, *ir, 0).view(torch.uint8)
        s_x, z_x = _act_constants(a_sg, a_bg, 0, 255)
        via = OPS.lsq_linear_w8_q8_q(lv, s_x, z_x, lwg, s_wg, zwg, None, oscg, oshg, *rng, relu, dtype)
        assert torch.equal(got, via) and torch.equal(got.cpu(), want)
        R.assert_not_vacuous(want, rng, "linear")
        cw, c_s, c_z = V.conv_weight(17, 16, (3, 3), torch.int8, 4)
        xc = torch.randn(2, 16, 5, 7, generator=gen).to(dtype).contiguous(memory_format=CL)
        geo = ([1, 1], [1, 1], [1, 1])
        osc, osh, rng = R.out_quantizer(OPS.lsq_conv2d_w8_a8(xc.float(), a_s, a_b, *ir, cw, c_s, c_z, None, *geo), unsigned, relu)
        want = OPS.lsq_conv2d_w8_a8_q(xc, a_s, a_b, *ir, cw, c_s, c_z, None, *geo, osc, osh, *rng, relu)
        xg, cwg, c_sg, c_zg, oscg, oshg = R.to(DEV, xc, cw, c_s, c_z, osc, osh)
        got = OPS.lsq_conv2d_w8_a8_q(xg, a_sg, a_bg, *ir, cwg, c_sg, c_zg, None, *geo, oscg, oshg, *rng, relu)
        lv = OPS.lsq_levels_per_tensor(xg, a_sg, a_bg, *ir, 0).view(torch.uint8)
        via = OPS.lsq_conv2d_w8_q8_q(lv, s_x, z_x, cwg, c_sg, c_zg, None, *geo, oscg, oshg, *rng, relu, dtype)
        assert got.is_contiguous(memory_format=CL) and torch.equal(got, via) and torch.equal(got.cpu(), want)
        R.assert_not_vacuous(want, rng, "conv")


@pytest.mark.parametrize("out_variant", R.OUT_VARIANTS[::2] + R.OUT_VARIANTS[1::6], ids=R.out_id)
def test_the_definition_against_the_three_existing_gpu_ops_composed(out_variant):
    """the code the parent commit ships, on the GPU, not the code under test: wide tiles (packets), split-K (bytes), generic,
    a convolution"""
    for M, N, K in ((2100, 1024, 144), (40, 37, 288), (21, 37, 40)):
        case = dev(R.linear_case(M, N, K, V.VARIANTS[1], out_variant, M))
        got = R.linear_q(*case)
        assert torch.equal(got, R.linear_composed(*case)), (M, N, K)
        R.assert_not_vacuous(got, case[9], (M, N, K))
    for geometry in (V.GEOMETRIES[0], V.GEOMETRIES[2]):
        case = dev(R.conv_case(geometry, V.VARIANTS[0], out_variant, 2))
        got = R.conv_q(*case)
        assert torch.equal(got, R.conv_composed(*case)), geometry
        R.assert_not_vacuous(got, case[10], geometry)


def test_launches_repeat_and_a_row_does_not_depend_on_m_or_its_place():
    case = R.linear_case(150, 80, 288, V.VARIANTS[1], R.OUT_VARIANTS[4], 6)
    d = dev(case)
    full = R.linear_q(*d)
    assert torch.equal(full, R.linear_q(*d))
    R.assert_not_vacuous(full, case[9])
    for lo, hi in ((0, 1), (5, 21), (33, 98), (149, 150), (60, 150)):          # decode-sized, 32-, 64- and 128-row tiles
        part = R.linear_q(d[0][lo:hi].contiguous(), *d[1:])
        assert torch.equal(part, full[lo:hi]), (lo, hi)
    rev = R.linear_q(d[0].flip(0).contiguous(), *d[1:])
    assert torch.equal(rev.flip(0), full)
    ccase = R.conv_case((3, 16, 6, 7, 20, (3, 3), (1, 1), (1, 1), (1, 1)), V.VARIANTS[0], R.OUT_VARIANTS[9], 2)
    dc = dev(ccase)
    fullc = R.conv_q(*dc)
    assert torch.equal(fullc, R.conv_q(*dc))
    assert torch.equal(R.conv_q(dc[0][1:2].contiguous(memory_format=CL), *dc[1:]), fullc[1:2])


def test_a_converted_chain_is_captured_in_a_graph_and_replayed():
    """conv-relu, conv, flatten, linear (qconv_w8_cases.qat_conv_model), converted by convert_w8a8_q: captured once (a host
    read-back in the captured region would end the capture with an error), replayed on new input; equal to the eager result and
    to the CPU modules"""
    from torchlsq.quantized import convert_w8a8_q
    model, q0, q1, q2 = V.qat_conv_model(with_linear=True)
    torch.manual_seed(9)
    xs = [torch.randn(6, 16, 7, 7).to(torch.bfloat16) for _ in range(2)]
    with torch.no_grad():
        out_q = R.trained_quantizer(model[4](q2(model[3](model[2](q1(model[1](model[0](q0(xs[0].float())))))))))
    cpu = convert_w8a8_q(model, {"0": q0, "2": q1, "4": q2}, {"0": q1, "2": q2, "4": out_q}, relu=("0",), mid_dtype=torch.bfloat16)
    gpu = convert_w8a8_q(model, {"0": q0, "2": q1, "4": q2}, {"0": q1, "2": q2, "4": out_q}, relu=("0",), mid_dtype=torch.bfloat16).to(DEV)
    assert gpu[0].weight_levels.is_contiguous(memory_format=CL)
    static = xs[0].to(DEV).contiguous(memory_format=CL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        eager = gpu(static).levels.clone()                                  # warm-up: loads every kernel before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        captured = gpu(static)
    for x in xs:
        static.copy_(x.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = cpu(x).levels
        assert torch.equal(captured.levels.cpu(), want) and len(want.unique()) > 8
        with torch.no_grad():
            assert torch.equal(gpu(static).levels, captured.levels)
    assert captured.scale.is_cuda and captured.zero_point.is_cuda and torch.equal(captured.scale.cpu(), cpu(xs[0]).scale)
    assert eager.shape == (6, 5)
