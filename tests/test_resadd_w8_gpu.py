"""GPU: the W8A8 layers that close a residual block (include/lsq_hip_resadd_w8.h, liblsq_hip_resadd_w8.so,
torch.ops.torchlsq.lsq_linear_w8_q8_add_q / lsq_conv2d_w8_q8_add_q, torchlsq.quantized.convert_w8a8_add_q) on the MI355X.

The contract defines every output byte (existing ops composed), so every comparison here is `torch.equal` on the levels: against
the package's CPU path -- which IS that composition and which tests/test_resadd_w8_cpu.py holds to integers at the rounding ties
-- and against the existing GPU ops composed.  No tolerance appears in this file.  The cases and the conditions every random case
of 336 outputs or more is held to (on the CPU result) are resadd_w8_cases'; the sweeps over small M are held to them on the
union of their results per output quantizer.
"""
import pytest
import torch

import qconv_w8_cases as V
import qlinear_w8_cases as W
import requant_w8_cases as R
import resadd_w8_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
OPS = torch.ops.torchlsq


def dev(case):
    return [t.to(DEV) if isinstance(t, torch.Tensor) else t for t in case]


def both_linear(case, note, seen=None):
    """the op on the CPU and on the GPU: equal levels; returns the GPU result"""
    want = A.linear_add(*case)
    got = A.linear_add(*dev(case))
    assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape, note
    assert torch.equal(got.cpu(), want), note
    if want.numel() >= 336:
        A.assert_conditions(want, case, False, note)
    if seen is not None:
        seen.setdefault(case[9], []).append(want.flatten())
    return got


def both_conv(case, note):
    want = A.conv_add(*case)
    got = A.conv_add(*dev(case))
    assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape and got.is_contiguous(memory_format=CL), note
    assert torch.equal(got.cpu(), want), note
    if want.numel() >= 336:
        A.assert_conditions(want, case, True, note)
    return got


def union_not_vacuous(seen):
    for rng, parts in seen.items():
        R.assert_not_vacuous(torch.cat(parts), rng, rng)


@pytest.mark.parametrize("N", [16, 17, 64, 80])
def test_linear_tiles_equal_the_cpu_path_bit_for_bit(N):
    """K = 144: a tail step.  N = 16 / 64: packets (loads and stores) on full tiles, 17: bytes and a tail column tile, 80: packets
    and a partial column tile.  M = 1, 15, 16, 17 and both sides of every plan threshold; the variants of the operands, of the
    output (level type, relu, mid_dtype) and of the residual (pre on / off, level type) taken in turn, so that each meets several"""
    from torchlsq import extension as E
    K = 144
    ms = sorted({1, 15, 16, 17} | {m for t in W.plan_row_thresholds(lambda M, n, k: E.resadd_w8_plan_linear(M, n, k), N, K)
                                   for m in (t - 1, t)})
    assert ms == [1, 15, 16, 17, 32, 33, 64, 65]
    pl = E.resadd_w8_plan_linear(33, N, K)
    assert pl["form"] == "mfma" and pl["store"] == pl["res_load"] == ("packets" if N % 16 == 0 else "bytes")
    seen, used, used_res = {}, set(), set()
    for j, M in enumerate(ms):
        for i, variant in enumerate(V.VARIANTS):
            ov = R.OUT_VARIANTS[(5 * j + 7 * i + N) % len(R.OUT_VARIANTS)]
            rv = A.RES_VARIANTS[(j + i + N // 16) % len(A.RES_VARIANTS)]
            used.add(ov)
            used_res.add(rv)
            both_linear(A.linear_case(M, N, K, variant, ov, rv, i), (M, i, R.out_id(ov), A.res_id(rv)), seen)
    assert len(used) == len(R.OUT_VARIANTS) and len(used_res) == len(A.RES_VARIANTS)
    union_not_vacuous(seen)


@pytest.mark.parametrize("res_variant", A.RES_VARIANTS, ids=A.res_id)
def test_every_variant_on_one_linear_and_one_conv_shape(res_variant):
    """pre on and off, both residual level types, with every output variant: split-K tiles with packets (N = 48) and with bytes
    (N = 37), and a convolution"""
    for out_variant in R.OUT_VARIANTS:
        for N in (48, 37):
            both_linear(A.linear_case(40, N, 144, V.VARIANTS[1], out_variant, res_variant, N), (N, R.out_id(out_variant)))
        both_conv(A.conv_case(V.GEOMETRIES[0], V.VARIANTS[0], out_variant, res_variant, 3), ("conv", R.out_id(out_variant)))


def test_wide_tiles_equal_the_cpu_path_bit_for_bit():
    """the 64-column tiles at 8, 2 and 4 sub-tiles, N read from the plan: once N % 16 != 0 (bytes, a tail column tile) and once
    N % 16 == 0 with a partial last column tile (packets: the tile's tail holds whole packets only)"""
    from torchlsq import extension as E
    plan = E.resadd_w8_plan_linear
    K = 144
    for M, rows in ((1927, 128), (20, 32), (50, 64)):
        col_tiles = next(t for t in range(1, 4097) if plan(M, 64 * t, K)["shape"] == "tiles")
        assert plan(M, 64 * (col_tiles - 1), K)["shape"] == "tiles_split_k"
        for N, how in ((64 * (col_tiles - 1) + 1, "bytes"), (64 * (col_tiles - 1) + 16, "packets")):
            N = N if plan(M, N, K)["shape"] == "tiles" else N + 64
            pl = plan(M, N, K)
            assert pl["shape"] == "tiles" and pl["cols_per_tile"] == 64 and pl["k_split"] == 1 and pl["rows_per_tile"] == rows, (M, N, pl)
            assert pl["store"] == pl["res_load"] == how and N % 64 != 0
            ov = R.OUT_VARIANTS[(rows // 32 + (how == "packets") * 5) % len(R.OUT_VARIANTS)]
            rv = A.RES_VARIANTS[(rows // 32 + (how == "packets")) % len(A.RES_VARIANTS)]
            both_linear(A.linear_case(M, N, K, V.VARIANTS[1 + (how == "packets")], ov, rv, rows), (M, N, how))


def _at_offset(t, offset):
    """(a buffer of 0x5A bytes, its view of t's shape that starts `offset` bytes past a 16-byte boundary and holds t's bytes, the
    view's first byte in the buffer)"""
    n = t.numel()
    buf = torch.full((n + 64,), 0x5A, dtype=t.dtype, device=DEV)
    first = 16 + offset + (-buf.data_ptr()) % 16
    view = buf[first:first + n].view(t.shape)
    view.copy_(t)
    return buf, view, first


def _guards_intact(buf, first, n):
    return bool((buf[first - 16:first] == 0x5A).all()) and bool((buf[first + n:first + n + 16] == 0x5A).all())


def test_alignment_of_the_residual_and_of_y_are_independent_and_their_surroundings_stay():
    from torchlsq import extension as E
    M, N, K = 40, 16, 144
    plan = E.resadd_w8_plan_linear
    assert (plan(M, N, K, True, True, False)["res_load"], plan(M, N, K, True, True, False)["store"]) == ("bytes", "packets")
    assert (plan(M, N, K, True, False, True)["res_load"], plan(M, N, K, True, False, True)["store"]) == ("packets", "bytes")
    for ov, rv in ((R.OUT_VARIANTS[0], A.RES_VARIANTS[3]), (R.OUT_VARIANTS[7], A.RES_VARIANTS[0])):
        case = A.linear_case(M, N, K, V.VARIANTS[0], ov, rv, 2)
        want = A.linear_add(*case)
        A.assert_conditions(want, case, False)
        d = dev(case)
        for res_off, y_off in ((1, 0), (0, 1), (0, 0), (1, 1)):              # misaligned residual; misaligned y; the aligned twin; both
            rbuf, rview, rfirst = _at_offset(d[12], res_off)
            ybuf, out, yfirst = _at_offset(torch.zeros(M, N, dtype=want.dtype, device=DEV), y_off)
            assert rview.data_ptr() % 16 == res_off and out.data_ptr() % 16 == y_off
            before = rbuf.clone()
            got = E.resadd_w8_linear_levels(*d[:9], *d[9], d[10], d[11], rview, *d[13:17], *d[17], out=out)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr() and torch.equal(out.cpu(), want), (res_off, y_off)
            assert _guards_intact(ybuf, yfirst, M * N) and torch.equal(rbuf, before), (res_off, y_off)


@pytest.mark.parametrize("geometry", V.GEOMETRIES, ids=V.geom_id)
def test_conv_levels_form_equals_the_cpu_path_bit_for_bit(geometry):
    from torchlsq import extension as E
    B, Cin, H, Wd, N, k, s, p, d = geometry
    pl = E.resadd_w8_plan_conv(B, Cin, H, Wd, N, k, s, p, d)
    assert pl["form"] == "mfma" and pl["res_load"] == ("packets" if N % 16 == 0 else "bytes")
    for i, variant in enumerate(V.VARIANTS):
        ov = R.OUT_VARIANTS[(5 * i + B + Cin + N) % len(R.OUT_VARIANTS)]
        rv = A.RES_VARIANTS[(i + B + N) % len(A.RES_VARIANTS)]
        both_conv(A.conv_case(geometry, variant, ov, rv, i), (V.geom_id(geometry), i, R.out_id(ov), A.res_id(rv)))


def test_generic_form_equals_the_cpu_path_bit_for_bit():
    """K = 150 (K % 16 != 0) and Cin = 3 (a stem)"""
    from torchlsq import extension as E
    stem = (2, 3, 12, 12, 24, (7, 7), (2, 2), (3, 3), (1, 1))
    assert E.resadd_w8_plan_conv(*stem[:5], 7, 2, 3)["form"] == "generic" and E.resadd_w8_plan_linear(21, 37, 150)["form"] == "generic"
    for i, (ov, rv) in enumerate(((R.OUT_VARIANTS[0], A.RES_VARIANTS[2]), (R.OUT_VARIANTS[4], A.RES_VARIANTS[1]),
                                  (R.OUT_VARIANTS[11], A.RES_VARIANTS[3]))):
        both_conv(A.conv_case(stem, V.VARIANTS[i], ov, rv, i), ("stem", i))
        both_linear(A.linear_case(21, 37, 150, V.VARIANTS[i + 1], ov, rv, i), ("K = 150", i))


def test_the_product_and_the_add_are_not_contracted():
    """resadd_w8_cases.contraction_case: float32 levels that an fma of the residual's product and the add would change; the
    matrix-core form (K = 16) and the generic one (the weight at byte offset 1)"""
    from torchlsq import extension as E
    case, k, two_step, fused = A.contraction_case()
    assert E.resadd_w8_plan_linear(11, 23, 16)["form"] == "mfma" and bool((two_step != fused).any())
    d = dev(case)
    assert torch.equal(A.linear_add(*d).cpu().to(torch.int64), two_step)
    buf = torch.zeros(23 * 16 + 32, dtype=torch.int8, device=DEV)
    first = 1 + (-buf.data_ptr()) % 16
    buf[first:first + 23 * 16] = d[3].flatten()
    d[3] = buf[first:first + 23 * 16].view(23, 16)
    assert d[3].data_ptr() % 16 == 1
    assert torch.equal(A.linear_add(*d).cpu().to(torch.int64), two_step)


@pytest.mark.parametrize("res_variant", A.RES_VARIANTS[1:3], ids=A.res_id)
@pytest.mark.parametrize("out_variant", R.OUT_VARIANTS[::2] + R.OUT_VARIANTS[1::6], ids=R.out_id)
def test_the_definition_against_the_existing_gpu_ops_composed(out_variant, res_variant):
    """the code the parent commit ships, on the GPU, not the code under test: wide tiles (packets), split-K (bytes), generic,
    a convolution"""
    for M, N, K in ((2100, 1024, 144), (40, 37, 288), (21, 37, 40)):
        case = A.linear_case(M, N, K, V.VARIANTS[1], out_variant, res_variant, M)
        d = dev(case)
        got = A.linear_add(*d)
        assert torch.equal(got, A.linear_composed(*d)), (M, N, K)
        R.assert_not_vacuous(got, case[9], (M, N, K))
    for geometry in (V.GEOMETRIES[0], V.GEOMETRIES[2]):
        case = A.conv_case(geometry, V.VARIANTS[0], out_variant, res_variant, 2)
        d = dev(case)
        got = A.conv_add(*d)
        assert torch.equal(got, A.conv_composed(*d)), geometry
        R.assert_not_vacuous(got, case[10], geometry)


def test_launches_repeat_and_a_row_does_not_depend_on_m_or_its_place():
    case = A.linear_case(150, 80, 288, V.VARIANTS[1], R.OUT_VARIANTS[4], A.RES_VARIANTS[2], 6)
    d = dev(case)
    full = A.linear_add(*d)
    assert torch.equal(full, A.linear_add(*d))
    A.assert_conditions(full.cpu(), case, False)
    for lo, hi in ((0, 1), (5, 21), (33, 98), (149, 150), (60, 150)):          # decode-sized, 32-, 64- and 128-row tiles
        part = A.linear_add(d[0][lo:hi].contiguous(), *d[1:12], d[12][lo:hi].contiguous(), *d[13:])
        assert torch.equal(part, full[lo:hi]), (lo, hi)
    rev = A.linear_add(d[0].flip(0).contiguous(), *d[1:12], d[12].flip(0).contiguous(), *d[13:])
    assert torch.equal(rev.flip(0), full)
    ccase = A.conv_case((3, 16, 6, 7, 20, (3, 3), (1, 1), (1, 1), (1, 1)), V.VARIANTS[0], R.OUT_VARIANTS[9], A.RES_VARIANTS[3], 2)
    dc = dev(ccase)
    fullc = A.conv_add(*dc)
    assert torch.equal(fullc, A.conv_add(*dc))
    one = A.conv_add(dc[0][1:2].contiguous(memory_format=CL), *dc[1:13], dc[13][1:2].contiguous(memory_format=CL), *dc[14:])
    assert torch.equal(one, fullc[1:2])


def test_a_converted_block_is_captured_in_a_graph_and_replayed():
    """resadd_w8_cases.BasicBlock converted by convert_w8a8_q and convert_w8a8_add_q: captured once (a host read-back in the
    captured region would end the capture with an error), replayed on new input bytes; equal to the eager chain of the EXISTING
    modules and ops and to the converted block on the CPU"""
    from torchlsq.functional import LevelsTensor
    block, qs, x = A.basic_block()
    mid = torch.bfloat16
    cpu = A.convert_block(block, qs, mid)
    gpu = A.convert_block(block, qs, mid).to(DEV)
    torch.manual_seed(3)
    xs = [LevelsTensor.from_quantized(qs["in"].quantize(x)), LevelsTensor.from_quantized(qs["in"].quantize(torch.randn(4, 16, 10, 10) * 1.5))]
    static = LevelsTensor(xs[0].levels.to(DEV).contiguous(memory_format=CL), xs[0].scale.to(DEV), xs[0].zero_point.to(DEV), 0, 255)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        eager = gpu(static).levels.clone()                                  # warm-up: loads every kernel before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        captured = gpu(static)
    for xl in xs:
        static.levels.copy_(xl.levels.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            want = A.block_written_out(block, qs, static, mid)             # the existing modules and ops, eager, on the GPU
        assert torch.equal(captured.levels, want) and torch.equal(captured.levels.cpu(), cpu(xl).levels)
        assert len(want.unique()) > 32
    assert captured.scale.is_cuda and captured.zero_point.is_cuda and eager.shape == (4, 32, 5, 5)
    assert not torch.equal(cpu(xs[0]).levels, cpu(xs[1]).levels)
