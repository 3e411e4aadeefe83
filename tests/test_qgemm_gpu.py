"""GPU: the matrix-core GEMM on packed group-wise weights (liblsq_hip_qgemm.so), reached through
torchlsq.functional.lsq_linear_packed with more than 16 rows of bfloat16 / float16 x and through direct calls of
lsq_qgemm_forward, against the fp64 reference, the bound and the exact-arithmetic inputs of tests/qlinear_cases.py (its
docstring derives the bound; nothing here widens it).

  * the bound and the exact test at M = 17, R, R + 1, 2 R + 3 (R: the plan's rows per tile) over a ragged column tile, one
    packet per group with a partial K step, 2-bit packets and groups of three packets beyond 4096 k, with and without a bias;
    the op and the direct call agree bit for bit -- the proof that the op took the GEMM;
  * zero points near 100 and far beyond the code range;
  * invariance: a row's bits do not depend on M, on its place, or on the tile shape (16- or 64-column tiles; 2, 4 or 8
    sub-tiles of 16 rows), and 20 launches repeat bit for bit;
  * the surface: x of [3, 7, K], an element-aligned view, the formats that stay on the dequantize route, a captured graph,
    PackedLinear, no weight-sized temporary, the error paths.
"""
import pytest
import torch
import torchlsq  # noqa: F401  (registers torch.ops.torchlsq.*)

import qlinear_cases as C
from torchlsq import extension as E
from torchlsq.functional import PackedGroupTensor, lsq_linear_packed

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_id = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))
DTYPES = [torch.bfloat16, torch.float16]
# (N, K, G, bits): a ragged column tile on one packet per group (three packets: a partial K step); 67 columns and groups of 4
# packets; 2-bit packets; groups of three packets (no power of two) beyond 4096 k
CASES = [(17, 96, 32, 4), (67, 384, 128, 4), (5, 512, 128, 2), (33, 4800, 96, 4)]
R = 128
CODE = {torch.bfloat16: E.LSQ_BF16, torch.float16: E.LSQ_F16, torch.float32: E.LSQ_F32}


def to_dev(p):
    return PackedGroupTensor(p.codes.to(DEV), p.scale.to(DEV), p.zero_point.to(DEV), p.bits, p.group_size, p.quant_min, p.shape)


def direct(x, pg, bias=None):
    """lsq_qgemm_forward itself, on the current stream"""
    lib = E.qgemm_library()
    M, K = x.shape
    N = pg.shape[0]
    assert x.is_contiguous() and pg.codes.is_contiguous() and pg.scale.dtype == torch.float32 and pg.zero_point.dtype == torch.int32
    y = torch.empty(M, N, dtype=x.dtype, device=DEV)
    rc = lib.lsq_qgemm_forward(CODE[x.dtype], x.data_ptr(), M, pg.codes.data_ptr(), N, K, pg.group_size, pg.bits,
                               pg.scale.data_ptr(), pg.zero_point.data_ptr(), None if bias is None else bias.data_ptr(),
                               0 if bias is None else CODE[bias.dtype], y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.lsq_qgemm_last_error()
    return y


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_the_plan_has_the_rows_per_tile_the_tests_assume():
    for N, K, G, bits in CASES:
        assert E.qgemm_plan(torch.bfloat16, 17, N, K, G, bits)["rows_per_tile"] == R
        assert E.qgemm_plan(torch.float16, 2 * R + 3, N, K, G, bits)["form"] == "mfma"


@pytest.mark.parametrize("dtype", DTYPES, **_id)
@pytest.mark.parametrize("case", CASES, **_id)
def test_bound_exactness_and_dispatch(case, dtype):
    N, K, G, bits = case
    p = C.random_packed(N, K, G, bits, seed=N)
    pg = to_dev(p)
    x = C.random_x((2 * R + 3, K), dtype, seed=N)
    xg = x.to(DEV)
    for bias in (None, C.random_bias(N, torch.float32, seed=K), C.random_bias(N, dtype, seed=K)):
        bg = None if bias is None else bias.to(DEV)
        r, Eb = C.reference(x, p, bias)             # once for all M: the rows of a shorter call are its first rows
        for M in (17, R, R + 1, 2 * R + 3):
            y = lsq_linear_packed(xg[:M], pg, bg)
            C.assert_within_bound(y, r[:M], Eb[:M], dtype, "gemm %s M %d bias %s" % (case, M, None if bias is None else bias.dtype))
            assert same_bits(y, direct(xg[:M], pg, bg)), "the op did not return the GEMM's bits at M = %d" % M
    if K <= 4096:
        pe, xe = C.exact_packed(N, K, G, bits, seed=N), C.exact_x((2 * R + 3, K), dtype, seed=N)
        peg, xeg = to_dev(pe), xe.to(DEV)
        r, _ = C.reference(xe, pe)
        for M in (17, R, R + 1, 2 * R + 3):
            y = lsq_linear_packed(xeg[:M], peg)
            C.assert_exact(y, r[:M], dtype, "gemm exact %s M %d" % (case, M))
            assert same_bits(y, direct(xeg[:M], peg))


@pytest.mark.parametrize("dtype", DTYPES, **_id)
def test_zero_points_near_100_and_far_outside_the_code_range(dtype):
    for what, p in (("affine export, qzero near 100", C.affine_packed(19, 256, 32)),
                    ("far zero points, 4 bits", C.far_packed(19, 256, 32, 4)),
                    ("far zero points, 2 bits", C.far_packed(7, 512, 64, 2))):
        K = p.shape[1]
        pg = to_dev(p)
        x = C.random_x((R + 1, K), dtype, seed=3)
        bias = C.random_bias(p.shape[0], torch.float32)
        r, Eb = C.reference(x, p, bias)
        for M in (17, R + 1):
            y = lsq_linear_packed(x[:M].to(DEV), pg, bias.to(DEV))
            C.assert_within_bound(y, r[:M], Eb[:M], dtype, "%s, M = %d" % (what, M))
            assert same_bits(y, direct(x[:M].to(DEV), pg, bias.to(DEV)))


@pytest.mark.parametrize("dtype", DTYPES, **_id)
@pytest.mark.parametrize("case", CASES, **_id)
def test_rows_do_not_depend_on_the_batch(case, dtype):
    """row m of one call is that row of any other call, wherever it sits; 17 / 40 and 64 / 65 and more rows compute 2 / 4 / 8
    sub-tiles of 16 rows"""
    N, K, G, bits = case
    pg = to_dev(C.random_packed(N, K, G, bits))
    x = C.random_x((2 * R + 3, K), dtype).to(DEV)
    bias = C.random_bias(N, dtype).to(DEV)
    y_all = lsq_linear_packed(x, pg, bias)
    assert same_bits(lsq_linear_packed(x[:17], pg, bias)[16], y_all[16])
    for m in (0, R - 1, R, 2 * R + 2):
        y = lsq_linear_packed(torch.cat([x[m:m + 1], x[:16]]), pg, bias)
        assert same_bits(y[0], y_all[m]), "row %d of %d, as row 0 of 17" % (m, 2 * R + 3)
    for M in (17, 32, 33, 40, 64, 65, R, R + 1):
        assert same_bits(lsq_linear_packed(x[:M], pg, bias), y_all[:M]), "the first %d rows" % M
    for _ in range(19):
        assert same_bits(lsq_linear_packed(x, pg, bias), y_all)
    first = lsq_linear_packed(x[:17], pg, bias)
    for _ in range(19):
        assert same_bits(lsq_linear_packed(x[:17], pg, bias), first)


@pytest.mark.parametrize("dtype", DTYPES, **_id)
@pytest.mark.parametrize("case", [(67, 384, 128, 4), (5, 512, 128, 2)], **_id)
def test_both_column_tiles_give_the_same_bits(case, dtype):
    """the plan takes 64-column tiles once they give every compute unit one: an M on each side of that choice"""
    N, K, G, bits = case
    tiles = next(t for t in range(1, 4097) if E.qgemm_plan(dtype, t * R, N, K, G, bits)["cols_per_tile"] == 64)
    M_wide = (tiles - 1) * R + 1
    assert E.qgemm_plan(dtype, M_wide, N, K, G, bits)["cols_per_tile"] == 64
    assert E.qgemm_plan(dtype, M_wide - 1, N, K, G, bits)["cols_per_tile"] == 16
    pg = to_dev(C.random_packed(N, K, G, bits))
    x = C.random_x((M_wide, K), dtype).to(DEV)
    bias = C.random_bias(N, torch.float32).to(DEV)
    y_wide = lsq_linear_packed(x, pg, bias)
    y_narrow = lsq_linear_packed(x[:M_wide - 1], pg, bias)
    assert same_bits(y_wide[:M_wide - 1], y_narrow)
    last = lsq_linear_packed(torch.cat([x[M_wide - 1:], x[:16]]), pg, bias)
    assert same_bits(last[0], y_wide[M_wide - 1])
    r, Eb = C.reference(x[-300:].cpu(), C.random_packed(N, K, G, bits), bias.cpu())
    C.assert_within_bound(y_wide[-300:], r, Eb, dtype, "64-column tiles, the last 300 of %d rows" % M_wide)


@pytest.mark.parametrize("dtype", DTYPES, **_id)
def test_views_of_x_and_what_stays_on_the_dequantize_route(dtype):
    N, K, G, bits = 21, 256, 32, 4
    p, pe = C.random_packed(N, K, G, bits, seed=5), C.exact_packed(N, K, G, bits, seed=5)
    x3, xe3 = C.random_x((3, 7, K), dtype), C.exact_x((3, 7, K), dtype)
    r, Eb = C.reference(x3, p)
    re_, _ = C.reference(xe3, pe)
    y = lsq_linear_packed(x3.to(DEV), to_dev(p))
    assert y.shape == (3, 7, N)
    C.assert_within_bound(y, r, Eb, dtype, "x [3, 7, K]")
    assert same_bits(y.reshape(21, N), direct(x3.to(DEV).reshape(21, K), to_dev(p)))
    ye = lsq_linear_packed(xe3.to(DEV), to_dev(pe))
    C.assert_exact(ye, re_, dtype, "x [3, 7, K]")
    # an x[1:]-style view: a storage offset of one element
    flat = torch.zeros(21 * K + 1, dtype=dtype, device=DEV)
    flat[1:] = xe3.reshape(-1).to(DEV)
    xv = flat[1:].view(3, 7, K)
    assert xv.data_ptr() % 16 != 0
    yv = lsq_linear_packed(xv, to_dev(pe))
    C.assert_exact(yv, re_, dtype, "x[1:]")
    assert same_bits(yv, ye) and same_bits(yv.reshape(21, N), direct(xv.reshape(21, K), to_dev(pe)))
    # codes at byte offset 1 of a larger buffer are not served: the dequantize route, within the bound
    buf = torch.zeros(p.codes.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = p.codes.reshape(-1).to(DEV)
    qv = PackedGroupTensor(buf[1:].view(N, -1), p.scale.to(DEV), p.zero_point.to(DEV), bits, G, p.quant_min, p.shape)
    assert qv.codes.data_ptr() % 16 != 0 and qv.codes.is_contiguous()
    C.assert_within_bound(lsq_linear_packed(x3.to(DEV), qv), r, Eb, dtype, "codes at byte offset 1")
    # float32 x, and a group below one packet: the dequantize route too
    x32 = C.random_x((3, 7, K), torch.float32)
    r32, E32 = C.reference(x32, p)
    C.assert_within_bound(lsq_linear_packed(x32.to(DEV), to_dev(p)), r32, E32, torch.float32, "float32 x, 21 rows")
    p8 = C.random_packed(9, 24, 8, 4)
    x8 = C.random_x((21, 24), dtype)
    r8, E8 = C.reference(x8, p8)
    C.assert_within_bound(lsq_linear_packed(x8.to(DEV), to_dev(p8)), r8, E8, dtype, "G = 8, 21 rows")


def test_a_captured_graph_at_40_rows():
    N, K, G, bits = 67, 384, 128, 4
    pg = to_dev(C.random_packed(N, K, G, bits))
    bias = C.random_bias(N, torch.float32).to(DEV)
    args = (pg.codes, pg.scale.reshape(-1), pg.zero_point.reshape(-1), bias)

    def f(x, codes, scale, zp, b):
        return torch.ops.torchlsq.lsq_linear_packed(x, codes, scale, zp, b, G, bits)

    x = C.random_x((40, K), torch.bfloat16).to(DEV)
    want = f(x, *args)
    assert same_bits(want, direct(x, pg, bias))
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f(static_x, *args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = f(static_x, *args)
    x2 = C.random_x((40, K), torch.bfloat16, seed=9).to(DEV)
    static_x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(static_y, f(x2, *args)) and not same_bits(static_y, want)


def test_packed_linear_module_at_40_rows():
    from torchlsq.quantized import PackedLinear
    p = C.random_packed(67, 384, 128, 4)
    bias = C.random_bias(67, torch.float32)
    m = PackedLinear.from_packed(p, bias).to(DEV)
    x = C.random_x((40, 384), torch.float16)
    r, Eb = C.reference(x, p, bias)
    y = m(x.to(DEV))
    C.assert_within_bound(y, r, Eb, torch.float16, "PackedLinear, 40 rows")
    assert same_bits(y, direct(x.to(DEV), to_dev(p), bias.to(DEV)))


def test_no_weight_sized_temporary():
    """a [512, 4096] weight is 8 MiB in float32 and 1 MiB as 4-bit codes: the call allocates y and nothing of that size"""
    N, K, G, bits = 512, 4096, 128, 4
    pg = to_dev(C.exact_packed(N, K, G, bits))
    x = C.exact_x((17, K), torch.bfloat16).to(DEV)
    lsq_linear_packed(x, pg)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y = lsq_linear_packed(x, pg)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < N * K // 2, "a temporary as large as the codes was allocated"
    assert y.shape == (17, N)


def test_error_paths_raise_and_launch_nothing():
    N, K, G, bits = 8, 64, 32, 4
    p = C.random_packed(N, K, G, bits)
    pg = to_dev(p)
    x = C.random_x((17, K), torch.bfloat16).to(DEV)
    with pytest.raises(RuntimeError, match="K = 64"):
        lsq_linear_packed(x[:, :32], pg)
    with pytest.raises(RuntimeError, match="bits must be 4 or 2"):
        torch.ops.torchlsq.lsq_linear_packed(x, pg.codes, pg.scale.reshape(-1), pg.zero_point.reshape(-1), None, G, 3)
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_linear_packed(x.clone().requires_grad_(True), pg)
    with pytest.raises(RuntimeError, match="bias needs 8 values"):
        lsq_linear_packed(x, pg, torch.zeros(7, device=DEV))
    # the library refuses what it does not serve and leaves y alone
    lib = E.qgemm_library()
    x32 = x.float()
    y = torch.full((17, N), 7.0, device=DEV)
    rc = lib.lsq_qgemm_forward(E.LSQ_F32, x32.data_ptr(), 17, pg.codes.data_ptr(), N, K, G, bits, pg.scale.data_ptr(),
                               pg.zero_point.data_ptr(), None, 0, y.data_ptr(), None)
    assert rc == -1 and b"not served" in lib.lsq_qgemm_last_error()
    yb = torch.full((17, N), 7.0, device=DEV, dtype=torch.bfloat16)
    rc = lib.lsq_qgemm_forward(E.LSQ_BF16, x.data_ptr(), 17, pg.codes.data_ptr() + 1, N, K, G, bits, pg.scale.data_ptr(),
                               pg.zero_point.data_ptr(), None, 0, yb.data_ptr(), None)
    assert rc == -1 and b"16-byte aligned" in lib.lsq_qgemm_last_error()
    rc = lib.lsq_qgemm_forward(E.LSQ_BF16, x.data_ptr(), 0, pg.codes.data_ptr(), N, K, G, bits, pg.scale.data_ptr(),
                               pg.zero_point.data_ptr(), None, 0, yb.data_ptr(), None)
    assert rc == -1 and b"rows of x" in lib.lsq_qgemm_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((yb == 7.0).all())
    assert lsq_linear_packed(x, pg).shape == (17, N)
