"""GPU: the linear op on packed group-wise weights (liblsq_hip_qlinear.so -> torchlsq.functional.lsq_linear_packed /
torchlsq.quantized.PackedLinear) against the fp64 reference, the bound and the exact-arithmetic inputs of
tests/qlinear_cases.py (its docstring derives the bound).

  * the bound and the exact test over the shapes at which the forms differ, three dtypes, with and without a bias, for x of
    [2, 3, K], an x[1:] view and codes at byte offset 1 of a larger buffer (the generic form);
  * zero points near 100 (an affine export in a -128..127 type) and far beyond the code range (the three-piece path);
  * M = 17, the dequantize-and-matmul route: the bound only;
  * repeated launches are bit-identical, and rows of the 16- and 5-row calls are the 1-row calls bit for bit;
  * shape-only tracing, a captured graph, the error paths, and the plan's native row limit.
"""
import pytest
import torch
import torchlsq  # noqa: F401  (registers torch.ops.torchlsq.*)

import qlinear_cases as C
from torchlsq.functional import PackedGroupTensor, lsq_linear_packed

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_id = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))


def to_dev(p):
    return PackedGroupTensor(p.codes.to(DEV), p.scale.to(DEV), p.zero_point.to(DEV), p.bits, p.group_size, p.quant_min, p.shape)


@pytest.mark.parametrize("dtype", C.DTYPES, **_id)
@pytest.mark.parametrize("shape", C.SHAPES + C.SHAPES_EXTRA, **_id)
def test_bound_and_exact(shape, dtype):
    M, N, K, G, bits = shape
    p = C.random_packed(N, K, G, bits, seed=M)
    pg = to_dev(p)
    x = C.random_x((M, K), dtype, seed=N)
    for bias in (None, C.random_bias(N, torch.float32, seed=K), C.random_bias(N, dtype, seed=K)):
        r, E = C.reference(x, p, bias)
        y = lsq_linear_packed(x.to(DEV), pg, None if bias is None else bias.to(DEV))
        C.assert_within_bound(y, r, E, dtype, "gpu %s bias %s" % (shape, None if bias is None else bias.dtype))
        C.assert_within_bound(lsq_linear_packed(x, p, bias), r, E, dtype, "cpu path")
    if K <= 4096:
        pe, xe = C.exact_packed(N, K, G, bits, seed=M), C.exact_x((M, K), dtype, seed=N)
        r, _ = C.reference(xe, pe)
        C.assert_exact(lsq_linear_packed(xe.to(DEV), to_dev(pe)), r, dtype, "gpu exact %s" % (shape,))


@pytest.mark.parametrize("dtype", C.DTYPES, **_id)
def test_views_of_x_and_of_the_codes(dtype):
    """x of [2, 3, K] is a 6-row call; x[1:] is element-aligned only; codes at byte offset 1 take the generic form"""
    N, K, G, bits = 21, 256, 32, 4
    p, pe = C.random_packed(N, K, G, bits, seed=5), C.exact_packed(N, K, G, bits, seed=5)
    x3, xe3 = C.random_x((2, 3, K), dtype), C.exact_x((2, 3, K), dtype)
    r, E = C.reference(x3, p)
    re_, _ = C.reference(xe3, pe)
    y = lsq_linear_packed(x3.to(DEV), to_dev(p))
    assert y.shape == (2, 3, N)
    C.assert_within_bound(y, r, E, dtype, "x [2, 3, K]")
    C.assert_exact(lsq_linear_packed(xe3.to(DEV), to_dev(pe)), re_, dtype, "x [2, 3, K]")
    # an x[1:]-style view: a storage offset of one element
    flat = torch.zeros(6 * K + 1, dtype=dtype, device=DEV)
    flat[1:] = xe3.reshape(-1).to(DEV)
    xv = flat[1:].view(2, 3, K)
    assert xv.data_ptr() % 16 != 0
    C.assert_exact(lsq_linear_packed(xv, to_dev(pe)), re_, dtype, "x[1:]")
    # the codes as a view at byte offset 1 of a larger buffer
    for q, xx, exact in ((p, x3, False), (pe, xe3, True)):
        buf = torch.zeros(q.codes.numel() + 1, dtype=torch.uint8, device=DEV)
        buf[1:] = q.codes.reshape(-1).to(DEV)
        qv = PackedGroupTensor(buf[1:].view(N, -1), q.scale.to(DEV), q.zero_point.to(DEV), bits, G, q.quant_min, q.shape)
        assert qv.codes.data_ptr() % 16 != 0 and qv.codes.is_contiguous()
        yv = lsq_linear_packed(xx.to(DEV), qv)
        if exact:
            C.assert_exact(yv, re_, dtype, "codes at byte offset 1")
        else:
            C.assert_within_bound(yv, r, E, dtype, "codes at byte offset 1")


@pytest.mark.parametrize("dtype", C.DTYPES, **_id)
def test_zero_points_near_100_and_far_outside_the_code_range(dtype):
    for what, p in (("affine export, qzero near 100", C.affine_packed(19, 256, 32)),
                    ("far zero points, 4 bits", C.far_packed(19, 256, 32, 4)),
                    ("far zero points, 2 bits", C.far_packed(7, 512, 64, 2)),
                    ("far zero points, generic form", C.far_packed(5, 48, 8, 4))):
        K = p.shape[1]
        for M in (1, 16):
            x = C.random_x((M, K), dtype, seed=M)
            bias = C.random_bias(p.shape[0], torch.float32)
            r, E = C.reference(x, p, bias)
            C.assert_within_bound(lsq_linear_packed(x.to(DEV), to_dev(p), bias.to(DEV)), r, E, dtype, "%s, M = %d" % (what, M))


@pytest.mark.parametrize("dtype", C.DTYPES, **_id)
def test_seventeen_rows_take_the_dequantize_route(dtype):
    N, K, G, bits = 67, 384, 128, 4
    p = C.random_packed(N, K, G, bits, seed=17)
    x = C.random_x((17, K), dtype, seed=17)
    for bias in (None, C.random_bias(N, torch.float32), C.random_bias(N, dtype)):
        r, E = C.reference(x, p, bias)
        y = lsq_linear_packed(x.to(DEV), to_dev(p), None if bias is None else bias.to(DEV))
        C.assert_within_bound(y, r, E, dtype, "M = 17, bias %s" % (None if bias is None else bias.dtype))


@pytest.mark.parametrize("shape", [(16, 67, 384, 128, 4), (5, 9, 24, 8, 4)], **_id)
def test_repeated_launches_are_bit_identical(shape):
    M, N, K, G, bits = shape
    pg = to_dev(C.random_packed(N, K, G, bits))
    x = C.random_x((M, K), torch.bfloat16).to(DEV)
    bias = C.random_bias(N, torch.float32).to(DEV)
    first = lsq_linear_packed(x, pg, bias)
    for _ in range(19):
        assert torch.equal(lsq_linear_packed(x, pg, bias).view(torch.int16), first.view(torch.int16))


@pytest.mark.parametrize("dtype", C.DTYPES, **_id)
@pytest.mark.parametrize("shape", [(67, 384, 128, 4), (33, 4800, 96, 4), (5, 4096, 128, 2), (9, 24, 8, 4)], **_id)
def test_batch_invariance(shape, dtype):
    """row m of the 16- and of the 5-row call is the 1-row call on x[m], bit for bit"""
    N, K, G, bits = shape
    pg = to_dev(C.random_packed(N, K, G, bits))
    x = C.random_x((16, K), dtype).to(DEV)
    bias = C.random_bias(N, dtype).to(DEV)
    y16, y5 = lsq_linear_packed(x, pg, bias), lsq_linear_packed(x[:5], pg, bias)
    for m in range(16):
        y1 = lsq_linear_packed(x[m:m + 1], pg, bias)
        assert torch.equal(y16[m:m + 1].view(C.INT[dtype]), y1.view(C.INT[dtype])), "row %d of 16" % m
        if m < 5:
            assert torch.equal(y5[m:m + 1].view(C.INT[dtype]), y1.view(C.INT[dtype])), "row %d of 5" % m


def test_fake_tracing_and_a_captured_graph():
    N, K, G, bits = 67, 384, 128, 4
    pg = to_dev(C.random_packed(N, K, G, bits))
    bias = C.random_bias(N, torch.float32).to(DEV)
    args = (pg.codes, pg.scale.reshape(-1), pg.zero_point.reshape(-1), bias)

    def f(x, codes, scale, zp, b):
        return torch.ops.torchlsq.lsq_linear_packed(x, codes, scale, zp, b, G, bits)

    x = C.random_x((2, 3, K), torch.bfloat16).to(DEV)
    want = f(x, *args)
    out = torch.compile(f, backend="aot_eager", fullgraph=True)(x, *args)
    assert out.shape == (2, 3, N) and out.dtype == torch.bfloat16 and torch.equal(out, want)
    # capture (after the warm-up call above), then replay on new contents of the static input
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f(static_x, *args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = f(static_x, *args)
    x2 = C.random_x((2, 3, K), torch.bfloat16, seed=9).to(DEV)
    static_x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_y, f(x2, *args))


def test_error_paths_raise_and_launch_nothing():
    N, K, G, bits = 8, 64, 32, 4
    p = C.random_packed(N, K, G, bits)
    pg = to_dev(p)
    x = C.random_x((2, K), torch.bfloat16).to(DEV)
    with pytest.raises(RuntimeError, match="K = 64"):
        lsq_linear_packed(x[:, :32], pg)
    with pytest.raises(RuntimeError, match="bits must be 4 or 2"):
        torch.ops.torchlsq.lsq_linear_packed(x, pg.codes, pg.scale.reshape(-1), pg.zero_point.reshape(-1), None, G, 3)
    p64 = PackedGroupTensor(pg.codes, pg.scale.double(), pg.zero_point, bits, G, p.quant_min, p.shape)
    with pytest.raises(RuntimeError, match="float64 scale"):
        lsq_linear_packed(x, p64)
    with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
        lsq_linear_packed(x.double(), pg)
    with pytest.raises(RuntimeError, match="GPU|all tensors on"):
        lsq_linear_packed(x.cpu(), pg)
    with pytest.raises(RuntimeError, match="GPU|all tensors on"):
        lsq_linear_packed(x, p)
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_linear_packed(x.clone().requires_grad_(True), pg)
    torch.cuda.synchronize()
    assert lsq_linear_packed(x, pg).shape == (2, N)


def test_the_plan_agrees_with_the_native_row_limit():
    """inside the plan's native rows a call is batch-invariant (the native kernel); the row count beyond is refused by the C
    entry point and served by the dequantize route, which the plan refuses to describe"""
    from torchlsq import extension as E
    N, K, G, bits = 67, 384, 128, 4
    pl = E.qlinear_plan(torch.bfloat16, 16, N, K, G, bits)
    rows = pl["native_rows"]
    assert rows == 16 and pl["form"] == "mfma" and pl["grid"] == 5
    assert E.qlinear_plan(torch.float32, 16, N, K, G, bits)["form"] == "generic"
    with pytest.raises(RuntimeError, match="serves 1 to 16"):
        E.qlinear_plan(torch.bfloat16, rows + 1, N, K, G, bits)
    pg = to_dev(C.random_packed(N, K, G, bits))
    x = C.random_x((rows + 1, K), torch.bfloat16).to(DEV)
    y = torch.empty(rows + 1, N, dtype=torch.bfloat16, device=DEV)
    lib = E.qlinear_library()
    rc = lib.lsq_qlinear_forward(E.LSQ_BF16, x.data_ptr(), rows + 1, pg.codes.data_ptr(), N, K, G, bits, pg.scale.data_ptr(),
                                 pg.zero_point.data_ptr(), None, 0, y.data_ptr(), None)
    assert rc == -1 and b"serves 1 to 16" in lib.lsq_qlinear_last_error()
    full = lsq_linear_packed(x[:rows], pg)
    assert torch.equal(full[rows - 1:].view(torch.int16), lsq_linear_packed(x[rows - 1:rows], pg).view(torch.int16))
    assert lsq_linear_packed(x, pg).shape == (rows + 1, N)


def test_packed_linear_module_on_the_gpu():
    from torchlsq.quantized import PackedLinear
    p = C.random_packed(67, 384, 128, 4)
    bias = C.random_bias(67, torch.float32)
    m = PackedLinear.from_packed(p, bias).to(DEV)
    x = C.random_x((4, 384), torch.float16)
    r, E = C.reference(x, p, bias)
    C.assert_within_bound(m(x.to(DEV)), r, E, torch.float16, "PackedLinear")
    other = PackedLinear(384, 67, bits=4, group_size=128, quant_min=0).to(DEV)
    other.load_state_dict(m.state_dict())
    assert torch.equal(other(x.to(DEV)), m(x.to(DEV)))
