"""GPU: the 8-bit-activation linear op on packed group-wise weights (liblsq_hip_qlinear_a8.so ->
torch.ops.torchlsq.lsq_linear_packed_q8 / lsq_linear_packed_a8, torchlsq.quantized.PackedLinearA8) against the int64 / float64
reference, the bound and the exact-arithmetic inputs of tests/qlinear_a8_cases.py (its docstring derives the bound).

  * the bound and the exact test over the shapes at which the forms differ, three output types, both level types, with and
    without a bias; lx - zx that fits a byte and that does not;
  * zero points of 70000, -5000, 300 and 2^23 (a 32-bit correction overflows), under the bound and in an exact case;
  * the fused form (floating x in) is the levels form on lsq_levels_per_tensor's bytes, bit for bit, NaN / inf / -0.0 /
    borders / a tie included;
  * repeated launches are bit-identical; rows of the 2-, 5- and 16-row calls are the 1-row calls bit for bit, both forms;
    a non-contiguous x, codes at a byte offset (the generic form);
  * M = 17 (beyond one launch's rows: the bound), empty M and N, shape-only tracing, a captured graph, the error paths, the
    module.
"""
import pytest
import torch
import torchlsq  # noqa: F401  (registers torch.ops.torchlsq.*)

import qlinear_a8_cases as A
import qlinear_cases as C
from torchlsq.functional import PackedGroupTensor, lsq_linear_packed_a8

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_id = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))
QUANTIZERS = [(0.05, 0.0, -128, 127, -128, 127), (0.03, -1.7, 0, 255, 0, 255), (0.04, 0.6, 0, 127, 0, 255)]


def to_dev(p):
    return PackedGroupTensor(p.codes.to(DEV), p.scale.to(DEV), p.zero_point.to(DEV), p.bits, p.group_size, p.quant_min, p.shape)


def q8(lx, s_x, zx, p, bias, dtype):
    s, z = A.act(s_x, zx, lx.device)
    return torch.ops.torchlsq.lsq_linear_packed_q8(lx, s, z, p.codes, p.scale.reshape(-1), p.zero_point.reshape(-1), bias,
                                                   p.group_size, p.bits, dtype)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(C.INT[a.dtype]), b.view(C.INT[b.dtype]))


@pytest.mark.parametrize("dtype", A.DTYPES, **_id)
@pytest.mark.parametrize("shape", A.SHAPES, **_id)
def test_bound_and_exact(shape, dtype):
    M, N, K, G, bits = shape
    p = C.random_packed(N, K, G, bits, seed=M)
    pg = to_dev(p)
    for lo, hi, zx in ((0, 255, 3), (-128, 127, -7)):
        lx = A.levels((M, K), lo, hi, seed=N)
        for bias in (None, C.random_bias(N, torch.float32, seed=K), C.random_bias(N, dtype, seed=K)):
            r, E = A.reference(lx, 0.02, zx, p, bias)
            y = q8(lx.to(DEV), 0.02, zx, pg, None if bias is None else bias.to(DEV), dtype)
            C.assert_within_bound(y, r, E, dtype, "gpu %s levels %d..%d bias %s" % (shape, lo, hi, None if bias is None else bias.dtype))
    if K <= 4096:
        pe = C.exact_packed(N, K, G, bits, seed=M)
        peg = to_dev(pe)
        # 0..255 with zx = 0 (lx - zx does not fit a byte), with zx = 131 (it does), and -128..127 with a negative zx
        for lo, hi, zx in ((0, 255, 0), (0, 255, 131), (-128, 127, -5)):
            lx = A.levels((M, K), lo, hi, seed=N)
            r, _ = A.reference(lx, A.S_X_EXACT, zx, pe)
            C.assert_exact(q8(lx.to(DEV), A.S_X_EXACT, zx, peg, None, dtype), r, dtype, "gpu exact %s zx %d" % (shape, zx))


@pytest.mark.parametrize("dtype", A.DTYPES, **_id)
def test_wide_zero_points(dtype):
    for what, p in (("4 bits", A.wide_packed(19, 256, 32, 4)), ("2 bits", A.wide_packed(7, 512, 64, 2)),
                    ("4 bits, two packets per MFMA", A.wide_packed(19, 256, 64, 4)), ("generic form", A.wide_packed(5, 48, 8, 4))):
        for M in (1, 16):
            lx = A.levels((M, p.shape[1]), 0, 255, seed=M)
            bias = C.random_bias(p.shape[0], torch.float32)
            r, E = A.reference(lx, 0.5, 128, p, bias)
            C.assert_within_bound(q8(lx.to(DEV), 0.5, 128, to_dev(p), bias.to(DEV), dtype), r, E, dtype,
                                  "wide zero points, %s, M = %d" % (what, M))
    for pe in (A.wide_exact_packed(19, 256, 32, 4), A.wide_exact_packed(7, 256, 64, 2), A.wide_exact_packed(5, 48, 8, 4)):
        assert int(pe.zero_point.max()) == 1 << 23
        lx = A.levels((3, pe.shape[1]), 0, 255, seed=1)
        r, _ = A.reference(lx, A.S_X_EXACT, 0, pe)
        C.assert_exact(q8(lx.to(DEV), A.S_X_EXACT, 0, to_dev(pe), None, dtype), r, dtype, "exact, wide zero points")


@pytest.mark.parametrize("dtype", A.DTYPES, **_id)
@pytest.mark.parametrize("quant", QUANTIZERS, **_id)
def test_fused_form_is_the_levels_form(quant, dtype):
    scale, shift, qmin, qmax, tmin, tmax = quant
    sc, sh = torch.tensor([scale], device=DEV), torch.tensor([shift], device=DEV)
    zx = int(torch.tensor(-shift / scale).clamp(tmin, tmax).round())
    for N, K, G, bits in ((17, 96, 32, 4), (9, 256, 64, 4), (5, 128, 64, 2), (9, 24, 8, 4)):      # three matrix-core kernels, generic
        p = C.random_packed(N, K, G, bits)
        pg = to_dev(p)
        x = A.special_x(3, K, dtype, scale, shift, qmin, qmax)
        bias = C.random_bias(N, torch.float32)
        y = lsq_linear_packed_a8(x.to(DEV), pg, bias.to(DEV), sc, sh, qmin, qmax, tmin, tmax)
        lv = torch.ops.torchlsq.lsq_levels_per_tensor(x.to(DEV), sc, sh, qmin, qmax, tmin, tmax, 0)
        assert int(lv[0, 0]) == (qmin if qmin < 128 else qmin - 256)               # the NaN went to quant_min
        lv = lv.view(torch.uint8) if tmax > 127 else lv
        want = q8(lv, scale, zx, pg, bias.to(DEV), dtype)
        assert same_bits(y, want), "fused != levels form, %s" % ((N, K, G, bits),)
        r, E = A.reference(lv, scale, zx, p, bias)
        C.assert_within_bound(y, r, E, dtype, "fused %s" % ((N, K, G, bits),))
        C.assert_within_bound(lsq_linear_packed_a8(x, p, bias, sc.cpu(), sh.cpu(), qmin, qmax, tmin, tmax), r, E, dtype, "cpu fused")


@pytest.mark.parametrize("shape", [(16, 67, 384, 128, 4), (5, 9, 24, 8, 4)], **_id)
def test_repeated_launches_are_bit_identical(shape):
    M, N, K, G, bits = shape
    pg = to_dev(C.random_packed(N, K, G, bits))
    lx = A.levels((M, K), 0, 255).to(DEV)
    x = C.random_x((M, K), torch.bfloat16).to(DEV)
    sc, sh = torch.tensor([0.02], device=DEV), torch.tensor([-2.5], device=DEV)         # zero point 125
    bias = C.random_bias(N, torch.float32).to(DEV)
    first, first_f = q8(lx, 0.02, 3, pg, bias, torch.bfloat16), lsq_linear_packed_a8(x, pg, bias, sc, sh, 0, 255)
    for _ in range(19):
        assert same_bits(q8(lx, 0.02, 3, pg, bias, torch.bfloat16), first)
        assert same_bits(lsq_linear_packed_a8(x, pg, bias, sc, sh, 0, 255), first_f)


@pytest.mark.parametrize("dtype", A.DTYPES, **_id)
@pytest.mark.parametrize("shape", [(67, 384, 128, 4), (33, 4800, 96, 4), (17, 96, 32, 4), (5, 4096, 128, 2), (9, 24, 8, 4)], **_id)
def test_row_invariance(shape, dtype):
    """row m of the 2-, 5- and 16-row calls is the 1-row call on row m, bit for bit, for both entry forms"""
    N, K, G, bits = shape
    pg = to_dev(C.random_packed(N, K, G, bits))
    lx = A.levels((16, K), 0, 255).to(DEV)
    x = C.random_x((16, K), dtype).to(DEV)
    sc, sh = torch.tensor([0.02], device=DEV), torch.tensor([-2.5], device=DEV)         # zero point 125
    bias = C.random_bias(N, dtype).to(DEV)
    forms = ((lambda rows: q8(lx[rows], 0.02, 3, pg, bias, dtype)),
             (lambda rows: lsq_linear_packed_a8(x[rows], pg, bias, sc, sh, 0, 255)))
    for f in forms:
        many = {n: f(slice(0, n)) for n in (2, 5, 16)}
        for m in range(16):
            y1 = f(slice(m, m + 1))
            for n, yn in many.items():
                if m < n:
                    assert same_bits(yn[m:m + 1], y1), "row %d of %d" % (m, n)


@pytest.mark.parametrize("dtype", A.DTYPES, **_id)
def test_views_of_x_and_of_the_codes(dtype):
    """a non-contiguous x for both entry forms; codes at byte offset 1 of a larger buffer take the generic form (the plan
    describes a 16-byte aligned pointer: mfma for this format, generic for G = 8) and give the same exact result"""
    from torchlsq import extension as E
    N, K, G, bits = 21, 256, 32, 4
    pe = C.exact_packed(N, K, G, bits, seed=5)
    lx = A.levels((2, 3, K), 0, 255)
    r, _ = A.reference(lx, A.S_X_EXACT, 7, pe)
    C.assert_exact(q8(lx.to(DEV), A.S_X_EXACT, 7, to_dev(pe), None, dtype), r, dtype, "x [2, 3, K]")
    wide = torch.zeros(2, 3, 2 * K, dtype=torch.uint8, device=DEV)
    wide[..., ::2] = lx.to(DEV)
    assert not wide[..., ::2].is_contiguous()
    C.assert_exact(q8(wide[..., ::2], A.S_X_EXACT, 7, to_dev(pe), None, dtype), r, dtype, "non-contiguous levels")
    xs = C.exact_x((6, 2 * K), dtype).to(DEV)
    sc, sh = torch.tensor([1.0], device=DEV), torch.tensor([-8.0], device=DEV)         # zero point 8: levels x + 8 in 0..16
    yv = lsq_linear_packed_a8(xs[:, ::2], to_dev(pe), None, sc, sh, 0, 255)
    assert same_bits(yv, lsq_linear_packed_a8(xs[:, ::2].contiguous(), to_dev(pe), None, sc, sh, 0, 255))
    buf = torch.zeros(pe.codes.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = pe.codes.reshape(-1).to(DEV)
    qv = PackedGroupTensor(buf[1:].view(N, -1), pe.scale.to(DEV), pe.zero_point.to(DEV), bits, G, pe.quant_min, pe.shape)
    assert qv.codes.data_ptr() % 16 != 0 and qv.codes.is_contiguous()
    assert E.qlinear_a8_plan(6, N, K, G, bits)["form"] == "mfma" and E.qlinear_a8_plan(6, N, 24, 8, bits)["form"] == "generic"
    C.assert_exact(q8(lx.to(DEV), A.S_X_EXACT, 7, qv, None, dtype), r, dtype, "codes at byte offset 1")


@pytest.mark.parametrize("dtype", A.DTYPES, **_id)
def test_seventeen_rows_meet_the_bound_through_the_prefill_route(dtype):
    N, K, G, bits = 67, 384, 128, 4
    p = C.random_packed(N, K, G, bits, seed=17)
    lx = A.levels((17, K), 0, 255, seed=17)
    x = C.random_x((17, K), dtype, seed=17)
    sc, sh = torch.tensor([0.02], device=DEV), torch.tensor([-2.0], device=DEV)         # zero point 100
    for bias in (None, C.random_bias(N, torch.float32), C.random_bias(N, dtype)):
        bg = None if bias is None else bias.to(DEV)
        r, E = A.reference(lx, 0.02, 100, p, bias)
        C.assert_within_bound(q8(lx.to(DEV), 0.02, 100, to_dev(p), bg, dtype), r, E, dtype, "M = 17, levels in")
        lv = torch.ops.torchlsq.lsq_levels_per_tensor(x.to(DEV), sc, sh, 0, 255, 0, 255, 0).view(torch.uint8)
        r, E = A.reference(lv, 0.02, 100, p, bias)
        C.assert_within_bound(lsq_linear_packed_a8(x.to(DEV), to_dev(p), bg, sc, sh, 0, 255), r, E, dtype, "M = 17, floating x in")


@pytest.mark.parametrize("shape", [(67, 384, 128, 4), (9, 24, 8, 4)], **_id)
def test_rows_beyond_one_launch_are_the_one_row_calls(shape):
    """33 rows are three launches (16 + 16 + 1): every row is still the 1-row call, bit for bit, for both entry forms and a
    [3, 11, K] x"""
    N, K, G, bits = shape
    pg = to_dev(C.random_packed(N, K, G, bits))
    lx = A.levels((33, K), 0, 255).to(DEV)
    x = C.random_x((3, 11, K), torch.bfloat16).to(DEV)
    sc, sh = torch.tensor([0.02], device=DEV), torch.tensor([-2.5], device=DEV)         # zero point 125
    bias = C.random_bias(N, torch.float32).to(DEV)
    y = q8(lx, 0.02, 3, pg, bias, torch.float16)
    assert y.shape == (33, N)
    for m in (0, 15, 16, 31, 32):
        assert same_bits(y[m:m + 1], q8(lx[m:m + 1], 0.02, 3, pg, bias, torch.float16)), "levels in, row %d" % m
    y = lsq_linear_packed_a8(x, pg, bias, sc, sh, 0, 255)
    assert y.shape == (3, 11, N)
    for m in (0, 15, 16, 31, 32):
        assert same_bits(y.reshape(33, N)[m:m + 1], lsq_linear_packed_a8(x.reshape(33, K)[m:m + 1], pg, bias, sc, sh, 0, 255)), \
            "floating x in, row %d" % m


def test_empty_shapes_fake_tracing_and_a_captured_graph():
    N, K, G, bits = 67, 384, 128, 4
    p = C.random_packed(N, K, G, bits)
    pg = to_dev(p)
    sc, sh = torch.tensor([0.02], device=DEV), torch.tensor([-2.5], device=DEV)         # zero point 125
    x = C.random_x((2, 3, K), torch.bfloat16).to(DEV)
    assert lsq_linear_packed_a8(x[:0], pg, None, sc, sh, 0, 255).shape == (0, 3, N)
    empty = PackedGroupTensor(pg.codes[:0], pg.scale[:0], pg.zero_point[:0], bits, G, -8, (0, K))
    assert lsq_linear_packed_a8(x, empty, None, sc, sh, 0, 255).shape == (2, 3, 0)
    assert q8(A.levels((0, K), 0, 255).to(DEV), 0.1, 0, pg, None, torch.float16).shape == (0, N)
    bias = C.random_bias(N, torch.float32).to(DEV)
    args = (sc, sh, pg.codes, pg.scale.reshape(-1), pg.zero_point.reshape(-1), bias)

    def f(x, sc, sh, codes, scale, zp, b):
        return torch.ops.torchlsq.lsq_linear_packed_a8(x, sc, sh, 0, 255, 0, 255, codes, scale, zp, b, G, bits)

    want = f(x, *args)
    out = torch.compile(f, backend="aot_eager", fullgraph=True)(x, *args)
    assert out.shape == (2, 3, N) and out.dtype == torch.bfloat16 and torch.equal(out, want)
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
    from torchlsq.quantized import PackedLinearA8
    N, K, G, bits = 8, 64, 32, 4
    p = C.random_packed(N, K, G, bits)
    pg = to_dev(p)
    x = C.random_x((2, K), torch.bfloat16).to(DEV)
    sc, sh = torch.tensor([0.02], device=DEV), torch.tensor([-2.5], device=DEV)         # zero point 125
    with pytest.raises(RuntimeError, match="K = 64"):
        lsq_linear_packed_a8(x[:, :32], pg, None, sc, sh, 0, 255)
    with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
        lsq_linear_packed_a8(x.double(), pg, None, sc.double(), sh.double(), 0, 255)
    with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
        q8(A.levels((2, K), 0, 255).to(DEV), 0.1, 0, pg, None, torch.float64)
    p64 = PackedGroupTensor(pg.codes, pg.scale.double(), pg.zero_point, bits, G, p.quant_min, p.shape)
    with pytest.raises(RuntimeError, match="float64 scale"):
        lsq_linear_packed_a8(x, p64, None, sc, sh, 0, 255)
    with pytest.raises(RuntimeError, match="GPU|all tensors on"):
        lsq_linear_packed_a8(x.cpu(), pg, None, sc, sh, 0, 255)
    with pytest.raises(RuntimeError, match="GPU|all tensors on"):
        lsq_linear_packed_a8(x, pg, None, sc.cpu(), sh, 0, 255)
    with pytest.raises(RuntimeError, match="inference-only"):
        lsq_linear_packed_a8(x.clone().requires_grad_(True), pg, None, sc, sh, 0, 255)
    from torch.ao.quantization.observer import MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    pc = LSQFakeQuantizer(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                          qscheme=torch.per_channel_symmetric, quant_min=-64, quant_max=63)
    pc(torch.randn(8, 64))
    with pytest.raises(ValueError, match="per-tensor"):
        PackedLinearA8.from_packed(p, None, pc)
    torch.cuda.synchronize()
    assert lsq_linear_packed_a8(x, pg, None, sc, sh, 0, 255).shape == (2, N)


def test_packed_linear_a8_module_on_the_gpu():
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer, PackedLinearA8
    q = LSQFakeQuantizer(observer=MovingAverageMinMaxObserver, otype="activation", dtype=torch.quint8,
                         qscheme=torch.per_tensor_affine, quant_min=0, quant_max=127)
    q.train()
    for i in range(3):
        q(C.random_x((8, 384), torch.float32, seed=i))
    q.disable_observer()
    q.eval()
    p = C.random_packed(67, 384, 128, 4)
    bias = C.random_bias(67, torch.float32)
    m = PackedLinearA8.from_packed(p, bias, q).to(DEV)
    x = C.random_x((4, 384), torch.float16)
    xq = q.quantize(x.float())
    lv = torch.ops.torchlsq.lsq_levels_per_tensor(x.to(DEV), m.input_scale, m.input_shift, 0, 127, 0, 255, 0).view(torch.uint8)
    r, E = A.reference(lv, xq.q_scale(), xq.q_zero_point(), p, bias)
    y = m(x.to(DEV))
    C.assert_within_bound(y, r, E, torch.float16, "PackedLinearA8")
    other = PackedLinearA8(384, 67, bits=4, group_size=128, quant_min=0, input_range=(-128, 127, -128, 127)).to(DEV)
    other.load_state_dict(m.state_dict())
    assert torch.equal(other(x.to(DEV)), y)
