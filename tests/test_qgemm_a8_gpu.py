"""GPU: the int8 matrix-core GEMM on packed group-wise weights (liblsq_hip_qgemm_a8.so), called directly so that the
threshold of rows does not matter, against the decode kernel 16 rows at a time -- "the block route": the existing ops
called with at most 16 rows -- bit for bit, and against the int64 / float64 reference, the bound and the exact-arithmetic
inputs of tests/qlinear_a8_cases.py.

  * every row of a 17-, 33-, 129-row call, and of the calls on both sides of every row count at which the plan changes SUBS
    or the tile's width, is the block route bit for bit: both level types, three types of x, three of y, three kinds of bias;
  * the bound and the exact inputs; zero points of 300, -5000, 70000 and 2^23;
  * the fused form is the levels form on lsq_levels_per_tensor's bytes, NaN / inf / -0.0 / borders / a tie beyond row 16;
  * repeated launches; a row's bits at positions 0, 16 and 128; views of x; codes at a byte offset;
  * through the ops at the threshold and below it (a spy on the host module), a captured graph, the module.
"""
import pytest
import torch
import torchlsq  # noqa: F401  (registers torch.ops.torchlsq.*)

import qlinear_a8_cases as A
import qlinear_cases as C
from torchlsq import _qgemm_a8_host, _qlinear_a8_host
from torchlsq import extension as E
from torchlsq.functional import PackedGroupTensor, lsq_linear_packed_a8

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_id = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))
# (N, K, G, bits): 3 spans, 13 empty chains, N no multiple of 16; 3 packets per group, spans of 12 packets, two chunks, the
# last ragged; a partial span; 2 bits, every chain one span; two packets per MFMA, three chunks, chains of several spans
FORMATS = [(67, 384, 128, 4), (33, 4800, 96, 4), (17, 96, 32, 4), (5, 4096, 128, 2), (21, 8320, 64, 4)]
# 17, 33, 129 and both sides of where SUBS changes (32 | 33, 64 | 65) and of one full 128-row tile (128 | 129)
ROWS = [17, 32, 33, 64, 65, 128, 129]
BLOCK = 16


def to_dev(p):
    return PackedGroupTensor(p.codes.to(DEV), p.scale.to(DEV), p.zero_point.to(DEV), p.bits, p.group_size, p.quant_min, p.shape)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(C.INT[a.dtype]), b.view(C.INT[b.dtype]))


def gemm_levels(lx, s_x, zx, p, bias, dtype):
    """the library, directly: one call for all rows"""
    s, z = A.act(s_x, zx, lx.device)
    return E.qgemm_a8_forward_levels(lx.contiguous(), s, z, p.codes, p.scale.reshape(-1), p.zero_point.reshape(-1), bias,
                                     p.group_size, p.bits, dtype)


def gemm_fused(x, sc, sh, rng, p, bias):
    return E.qgemm_a8_forward(x.contiguous(), sc, sh, *rng, p.codes, p.scale.reshape(-1), p.zero_point.reshape(-1), bias,
                              p.group_size, p.bits)


def block_levels(lx, s_x, zx, p, bias, dtype):
    """the block route: the existing op, at most 16 rows per call"""
    s, z = A.act(s_x, zx, lx.device)
    assert E.qgemm_a8_min_rows() > BLOCK
    return torch.cat([torch.ops.torchlsq.lsq_linear_packed_q8(lx[m0:m0 + BLOCK], s, z, p.codes, p.scale.reshape(-1),
                                                              p.zero_point.reshape(-1), bias, p.group_size, p.bits, dtype)
                      for m0 in range(0, lx.size(0), BLOCK)])


def block_fused(x, sc, sh, rng, p, bias):
    return torch.cat([lsq_linear_packed_a8(x[m0:m0 + BLOCK], p, bias, sc, sh, *rng) for m0 in range(0, x.size(0), BLOCK)])


def biases(N, dtype):
    return (None, C.random_bias(N, torch.float32).to(DEV), C.random_bias(N, dtype, seed=1).to(DEV))


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("fmt", FORMATS, **_id)
def test_every_row_is_the_block_route_bit_for_bit(fmt, M):
    N, K, G, bits = fmt
    pg = to_dev(C.random_packed(N, K, G, bits, seed=M))
    assert E.qgemm_a8_plan(M, N, K, G, bits)["subs"] == (2 if M <= 32 else 4 if M <= 64 else 8)
    for lo, hi, zx in ((0, 255, 3), (-128, 127, -7)):
        lx = A.levels((M, K), lo, hi, seed=N).to(DEV)
        for dtype in A.DTYPES:
            for bias in biases(N, dtype):
                y = gemm_levels(lx, 0.02, zx, pg, bias, dtype)
                assert same_bits(y, block_levels(lx, 0.02, zx, pg, bias, dtype)), \
                    "levels %d..%d, y %s, bias %s" % (lo, hi, dtype, None if bias is None else bias.dtype)
    sc, sh = torch.tensor([0.02], device=DEV), torch.tensor([-2.5], device=DEV)         # zero point 125
    for dtype in A.DTYPES:
        x = C.random_x((M, K), dtype, seed=M).to(DEV)
        for rng in ((0, 255, 0, 255), (-128, 127, -128, 127)):
            for bias in biases(N, dtype):
                y = gemm_fused(x, sc, sh, rng, pg, bias)
                assert same_bits(y, block_fused(x, sc, sh, rng, pg, bias)), \
                    "x %s, range %s, bias %s" % (dtype, rng, None if bias is None else bias.dtype)


@pytest.mark.parametrize("fmt", FORMATS, **_id)
def test_both_tile_widths(fmt):
    """a format takes 16-column tiles while 64-column tiles would leave compute units without one, and 64-column tiles from
    the next row on (N = 67: two wide column tiles): the rows of both calls are the block route's.  The rows repeat a 17-row
    pattern, so the block route is two launches."""
    N, K, G, bits = fmt
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wide = -(-N // 64)
    narrow = ((cus - 1) // wide) * 128          # row tiles * wide column tiles < compute units
    assert E.qgemm_a8_plan(narrow, N, K, G, bits)["cols_per_tile"] == 16 and E.qgemm_a8_plan(narrow + 1, N, K, G, bits)["cols_per_tile"] == 64
    pg = to_dev(C.random_packed(N, K, G, bits))
    base = A.levels((17, K), 0, 255).to(DEV)
    bias = C.random_bias(N, torch.float32).to(DEV)
    want = block_levels(base, 0.02, 3, pg, bias, torch.float32)
    for M in (narrow, narrow + 1):
        reps = -(-M // 17)
        y = gemm_levels(base.repeat(reps, 1)[:M], 0.02, 3, pg, bias, torch.float32)
        assert same_bits(y, want.repeat(reps, 1)[:M]), "M = %d" % M


@pytest.mark.parametrize("fmt", [(96, 32, 4), (128, 64, 4), (128, 64, 2)], **_id)
def test_wide_tiles_with_few_rows(fmt):
    """64-column tiles of 2, 4 and 8 sub-tiles: enough columns that 64-column tiles give every compute unit one"""
    K, G, bits = fmt
    N = 64 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    pg = to_dev(C.random_packed(N, K, G, bits))
    bias = C.random_bias(N, torch.float32).to(DEV)
    for M in (17, 33, 65):
        pl = E.qgemm_a8_plan(M, N, K, G, bits)
        assert pl["cols_per_tile"] == 64 and pl["subs"] == (2 if M <= 32 else 4 if M <= 64 else 8)
        lx = A.levels((M, K), 0, 255, seed=M).to(DEV)
        assert same_bits(gemm_levels(lx, 0.02, 3, pg, bias, torch.float32), block_levels(lx, 0.02, 3, pg, bias, torch.float32)), M


@pytest.mark.parametrize("M", [17, 129])
@pytest.mark.parametrize("fmt", FORMATS, **_id)
def test_bound_and_exact(fmt, M):
    N, K, G, bits = fmt
    p = C.random_packed(N, K, G, bits, seed=M)
    pg = to_dev(p)
    for lo, hi, zx in ((0, 255, 3), (-128, 127, -7)):
        lx = A.levels((M, K), lo, hi, seed=N)
        bias = C.random_bias(N, torch.float32, seed=K)
        r, Eb = A.reference(lx, 0.02, zx, p, bias)
        for dtype in A.DTYPES:
            C.assert_within_bound(gemm_levels(lx.to(DEV), 0.02, zx, pg, bias.to(DEV), dtype), r, Eb, dtype,
                                  "gemm %s M %d levels %d..%d" % (fmt, M, lo, hi))
    if K <= 4096:
        pe = C.exact_packed(N, K, G, bits, seed=M)
        for lo, hi, zx in ((0, 255, 0), (0, 255, 131), (-128, 127, -5)):
            lx = A.levels((M, K), lo, hi, seed=N)
            r, _ = A.reference(lx, A.S_X_EXACT, zx, pe)
            for dtype in A.DTYPES:
                C.assert_exact(gemm_levels(lx.to(DEV), A.S_X_EXACT, zx, to_dev(pe), None, dtype), r, dtype, "gemm exact %s zx %d" % (fmt, zx))


@pytest.mark.parametrize("dtype", A.DTYPES, **_id)
def test_wide_zero_points(dtype):
    for what, p in (("4 bits", A.wide_packed(19, 256, 32, 4)), ("2 bits", A.wide_packed(7, 512, 64, 2)),
                    ("4 bits, two packets per MFMA", A.wide_packed(19, 256, 64, 4))):
        assert {300, -5000, 70000, 1 << 23} <= set(p.zero_point.reshape(-1).tolist())
        for M in (17, 129):
            lx = A.levels((M, p.shape[1]), 0, 255, seed=M)
            bias = C.random_bias(p.shape[0], torch.float32)
            r, Eb = A.reference(lx, 0.5, 128, p, bias)
            y = gemm_levels(lx.to(DEV), 0.5, 128, to_dev(p), bias.to(DEV), dtype)
            C.assert_within_bound(y, r, Eb, dtype, "wide zero points, %s, M = %d" % (what, M))
            assert same_bits(y, block_levels(lx.to(DEV), 0.5, 128, to_dev(p), bias.to(DEV), dtype)), (what, M)
    for pe in (A.wide_exact_packed(19, 256, 32, 4), A.wide_exact_packed(7, 256, 64, 2)):
        assert int(pe.zero_point.max()) == 1 << 23
        lx = A.levels((33, pe.shape[1]), 0, 255, seed=1)
        r, _ = A.reference(lx, A.S_X_EXACT, 0, pe)
        y = gemm_levels(lx.to(DEV), A.S_X_EXACT, 0, to_dev(pe), None, dtype)
        C.assert_exact(y, r, dtype, "exact, wide zero points")
        assert same_bits(y, block_levels(lx.to(DEV), A.S_X_EXACT, 0, to_dev(pe), None, dtype))


QUANTIZERS = [(0.05, 0.0, -128, 127, -128, 127), (0.03, -1.7, 0, 255, 0, 255), (0.04, 0.6, 0, 127, 0, 255)]


@pytest.mark.parametrize("dtype", A.DTYPES, **_id)
@pytest.mark.parametrize("quant", QUANTIZERS, **_id)
def test_fused_form_is_the_levels_form(quant, dtype):
    scale, shift, qmin, qmax, tmin, tmax = quant
    sc, sh = torch.tensor([scale], device=DEV), torch.tensor([shift], device=DEV)
    zx = int(torch.tensor(-shift / scale).clamp(tmin, tmax).round())
    for N, K, G, bits in ((17, 96, 32, 4), (9, 256, 64, 4), (5, 128, 64, 2)):
        p = C.random_packed(N, K, G, bits)
        pg = to_dev(p)
        x = torch.roll(A.special_x(33, K, dtype, scale, shift, qmin, qmax), 17, 0).to(DEV)   # the special values in row 17
        assert bool(torch.isnan(x[17, 0]))
        bias = C.random_bias(N, torch.float32)
        y = gemm_fused(x, sc, sh, (qmin, qmax, tmin, tmax), pg, bias.to(DEV))
        lv = torch.ops.torchlsq.lsq_levels_per_tensor(x, sc, sh, qmin, qmax, tmin, tmax, 0)
        assert int(lv[17, 0]) == (qmin if qmin < 128 else qmin - 256)              # the NaN went to quant_min
        lv = lv.view(torch.uint8) if tmax > 127 else lv
        assert same_bits(y, gemm_levels(lv, scale, zx, pg, bias.to(DEV), dtype)), "fused != levels form, %s" % ((N, K, G, bits),)
        assert same_bits(y, block_fused(x, sc, sh, (qmin, qmax, tmin, tmax), pg, bias.to(DEV)))
        r, Eb = A.reference(lv, scale, zx, p, bias)
        C.assert_within_bound(y, r, Eb, dtype, "fused %s" % ((N, K, G, bits),))


def test_repeated_launches_are_bit_identical():
    N, K, G, bits = 67, 384, 128, 4
    pg = to_dev(C.random_packed(N, K, G, bits))
    lx = A.levels((129, K), 0, 255).to(DEV)
    x = C.random_x((129, K), torch.bfloat16).to(DEV)
    sc, sh = torch.tensor([0.02], device=DEV), torch.tensor([-2.5], device=DEV)
    bias = C.random_bias(N, torch.float32).to(DEV)
    first, first_f = gemm_levels(lx, 0.02, 3, pg, bias, torch.bfloat16), gemm_fused(x, sc, sh, (0, 255, 0, 255), pg, bias)
    for _ in range(19):
        assert same_bits(gemm_levels(lx, 0.02, 3, pg, bias, torch.bfloat16), first)
        assert same_bits(gemm_fused(x, sc, sh, (0, 255, 0, 255), pg, bias), first_f)


@pytest.mark.parametrize("fmt", FORMATS, **_id)
def test_a_rows_bits_do_not_depend_on_m_or_on_its_place(fmt):
    N, K, G, bits = fmt
    pg = to_dev(C.random_packed(N, K, G, bits))
    lx = A.levels((129, K), 0, 255).to(DEV)
    row = lx[5:6].clone()
    for at in (0, 16, 128):
        lx[at] = row[0]
    one = block_levels(row, 0.02, 3, pg, None, torch.float32)                   # the 1-row decode call
    y129, y17 = gemm_levels(lx, 0.02, 3, pg, None, torch.float32), gemm_levels(lx[:17], 0.02, 3, pg, None, torch.float32)
    for at in (0, 16, 128):
        assert same_bits(y129[at:at + 1], one), at
    assert same_bits(y17[0:1], one) and same_bits(y17[16:17], one) and same_bits(y17, y129[:17])
    assert same_bits(gemm_levels(row, 0.02, 3, pg, None, torch.float32), one)  # M = 1 is served too


def test_views_of_x_and_of_the_codes(monkeypatch):
    """a non-contiguous x and a [3, 43, K] x through the ops, on the GEMM's route; codes at byte offset 1 are refused by the
    library and served by the ops all the same"""
    monkeypatch.setattr(_qgemm_a8_host, "QGEMM_A8_MIN_ROWS", 17)
    N, K, G, bits = 21, 256, 32, 4
    pe = C.exact_packed(N, K, G, bits, seed=5)
    peg = to_dev(pe)
    lx = A.levels((3, 43, K), 0, 255)
    r, _ = A.reference(lx, A.S_X_EXACT, 7, pe)
    s, z = A.act(A.S_X_EXACT, 7, DEV)

    def q8(l, p):
        return torch.ops.torchlsq.lsq_linear_packed_q8(l, s, z, p.codes, p.scale.reshape(-1), p.zero_point.reshape(-1), None, G, bits,
                                                       torch.float32)

    y = q8(lx.to(DEV), peg)
    assert y.shape == (3, 43, N)
    C.assert_exact(y, r, torch.float32, "x [3, 43, K]")
    assert same_bits(y.reshape(129, N), gemm_levels(lx.reshape(129, K).to(DEV), A.S_X_EXACT, 7, peg, None, torch.float32))
    wide = torch.zeros(3, 43, 2 * K, dtype=torch.uint8, device=DEV)
    wide[..., ::2] = lx.to(DEV)
    assert not wide[..., ::2].is_contiguous()
    C.assert_exact(q8(wide[..., ::2], peg), r, torch.float32, "non-contiguous levels")
    xs = C.exact_x((40, 2 * K), torch.bfloat16).to(DEV)
    sc, sh = torch.tensor([1.0], device=DEV), torch.tensor([-8.0], device=DEV)         # zero point 8: levels x + 8 in 0..16
    yv = lsq_linear_packed_a8(xs[:, ::2], peg, None, sc, sh, 0, 255)
    assert same_bits(yv, gemm_fused(xs[:, ::2].contiguous(), sc, sh, (0, 255, 0, 255), peg, None))
    assert same_bits(yv, block_fused(xs[:, ::2], sc, sh, (0, 255, 0, 255), peg, None))
    # levels at a byte offset that is no multiple of 16: the library reads them all the same
    buf = torch.zeros(129 * K + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = lx.reshape(-1).to(DEV)
    assert buf[1:].data_ptr() % 16 != 0
    C.assert_exact(gemm_levels(buf[1:].view(129, K), A.S_X_EXACT, 7, peg, None, torch.float32), r.reshape(129, N), torch.float32,
                   "levels at byte offset 1")
    buf = torch.zeros(pe.codes.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = pe.codes.reshape(-1).to(DEV)
    qv = PackedGroupTensor(buf[1:].view(N, -1), pe.scale.to(DEV), pe.zero_point.to(DEV), bits, G, pe.quant_min, pe.shape)
    assert qv.codes.data_ptr() % 16 != 0 and qv.codes.is_contiguous()
    with pytest.raises(RuntimeError, match=r"\(-1\).*not served.*16-byte aligned"):
        gemm_levels(lx.reshape(129, K).to(DEV), A.S_X_EXACT, 7, qv, None, torch.float32)
    torch.cuda.synchronize()
    C.assert_exact(q8(lx.to(DEV), qv), r, torch.float32, "codes at byte offset 1")


class Spy:
    def __init__(self, monkeypatch):
        self.calls = []
        for mod, name in ((_qlinear_a8_host, "qgemm_a8_forward_levels"), (_qlinear_a8_host, "qgemm_a8_forward"),
                          (_qlinear_a8_host, "_launch_row_blocks")):
            monkeypatch.setattr(mod, name, self._wrap(name, getattr(mod, name)))

    def _wrap(self, name, fn):
        def inner(*args, **kw):
            self.calls.append(name)
            return fn(*args, **kw)
        return inner


def test_the_ops_take_the_gemm_from_the_threshold_on(monkeypatch):
    N, K, G, bits = 67, 384, 128, 4
    rows = E.qgemm_a8_min_rows()
    pg = to_dev(C.random_packed(N, K, G, bits))
    lx = A.levels((rows, K), 0, 255).to(DEV)
    x = C.random_x((rows, K), torch.float16).to(DEV)
    sc, sh = torch.tensor([0.02], device=DEV), torch.tensor([-2.5], device=DEV)
    s, z = A.act(0.02, 3, DEV)
    bias = C.random_bias(N, torch.float32).to(DEV)
    spy = Spy(monkeypatch)

    def q8(l):
        return torch.ops.torchlsq.lsq_linear_packed_q8(l, s, z, pg.codes, pg.scale.reshape(-1), pg.zero_point.reshape(-1), bias, G, bits,
                                                       torch.bfloat16)

    y = q8(lx)
    assert spy.calls == ["qgemm_a8_forward_levels"] and same_bits(y, gemm_levels(lx, 0.02, 3, pg, bias, torch.bfloat16))
    del spy.calls[:]
    y = lsq_linear_packed_a8(x, pg, bias, sc, sh, 0, 255)
    assert spy.calls == ["qgemm_a8_forward"] and same_bits(y, gemm_fused(x, sc, sh, (0, 255, 0, 255), pg, bias))
    del spy.calls[:]
    y = q8(lx[:rows - 1])
    assert spy.calls == ["_launch_row_blocks"] and same_bits(y, gemm_levels(lx[:rows - 1], 0.02, 3, pg, bias, torch.bfloat16))
    del spy.calls[:]
    y = lsq_linear_packed_a8(x[:rows - 1], pg, bias, sc, sh, 0, 255)
    assert spy.calls == ["_launch_row_blocks"] and same_bits(y, gemm_fused(x[:rows - 1], sc, sh, (0, 255, 0, 255), pg, bias))
    # a format the library does not serve stays on the block route, whatever M is
    del spy.calls[:]
    pgen = to_dev(C.random_packed(9, 24, 8, 4))
    yg = torch.ops.torchlsq.lsq_linear_packed_q8(A.levels((rows, 24), 0, 255).to(DEV), s, z, pgen.codes, pgen.scale.reshape(-1),
                                                 pgen.zero_point.reshape(-1), None, 8, 4, torch.float32)
    assert spy.calls == ["_launch_row_blocks"] and yg.shape == (rows, 9)


def test_a_captured_graph_replays_to_the_eager_result(monkeypatch):
    monkeypatch.setattr(_qgemm_a8_host, "QGEMM_A8_MIN_ROWS", 17)
    N, K, G, bits = 67, 384, 128, 4
    pg = to_dev(C.random_packed(N, K, G, bits))
    sc, sh = torch.tensor([0.02], device=DEV), torch.tensor([-2.5], device=DEV)
    bias = C.random_bias(N, torch.float32).to(DEV)
    args = (sc, sh, pg.codes, pg.scale.reshape(-1), pg.zero_point.reshape(-1), bias)

    def f(x, sc, sh, codes, scale, zp, b):
        return torch.ops.torchlsq.lsq_linear_packed_a8(x, sc, sh, 0, 255, 0, 255, codes, scale, zp, b, G, bits)

    static_x = C.random_x((3, 43, K), torch.bfloat16).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f(static_x, *args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = f(static_x, *args)
    x2 = C.random_x((3, 43, K), torch.bfloat16, seed=9).to(DEV)
    static_x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    want = f(x2, *args)
    assert same_bits(static_y, want)
    assert same_bits(want.reshape(129, N), gemm_fused(x2.reshape(129, K), sc, sh, (0, 255, 0, 255), pg, bias))


def test_packed_linear_a8_module_on_a_129_row_batch():
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
    x = C.random_x((129, 384), torch.float16)
    xq = q.quantize(x.float())
    lv = torch.ops.torchlsq.lsq_levels_per_tensor(x.to(DEV), m.input_scale, m.input_shift, 0, 127, 0, 255, 0).view(torch.uint8)
    r, Eb = A.reference(lv, xq.q_scale(), xq.q_zero_point(), p, bias)
    y = m(x.to(DEV))
    C.assert_within_bound(y, r, Eb, torch.float16, "PackedLinearA8, 129 rows")
    assert same_bits(y, torch.cat([m(x[m0:m0 + BLOCK].to(DEV)) for m0 in range(0, 129, BLOCK)]))
