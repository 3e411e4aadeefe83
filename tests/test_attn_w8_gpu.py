"""The attention core on 8-bit levels on the GPU (liblsq_hip_attn_w8.so): bit for bit against the CPU path of the same ops
(tests/test_attn_w8_cpu.py holds that path to plain integers, to the W8A8 linear, to numpy and to float64), in every kernel family
and form, on both sides of every threshold of the plans, on strided operands and outputs with guard bytes.  No tolerance anywhere;
the softmax tables are built once on the CPU and moved.
"""
import pytest
import torch

import attn_w8_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
GUARD = 0x5A


def _same(got, want, note=""):
    assert got.shape == want.shape and got.dtype == want.dtype, note
    assert torch.equal(A.bits(got.cpu()), A.bits(want)), note


def _strides(t):
    from torchlsq._attn_w8_host import _strides4
    s = _strides4(t)
    return (s.s0, s.s1, s.ld)


def _bmm_everything(ops, family, note, shift=()):
    """floats out in three dtypes and levels out in both level dtypes against the CPU path; the plan's family first"""
    from torchlsq import extension as E
    a, b, nt = ops[0], ops[3], ops[6]
    lead = tuple(a.shape[:-2])
    B = (1,) * (2 - len(lead)) + lead
    pl = E.attn_w8_plan_bmm(B, a.shape[-2], b.shape[-2] if nt else b.shape[-1], a.shape[-1], nt, a_strides=_strides(a), b_strides=_strides(b),
                            aligned=not shift, a_dtype=a.dtype, b_dtype=b.dtype)
    assert pl["family"] == family and pl["form"] == ("nt" if nt else "nn"), (note, pl)
    want = A.run_bmm("cpu", ops, None, F32)
    _same(A.run_bmm(DEV, ops, None, F32, shift), want, note)
    for mid in (BF16, F16):
        _same(A.run_bmm(DEV, ops, None, mid, shift), A.run_bmm("cpu", ops, None, mid), (note, mid))
    for unsigned, mid in ((True, BF16), (False, F32)):
        q = A.fit_quantizer(want, unsigned)
        w = A.run_bmm("cpu", ops, q, mid)
        assert want.numel() < 8 or len(w.unique()) > min(8, want.numel() // 2), note
        _same(A.run_bmm(DEV, ops, q, mid, shift), w, (note, unsigned))


PAIRS = ((U8, I8), (I8, U8), (U8, U8), (I8, I8))


@pytest.mark.parametrize("case", [(1, 1, 1, 16), (2, 17, 18, 64), (1, 16, 16, 272), (1, 33, 70, 80), (1, 65, 64, 16), (1, 64, 65, 32),
                                  (3, 130, 129, 48), ((2, 2), 19, 19, 32)], ids=str)
def test_bmm_nt_on_the_matrix_cores(case):
    B, M, N, K = case
    for i, (ad, bd) in enumerate(PAIRS[:2] if M > 100 else PAIRS):
        _bmm_everything(A.bmm_operands(B, M, N, K, True, i, ad, bd), "mfma", (case, ad, bd))


def test_bmm_nt_masked_tail_and_generic():
    # rows of 197 bytes 208 apart: the matrix cores, the last packet's 11 bytes of padding (0xFF) masked in registers
    _bmm_everything(A.bmm_operands(2, 5, 7, 197, True, 0, U8, I8, a_ld=208, b_ld=208), "mfma", "padded")
    _bmm_everything(A.bmm_operands(2, 5, 7, 197, True, 1, I8, U8, a_ld=208, b_ld=208, za=3, zb=140), "mfma", "padded, far zero points")
    # the same rows dense, and a base one byte off: the generic kernel
    _bmm_everything(A.bmm_operands(2, 5, 7, 197, True, 0, U8, I8), "generic", "dense")
    _bmm_everything(A.bmm_operands(2, 17, 18, 64, True, 2, U8, I8), "generic", "a one byte off", shift=(0,))
    _bmm_everything(A.bmm_operands(2, 17, 18, 64, True, 2, U8, I8), "generic", "b one byte off", shift=(3,))


def test_bmm_sums_beyond_32_bits():
    a = torch.full((1, 1, 65536), 255, dtype=U8)
    b = torch.stack([torch.full((65536,), 127, dtype=I8), torch.full((65536,), -128, dtype=I8)]).unsqueeze(0)
    for shift, family in (((), "mfma"), ((0,), "generic")):
        ops = (a, A.one(A.S_A), A.one(0, torch.int32), b, A.one(A.S_B), A.one(-128, torch.int32), True)
        want = A.run_bmm("cpu", ops, None, F32)
        assert want[0, 0, 0].item() > 2.0 ** 31 * A.S_A * A.S_B and want[0, 0, 1].item() == 0.0
        _same(A.run_bmm(DEV, ops, None, F32, shift), want, family)
    ops = A.bmm_operands(1, 1, 2, 65536, True, 9, I8, I8, za=5, zb=128)
    _bmm_everything(ops, "mfma", "K = 65536, random")


@pytest.mark.parametrize("case", [(1, 5, 16, 16), (1, 33, 80, 70), (1, 65, 64, 16), (1, 64, 128, 65), (3, 130, 144, 100), ((2, 2), 19, 32, 19)], ids=str)
def test_bmm_nn_on_the_matrix_cores(case):
    B, M, N, K = case
    ld = (K + 15) // 16 * 16
    for i, (ad, bd) in enumerate(PAIRS[:2] if M > 100 else PAIRS):
        _bmm_everything(A.bmm_operands(B, M, N, K, False, i, ad, bd, a_ld=ld if ld != K else None), "mfma", (case, ad, bd))


def test_bmm_nn_ragged_columns_and_generic():
    _bmm_everything(A.bmm_operands(2, 17, 64, 197, False, 0, U8, I8, a_ld=208), "mfma", "probabilities 208 apart")
    # N = 72 and N = 8: B's rows padded to a multiple of 16 run on the matrix cores, dense they do not
    for N, ld in ((72, 80), (8, 16)):
        _bmm_everything(A.bmm_operands(2, 17, N, 48, False, N, U8, U8, b_ld=ld), "mfma", (N, "padded"))
        _bmm_everything(A.bmm_operands(2, 17, N, 48, False, N, U8, U8), "generic", (N, "dense"))
    _bmm_everything(A.bmm_operands(2, 17, 64, 48, False, 3, I8, U8), "generic", "b one byte off", shift=(3,))
    _bmm_everything(A.bmm_operands(2, 5, 7, 197, False, 4, I8, I8), "generic", "dense rows of 197")


def test_bmm_strided_operands_and_guard_bytes():
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, lsq_bmm_w8, lsq_bmm_w8_q
    qkv = A.levels((2, 19, 3, 3, 32), 7, U8)
    q, k, v = A.qkv_heads(qkv)
    gq, gk, gv = A.qkv_heads(qkv, DEV)
    assert gq.levels.stride() == (19 * 288, 32, 288, 1) and gk.levels.data_ptr() == gq.levels.data_ptr() + 96
    assert E.attn_w8_plan_bmm((2, 3), 19, 19, 32, True, a_strides=(19 * 288, 32, 288), b_strides=(19 * 288, 32, 288))["family"] == "mfma"
    s = lsq_bmm_w8(q, k, True)
    gs = lsq_bmm_w8(gq, gk, True)
    _same(gs, s, "scores of the views")
    sq = A.fit_quantizer(s, True)
    p = lsq_bmm_w8_q(q, k, True, *sq, mid_dtype=BF16)
    gp = lsq_bmm_w8_q(gq, gk, True, *A.to(DEV, sq), mid_dtype=BF16)
    _same(gp.levels, p.levels, "score levels")
    # a batch's result equals the single-batch call; launches repeat bit for bit
    one_b = lsq_bmm_w8_q(LevelsTensor(gq.levels[1, 2], gq.scale, gq.zero_point, 0, 255), LevelsTensor(gk.levels[1, 2], gk.scale, gk.zero_point, 0, 255),
                         True, *A.to(DEV, sq), mid_dtype=BF16)
    assert torch.equal(one_b.levels, gp.levels[1, 2]) and torch.equal(lsq_bmm_w8(gq, gk, True), gs)
    # the context through the [B, H, T, D] view of a [B, T, H D] buffer, rows 112 apart: guard bytes between the rows and around
    cq = A.fit_quantizer(lsq_bmm_w8(p, v), False)
    want = lsq_bmm_w8_q(p, v, False, *cq, mid_dtype=F16).levels
    pp = LevelsTensor(A.place(A.padded(p.levels, 32), DEV), gp.scale, gp.zero_point, 0, 255)
    for off, store in ((0, "packets"), (3, "elements")):
        buf = torch.full((2 * 19 * 112 + 32,), GUARD, dtype=I8, device=DEV)
        body = buf[16:16 + 2 * 19 * 112].view(2, 19, 112)
        out = body[..., off:off + 96].view(2, 19, 3, 32).permute(0, 2, 1, 3)
        assert E.attn_w8_plan_bmm((2, 3), 19, 32, 19, False, a_strides=(3 * 19 * 32, 19 * 32, 32), b_strides=(19 * 288, 32, 288),
                                  y_strides=(19 * 112, 32, 112), y_aligned=off == 0)["store"] == store
        got = lsq_bmm_w8_q(pp, gv, False, *A.to(DEV, cq), mid_dtype=F16, out=out)
        assert got.levels.data_ptr() == out.data_ptr()
        _same(out, want, store)
        mask = torch.ones_like(body, dtype=torch.bool)
        mask[..., off:off + 96] = False
        assert bool((body[mask] == GUARD).all()) and bool((buf[:16] == GUARD).all()) and bool((buf[-16:] == GUARD).all()), store
    # floats through a strided `out`: nothing but the logical y is written
    fbuf = torch.full((2, 3, 19, 40), 7.0, dtype=BF16, device=DEV)
    E.attn_w8_bmm(pp.levels, pp.scale, pp.zero_point, gv.levels, gv.scale, gv.zero_point, False, BF16, out=fbuf[..., 4:36])
    _same(fbuf[..., 4:36], lsq_bmm_w8(p, v, False, BF16), "floats, strided")
    assert bool((fbuf[..., :4] == 7.0).all()) and bool((fbuf[..., 36:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------
# softmax
# ---------------------------------------------------------------------------------------------------
def _softmax_everything(x, tab, family, note, shift=(), lanes=None):
    from torchlsq import extension as E
    R, C = x.shape
    pl = E.attn_w8_plan_softmax(R, C, x.stride(0) if R > 1 else C, C, aligned=not shift, x_dtype=x.dtype)
    if family == "packets":             # the op's own y is dense: the packets family needs C % 16 == 0 there, else row_pad
        pl = E.attn_w8_plan_softmax(R, C, x.stride(0) if R > 1 else (C + 15) // 16 * 16, (C + 15) // 16 * 16, x_dtype=x.dtype)
    assert pl["family"] == family and (lanes is None or (pl["lanes_per_row"], pl["packets_per_lane"]) == lanes), (note, pl)
    pad = 16 if family == "packets" else 1
    for mid in A.MIDS:
        _same(A.run_softmax(DEV, x, tab, None, mid, shift=shift), A.run_softmax("cpu", x, tab, None, mid), (note, mid))
    for q, mid in ((A.PROB_Q, BF16), ((A.one(1.0 / 255), A.one(128.0 / 255), -128, 127, -128, 127), F32)):
        want = A.run_softmax("cpu", x, tab, q, mid)
        got = A.run_softmax(DEV, x, tab, q, mid, pad, shift)
        assert pad == 1 or C % 16 == 0 or got.stride(0) == (C + 15) // 16 * 16
        _same(got, want, (note, mid))


@pytest.mark.parametrize("C,lanes", [(16, (4, 1)), (64, (4, 1)), (65, (8, 1)), (197, (16, 1)), (257, (32, 1)), (1024, (64, 1)), (1025, (64, 2)),
                                     (2049, (64, 4)), (4100, (64, 8)), (8192, (64, 8))], ids=str)
def test_softmax_packets_family(C, lanes):
    ld = (C + 15) // 16 * 16
    for dtype, tab in ((U8, A.table()), (I8, A.table(0.02, 1.0))):
        x = A.score_rows(5 if C > 300 else 37, C, C, dtype)
        _softmax_everything(A.padded(x, ld, GUARD) if ld != C else x, tab, "packets", (C, dtype), lanes=lanes)


def test_softmax_generic_family_and_edges():
    tab = A.table()
    _softmax_everything(torch.tensor([[200]], dtype=U8), tab, "generic", "one element")
    _softmax_everything(A.score_rows(3, 16, 0, I8), tab, "packets", "(3, 16)", lanes=(4, 1))
    _softmax_everything(A.score_rows(5, 197, 1, U8), tab, "generic", "dense rows of 197")
    _softmax_everything(A.score_rows(2, 8208, 2, I8), A.table(0.004, 1.0), "generic", "beyond 8192")
    _softmax_everything(A.score_rows(5, 208, 3, U8), tab, "generic", "x one byte off", shift=(0,))
    # a table with zeros: one maximum, the rest 255 below it; and rows of the bulk
    tz = A.table_with_zeros()
    x = torch.zeros(4, 64, dtype=U8)
    x[0, 5] = x[1, 63] = x[2, 0] = 255
    for t in (x, A.score_rows(6, 197, 4, U8)):
        _softmax_everything(t if t.shape[1] == 64 else A.padded(t, 208), tz, "packets", "zeros in the table")
        _softmax_everything(t[:, :61].contiguous(), tz, "generic", "zeros in the table, generic")
    # S beyond 2^32: every entry 2^24, C = 65536 (generic) and 8192 (packets, 128 entries a lane: 2^31 in the 32-bit partial sum)
    full = A.full_table()
    for C, family in ((65536, "generic"), (8192, "packets")):
        x = A.levels((1, C), 5, U8)
        want = A.run_softmax("cpu", x, full, None, F32)
        assert bool((want == 1.0 / C).all())
        _same(A.run_softmax(DEV, x, full, None, F32), want, family)
        _softmax_everything(A.levels((2, C), 6, I8), full, family, ("all 2^24", C))


def test_softmax_padded_rows_guard_bytes_rows_and_repeats():
    from torchlsq import extension as E
    tab = A.table().to(DEV)
    x = A.score_rows(5, 197, 7, U8)
    want = A.run_softmax("cpu", x, A.table(), A.PROB_Q, BF16)
    gx = A.place(A.padded(x, 208, 0xFF), DEV)
    q = A.to(DEV, A.PROB_Q)
    assert E.attn_w8_plan_softmax(5, 197, 208, 208)["family"] == "packets"
    buf = torch.full((5 * 208 + 32,), GUARD, dtype=U8, device=DEV)
    body = buf[16:16 + 5 * 208].view(5, 208)
    E.attn_w8_softmax_q(gx, tab, *q, BF16, 1, out=body[:, :197])
    _same(body[:, :197], want, "ldx = ldy = 208")
    assert bool((body[:, 197:] == GUARD).all()) and bool((buf[:16] == GUARD).all()) and bool((buf[-16:] == GUARD).all())
    # the generic kernel into the same rows, one byte off
    buf.fill_(GUARD)
    E.attn_w8_softmax_q(gx, tab, *q, BF16, 1, out=body[:, 1:198])
    _same(body[:, 1:198], want, "y one byte off")
    assert bool((body[:, 198:] == GUARD).all()) and bool((body[:, 0] == GUARD).all()) and bool((buf[:16] == GUARD).all())
    # rows equal the single-row calls; launches repeat bit for bit
    again = E.attn_w8_softmax_q(gx, tab, *q, BF16, 16)
    assert again.stride(0) == 208 and torch.equal(again, body[:, 1:198])
    for r in range(5):
        assert torch.equal(E.attn_w8_softmax_q(gx[r:r + 1], tab, *q, BF16, 16), again[r:r + 1]), r
    fl = E.attn_w8_softmax(gx, tab, F32)
    assert torch.equal(fl, E.attn_w8_softmax(gx, tab, F32))
    _same(fl, A.run_softmax("cpu", x, A.table(), None, F32), "floats from padded rows")


@pytest.mark.parametrize("C,G", [(16, 64), (1024, 4)], ids=str)
def test_softmax_rows_per_workgroup_threshold(C, G):
    """(256 / L) groups of 4 rows from 512 workgroups on, of one row below"""
    from torchlsq import extension as E
    edge = 511 * G * 4 + 1
    tab = A.table()
    x = A.score_rows(edge, C, 11, U8)
    want = A.run_softmax("cpu", x, tab, A.PROB_Q, BF16)
    for R in (edge, edge - 1):
        assert E.attn_w8_plan_softmax(R, C)["rows_per_workgroup"] == (4 * G if R == edge else G)
        _same(A.run_softmax(DEV, x[:R], tab, A.PROB_Q, BF16), want[:R], R)


# ---------------------------------------------------------------------------------------------------
# the core
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 19, 32), (1, 2, 197, 64)], ids=str)
def test_attention_core_equals_the_cpu_core_and_replays_in_a_graph(shape):
    import copy
    core, qkv, want = A.core_case(*shape)
    qkv2 = A.levels(qkv.shape, 99, U8)
    want2 = core(*A.qkv_heads(qkv2)).levels
    assert not torch.equal(want.levels, want2) and len(want.levels.unique()) > 32
    gpu = copy.deepcopy(core).to(DEV)
    assert torch.equal(gpu.softmax.table.cpu(), core.softmax.table)
    static = qkv.to(DEV)
    heads = A.qkv_heads(static, DEV)
    assert heads[0].levels.data_ptr() == static.data_ptr()
    eager = gpu(*heads)
    _same(eager.levels, want.levels, "eager")
    assert torch.equal(eager.scale.cpu(), want.scale) and torch.equal(eager.zero_point.cpu(), want.zero_point)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gpu(*heads)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gpu(*heads).levels
    graph.replay()
    assert torch.equal(out.cpu(), want.levels)
    static.copy_(qkv2)
    graph.replay()
    assert torch.equal(out.cpu(), want2)


def test_device_built_table_differs_by_at_most_one():
    from torchlsq.functional import lsq_softmax_table
    for s_x, alpha, _ in A.TRIALS:
        got = lsq_softmax_table(A.one(s_x).to(DEV), alpha)
        assert got.device.type == "cuda" and got.dtype == torch.int32 and int(got[0]) == 1 << 24
        assert int((got.cpu().long() - A.table(s_x, alpha).long()).abs().max()) <= 1


def test_bmm_rows_that_overlap_and_far_zero_points():
    """an expanded row and a sliding-window view are copied, not read with an invented row stride; zero points of 16 bits take the
    64-bit form of the sum in both families"""
    base = A.levels((40,), 21, U8)
    other = A.levels((7, 32), 22, I8)
    s, za, zb = A.one(A.S_A), A.one(117, torch.int32), A.one(3, torch.int32)
    gbase, gother = base.to(DEV), other.to(DEV)
    views = lambda t: (t[:32].unsqueeze(0).expand(5, 32), t.as_strided((5, 32), (2, 1)))
    for v, gv in zip(views(base), views(gbase)):
        assert gv.stride() == v.stride() and gv.untyped_storage().nbytes() < 5 * 32
        for mid in A.MIDS:
            want = torch.ops.torchlsq.lsq_bmm_w8_q8(v, s, za, other, s, zb, True, mid)
            _same(torch.ops.torchlsq.lsq_bmm_w8_q8(gv, s.to(DEV), za.to(DEV), gother, s.to(DEV), zb.to(DEV), True, mid), want, v.stride())
        want = torch.ops.torchlsq.lsq_bmm_w8_q8(other, s, zb, v, s, za, True, F32)
        _same(torch.ops.torchlsq.lsq_bmm_w8_q8(gother, s.to(DEV), zb.to(DEV), gv, s.to(DEV), za.to(DEV), True, F32), want, "as B")
    for za_, zb_ in ((32767, -32768), (-30000, -30000), (3, 32767)):
        for K, shift, family in ((64, (), "mfma"), (7, (), "generic"), (64, (0,), "generic")):
            ops = (A.levels((2, 17, K), 31, U8), A.one(A.S_A), A.one(za_, torch.int32), A.levels((2, 18, K), 32, I8), A.one(A.S_B),
                   A.one(zb_, torch.int32), True)
            _same(A.run_bmm(DEV, ops, None, F32, shift), A.run_bmm("cpu", ops, None, F32), (za_, zb_, family))
