"""The masked softmax on 8-bit levels on the GPU (liblsq_hip_attn_mask_w8.so): bit for bit against the CPU path -- the definition,
which tests/test_attn_mask_w8_cpu.py holds to the existing unmasked op -- for the same CPU-built table: every packets
instantiation at every prefix length that changes what a lane does, the generic family, guard bytes and poisoned bytes beyond the
prefix, both sides of the rows-per-workgroup threshold, graph capture with lengths rewritten on the device, and repeats.
"""
import pytest
import torch

import attn_mask_w8_cases as M
import attn_w8_cases as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
GUARD = 0xA5
SIDES = ((A.PROB_Q, BF16), (None, F32), (None, BF16))


def _floats_through_packets(x, tab, mid, offset, lengths, lanes):
    """floats out THROUGH THE PACKETS FAMILY: the op alone would allocate a dense y, whose row stride C sends every C % 16 != 0 to the
    generic kernel, so y is the [.., :C] view of a float buffer whose rows lie a multiple of 16 elements apart (its base 16-byte
    aligned); the plan for exactly these strides is asserted, and the padding of every row must come back untouched"""
    from torchlsq import extension as E
    C, Tq = int(x.shape[-1]), int(x.shape[-2])
    R, ld = x.numel() // C, (C + 15) // 16 * 16
    assert x.stride(-2) % 16 == 0
    pl = E.attn_mask_w8_plan_softmax(R, C, Tq, x.stride(-2), ld, x_dtype=x.dtype, causal=offset is not None, causal_offset=offset or 0,
                                     rows_per_length=None if lengths is None else R // int(x.shape[0]))
    assert pl["family"] == "packets" and (pl["lanes_per_row"], pl["packets_per_lane"]) == lanes, pl
    gx, = A.to(DEV, (x,))
    buf = torch.full(tuple(x.shape[:-1]) + (ld,), -7.0, dtype=mid, device=DEV)
    assert buf.data_ptr() % 16 == 0 and gx.data_ptr() % 16 == 0
    got = E.attn_mask_w8_softmax(gx, tab.to(DEV), mid, offset is not None, offset or 0, M.lens_tensor(lengths, DEV), out=buf[..., :C])
    assert got.data_ptr() == buf.data_ptr() and bool((buf[..., C:] == -7.0).all())
    return got


def _check(x, tab, offset, lengths, note, sides=SIDES, shift=(), pad=16, lanes=None):
    """GPU against the CPU path on every side; `lanes`: the (L, P) of the packets instantiation that every side, the floats too, must run"""
    for q, mid in sides:
        want = M.run_masked("cpu", x, tab, q, mid, offset, lengths)
        if q is None and lanes is not None:
            got = _floats_through_packets(x, tab, mid, offset, lengths, lanes)
        else:
            got = M.run_masked(DEV, x, tab, q, mid, offset, lengths, pad if q is not None else 1, shift)
        M.same(got, want, (note, offset, lengths, q is None, mid))


# ---------------------------------------------------------------------------------------------------
# 1: every packets instantiation
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,lanes", [(16, (4, 1)), (64, (4, 1)), (65, (8, 1)), (197, (16, 1)), (257, (32, 1)), (1024, (64, 1)), (1025, (64, 2)),
                                     (2049, (64, 4)), (8192, (64, 8))], ids=str)
def test_packets_family_at_every_prefix_length(C, lanes):
    from torchlsq import extension as E
    L = lanes[0]
    ld = (C + 15) // 16 * 16
    targets = sorted(set(min(v, C) for v in (0, 1, 15, 16, 17, 16 * L - 1, 16 * L, 16 * L + 1, C - 1, C)))
    Tq = min(35, C)
    for dtype, tab in ((U8, A.table()), (I8, A.table(0.02, 1.0))):
        # through key_lengths: [2, 2, 3, C], a pair of lengths a launch
        x = A.score_rows(2 * 2 * 3, C, C, dtype).view(2, 2, 3, C)
        x = A.padded(x, ld, GUARD) if ld != C else x
        pl = E.attn_mask_w8_plan_softmax(12, C, 3, ld, ld, x_dtype=dtype, rows_per_length=6)
        assert pl["family"] == "packets" and (pl["lanes_per_row"], pl["packets_per_lane"]) == lanes, pl
        pairs = list(zip(targets[0::2], targets[1::2])) + ([(targets[-1], targets[0])] if len(targets) % 2 else [])
        assert sorted(set(v for p in pairs for v in p)) == targets
        for pair in pairs:
            _check(x, tab, None, list(pair), (C, dtype, "lengths"), lanes=lanes)
        # through causal rows: [2, 2, Tq, C] with the offsets 0 and C - Tq, and those that put every target inside a matrix
        x = A.score_rows(2 * 2 * Tq, C, C + 1, dtype).view(2, 2, Tq, C)
        x = A.padded(x, ld, GUARD) if ld != C else x
        pl = E.attn_mask_w8_plan_softmax(4 * Tq, C, Tq, ld, ld, x_dtype=dtype, causal=True, causal_offset=C - Tq)
        assert pl["family"] == "packets" and (pl["lanes_per_row"], pl["packets_per_lane"]) == lanes, pl
        offsets = [0, C - Tq]
        seen = set()
        for off in offsets:
            seen.update(M.prefix_lengths(x.shape, off))
        for t in targets:
            if t >= 1 and t not in seen:
                off = max(t - 1 - Tq // 2, 0)
                offsets.append(off)
                seen.update(M.prefix_lengths(x.shape, off))
        assert set(targets) - {0} <= seen
        for off in offsets:
            _check(x, tab, off, None, (C, dtype, "causal"), lanes=lanes)
        # both together: the lengths cut the causal rows, one of them to nothing
        _check(x, tab, C - Tq, [0, C - 1], (C, dtype, "both"), lanes=lanes)


# ---------------------------------------------------------------------------------------------------
# 2: the generic family
# ---------------------------------------------------------------------------------------------------
def test_generic_family():
    from torchlsq import extension as E
    tab = A.table()
    P = E.attn_mask_w8_plan_softmax
    # beyond 8192
    assert P(8, 8193, 2, 8208, 8208)["family"] == "generic"
    x = A.padded(A.score_rows(8, 8193, 1, I8).view(2, 2, 2, 8193), 8208, GUARD)
    for off, lens in ((8191, None), (None, [8193, 4097]), (0, [0, 8192]), (None, None)):
        _check(x, A.table(0.004, 1.0), off, lens, "beyond 8192", sides=SIDES[:2])
    # ldx not a multiple of 16: dense rows of 197
    assert P(2 * 2 * 35, 197, 35)["family"] == "generic"
    x = A.score_rows(2 * 2 * 35, 197, 2, U8).view(2, 2, 35, 197)
    for off, lens in ((0, None), (162, None), (None, [196, 0]), (5, [64, 65]), (None, None)):
        _check(x, tab, off, lens, "dense rows of 197", pad=1)
    # a base one byte off
    x = A.score_rows(2 * 2 * 5, 208, 3, U8).view(2, 2, 5, 208)
    for off, lens in ((203, None), (None, [17, 208]), (0, [3, 1])):
        _check(x, tab, off, lens, "x one byte off", shift=(0,))
    # C = 1
    x = torch.tensor([200, 3, 17, 255, 0, 9], dtype=U8).view(3, 2, 1, 1)
    for off, lens in ((0, None), (None, [1, 0, -1]), (0, [0, 1, 7])):
        _check(x, tab, off, lens, "one element", pad=1)
    # a table with zeros and one whose sum leaves 32 bits
    x = A.padded(A.score_rows(2 * 2 * 3, 197, 4, U8).view(2, 2, 3, 197), 208)
    _check(x, A.table_with_zeros(), 100, [197, 150], "zeros in the table")
    _check(x[..., :61].contiguous(), A.table_with_zeros(), 30, [61, 2], "zeros in the table, generic")
    full = A.full_table()
    x = A.levels((2, 1, 1, 8192), 5, U8)
    _check(x, full, None, [8192, 8000], "all 2^24, packets", sides=SIDES[1:2])
    x = A.levels((2, 1, 1, 65536), 6, I8)
    _check(x, full, None, [65536, 40000], "all 2^24, generic", sides=SIDES[1:2])


def test_lengths_on_another_device_are_refused():
    x, tab = A.score_rows(4, 16, 0, U8).view(2, 1, 2, 16).to(DEV), A.table().to(DEV)
    with pytest.raises(RuntimeError, match="key_lengths must be on the levels' device"):
        torch.ops.torchlsq.lsq_softmax_mask_w8_q8(x, tab, F32, False, 0, torch.tensor([3, 4], dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------
# 3: guard bytes, poisoned bytes beyond the prefix
# ---------------------------------------------------------------------------------------------------
def test_guard_bytes_and_poison():
    from torchlsq import extension as E
    tab = A.table()
    shape = (2, 2, 5, 197)
    x = A.score_rows(20, 197, 7, U8).view(shape)
    off, lens = 100, [197, 120]
    n = M.prefix_lengths(shape, off, lens)
    want = M.run_masked("cpu", x, tab, A.PROB_Q, BF16, off, lens)
    want_f = M.run_masked("cpu", x, tab, None, F32, off, lens)
    q = A.to(DEV, A.PROB_Q)
    gtab, glens = tab.to(DEV), M.lens_tensor(lens, DEV)
    assert E.attn_mask_w8_plan_softmax(20, 197, 5, 208, 208, causal=True, causal_offset=off, rows_per_length=10)["family"] == "packets"
    for how in ("none", "max", "random"):
        px = x if how == "none" else M.poisoned(x, n, how)
        # the last row's final packet ends exactly at the end of the storage: 20 rows of 208 bytes, nothing behind them
        padded = A.padded(px, 208, 0xFF)
        assert padded.untyped_storage().nbytes() == 20 * 208
        gx = A.place(padded, DEV)
        buf = torch.full((20 * 208 + 32,), GUARD, dtype=U8, device=DEV)
        body = buf[16:16 + 20 * 208].view(2, 2, 5, 208)
        E.attn_mask_w8_softmax_q(gx, gtab, *q, BF16, True, off, glens, 1, out=body[..., :197])
        M.same(body[..., :197], want, ("ldx = ldy = 208", how))
        assert bool((body[..., 197:] == GUARD).all()) and bool((buf[:16] == GUARD).all()) and bool((buf[-16:] == GUARD).all())
        # the generic kernel into the same rows, one byte off
        buf.fill_(GUARD)
        E.attn_mask_w8_softmax_q(gx, gtab, *q, BF16, True, off, glens, 1, out=body[..., 1:198])
        M.same(body[..., 1:198], want, ("y one byte off", how))
        assert bool((body[..., 198:] == GUARD).all()) and bool((body[..., 0] == GUARD).all()) and bool((buf[:16] == GUARD).all())
        # floats into padded rows
        fbuf = torch.full((20 * 208 + 8,), -7.0, dtype=F32, device=DEV)
        fbody = fbuf[4:4 + 20 * 208].view(2, 2, 5, 208)
        E.attn_mask_w8_softmax(gx, gtab, F32, True, off, glens, out=fbody[..., :197])
        M.same(fbody[..., :197], want_f, ("floats", how))
        assert bool((fbody[..., 197:] == -7.0).all()) and bool((fbuf[:4] == -7.0).all()) and bool((fbuf[-4:] == -7.0).all())


# ---------------------------------------------------------------------------------------------------
# 4: both sides of the rows-per-workgroup threshold
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,G", [(16, 64), (1024, 4)], ids=str)
def test_rows_per_workgroup_threshold(C, G):
    """(256 / L) groups of 4 rows from 512 workgroups on, of one row below: rows b G K + g + k G must still find their (batch, t)"""
    from torchlsq import extension as E
    Tq = 16
    B_hi = (511 * G * 4) // Tq + 1          # the first batch count whose rows need 512 workgroups of 4 G rows
    B_lo = (511 * G * 4) // Tq
    assert B_hi * Tq >= 511 * G * 4 + 1 > B_lo * Tq
    tab = A.table()
    x = A.score_rows(B_hi * Tq, C, 11, U8).view(B_hi, Tq, C)
    lens = ((torch.arange(B_hi) * 7919) % (C + 2) - 1).to(torch.int32)          # -1 .. C, spread over the batches
    off = C - Tq
    want = M.run_masked("cpu", x, tab, A.PROB_Q, BF16, off, lens)
    for B in (B_hi, B_lo):
        pl = E.attn_mask_w8_plan_softmax(B * Tq, C, Tq, causal=True, causal_offset=off, rows_per_length=Tq)
        assert pl["rows_per_workgroup"] == (4 * G if B == B_hi else G), pl
        M.same(M.run_masked(DEV, x[:B], tab, A.PROB_Q, BF16, off, lens[:B]), want[:B], B)


# ---------------------------------------------------------------------------------------------------
# 5: graph capture: the lengths are read on the device
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tq,Tk", [(19, 19), (1, 40)], ids=str)
def test_masked_core_replays_in_a_graph_with_new_lengths(Tq, Tk):
    import copy
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import AttentionCoreW8Q
    B, H, D = 2, 3, 32
    span = 6.0 * A.QKV_S * A.QKV_S * 74 * 74 * D ** 0.5
    core = AttentionCoreW8Q(A.trained(-span, span), A.trained(0.0, 1.0), A.trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16, causal=True)
    s, z = A.one(A.QKV_S), A.one(A.QKV_Z, torch.int32)
    host = [A.levels((B, H, T, D), 80 + i, U8) for i, T in enumerate((Tq, Tk, Tk))]
    first, second = torch.tensor([Tk, 7], dtype=torch.int32), torch.tensor([3, Tk - 1], dtype=torch.int32)
    want1 = core(*(LevelsTensor(t, s, z, 0, 255) for t in host), key_lengths=first).levels
    want2 = core(*(LevelsTensor(t, s, z, 0, 255) for t in host), key_lengths=second).levels
    assert not torch.equal(want1, want2) and len(want1.unique()) > 16
    gpu = copy.deepcopy(core).to(DEV)
    assert torch.equal(gpu.softmax.table.cpu(), core.softmax.table)
    heads = [LevelsTensor(t.to(DEV), s.to(DEV), z.to(DEV), 0, 255) for t in host]
    lens = first.to(DEV)
    M.same(gpu(*heads, key_lengths=lens).levels, want1, "eager")
    fused = copy.deepcopy(gpu)
    fused.fused = True
    M.same(fused(*heads, key_lengths=lens).levels, want1, "fused=True: the same three launches")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gpu(*heads, key_lengths=lens)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gpu(*heads, key_lengths=lens).levels
    graph.replay()
    assert torch.equal(out.cpu(), want1)
    lens.copy_(second)
    graph.replay()
    assert torch.equal(out.cpu(), want2)


# ---------------------------------------------------------------------------------------------------
# 6: repeats, and a row depends on its own bytes and n alone
# ---------------------------------------------------------------------------------------------------
def test_repeats_and_rows_are_independent():
    tab = A.table()
    for C, ld in ((197, 208), (1025, 1040), (197, 197)):
        shape = (2, 2, 6, C)
        x = A.score_rows(24, C, 9, I8).view(shape)
        x = A.padded(x, ld, GUARD) if ld != C else x
        off, lens = C - 20, [C, C // 2]
        a = M.run_masked(DEV, x, tab, A.PROB_Q, BF16, off, lens, 16)
        b = M.run_masked(DEV, x, tab, A.PROB_Q, BF16, off, lens, 16)
        assert torch.equal(a, b)
        # every other row replaced: the rows that stayed give the bytes they gave
        other = A.levels(shape, 77, I8)
        keep = torch.zeros(24, dtype=torch.bool)
        keep[::2] = True
        mixed = torch.where(keep.view(2, 2, 6, 1), x, other)
        mixed = A.padded(mixed, ld, 0x11) if ld != C else mixed
        c = M.run_masked(DEV, mixed, tab, A.PROB_Q, BF16, off, lens, 16)
        assert torch.equal(c.reshape(24, C)[keep], a.reshape(24, C)[keep]) and not torch.equal(c, a)
        # a row alone, with its own n as its length, gives the same bytes
        n = M.prefix_lengths(shape, off, lens)
        rows = x.reshape(24, C) if ld == C else x.reshape(24, C)
        for r in (0, 7, 23):
            one_row = rows[r].reshape(1, 1, 1, C).contiguous()
            alone = M.run_masked(DEV, A.padded(one_row, ld) if ld != C else one_row, tab, A.PROB_Q, BF16, None, [n[r]], 16)
            assert torch.equal(alone.reshape(C), a.reshape(24, C)[r]), (C, r)
