"""The paged KV cache on 8-bit levels on the GPU (liblsq_hip_attn_paged_w8.so): bit for bit against the parent commit's code --
`attn_decode_w8_cases.definition` on the gathered keys, and the dense `KVCacheW8` route --, at the smallest shapes at which each
mechanism of the kernels can fail.  Before every comparison the plan's family and the forced split count are asserted, and beside the
op the library's C entry is called directly with a workspace the test made -- no Python host, no fallback --: status 0 and the same
bytes are the paged kernels' own, EINVAL with y's 0x5A guard bytes untouched means "composition".  Guard bytes sit behind the
workspace and around y.  Every comparison is torch.equal.
"""
import copy

import pytest
import torch

import attn_decode_w8_cases as C
import attn_paged_w8_cases as P
import attn_w8_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
GUARD, LSQ_EINVAL, Z3, SIGNED_PV = P.GUARD, P.LSQ_EINVAL, P.Z3, P.SIGNED_PV
LENGTHS = (-3, 0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 199, 200, 205)


def _equals(c, pg, splits, note="", family="paged", shift=(0, 0), q_shift=0):
    pl = P.plan_of(c, pg, splits, qkv_aligned=not (any(shift) or q_shift))
    assert pl["family"] == family, (note, pl)
    if family == "paged" and splits:
        assert pl["splits"] == splits and pl["grid"] == c.shape[0] * c.shape[2] * splits, (note, pl)
    C.check_not_degenerate(c)
    got = P.run(c, pg, DEV, splits, shift, q_shift)
    assert got.shape == c.want.shape and got.dtype == c.want.dtype, note
    assert torch.equal(got.cpu(), c.want), note
    if not q_shift:
        rc, y, _, _ = P.c_entry(c, pg, DEV, splits, shift)
        if family == "paged":
            assert rc == 0 and torch.equal(y.cpu(), c.want), (note, rc)
        else:
            assert rc == LSQ_EINVAL and bool((y.view(U8) == GUARD).all()), (note, rc)
    return pl


# (B, Hkv, G, Tq, ps, Mp, D), splits, key_lengths, causal: one page of one sub-tile; chunks that span several pages, a short batch;
# a full row tile and one key in the second page; five column sub-tiles and 2 keys in the fifth page; two query rows per head at
# D 128, causal; 1024 keys in one chunk (four rounds of launch 1), in four and in sixteen; a page larger than the chunk
BORDERS = [((1, 1, 1, 1, 16, 1, 16), 1, None, True), ((2, 2, 4, 1, 16, 13, 32), 2, (200, 37), True), ((2, 2, 4, 1, 16, 13, 32), 4, (200, 37), True),
           ((1, 1, 16, 1, 64, 2, 64), 2, (65,), True), ((1, 1, 2, 1, 32, 5, 80), 3, (130,), True), ((1, 1, 8, 2, 128, 2, 128), 4, (197,), True),
           ((1, 1, 4, 1, 256, 4, 64), 1, (1024,), True), ((1, 1, 4, 1, 256, 4, 64), 4, (1024,), True), ((1, 1, 4, 1, 256, 4, 64), 16, (1024,), True),
           ((1, 1, 4, 1, 1024, 2, 64), 8, (1500,), True)]


@pytest.mark.parametrize("shape,splits,lengths,causal", BORDERS, ids=str)
def test_page_and_chunk_borders(shape, splits, lengths, causal):
    B, Hkv, G, Tq, ps, Mp, D = shape
    Tk = ps * Mp
    for dtypes, unsigned in C.COMBOS if Tk < 1024 else ((C.ALL_U8, SIGNED_PV),):
        c = C.case(B, Hkv, G, Tq, Tk, D, 0, dtypes, unsigned, BF16, Z3, None, causal, lengths)
        pl = _equals(c, P.paged(c, ps, "perm", "hsd", seed=Mp), splits, (shape, splits))
        assert pl["reduce_grid"] == B * Hkv and pl["rows"] == G * Tq and pl["threads"] == 256 and pl["lds_bytes"] == 3840 + 160 * D
        assert pl["chunk"] % 64 == 0 and (splits - 1) * pl["chunk"] < Tk <= splits * pl["chunk"]
        assert pl["workspace_bytes"] == B * Hkv * G * Tq * Tk + 8 * B * Hkv * splits * G * Tq * D


def test_the_capacity_under_the_librarys_own_chunk():
    c = C.case(1, 1, 1, 1, 65536, 128, 7, C.ALL_U8, SIGNED_PV, BF16, Z3, None, True, (65533,))
    pg = P.paged(c, 256, "perm", extra=1)
    pl = _equals(c, pg, 0, "capacity")
    assert pl["chunk"] == 1024 and pl["splits"] == 64


@pytest.mark.parametrize("order", ["hsd", "shd"])
def test_layouts_and_tables(order):
    c = C.case(2, 2, 4, 1, 208, 32, 1, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (200, 37))
    for kind, pad in (("perm", 0), ("rev", 0), ("perm", 3), ("ident", 0)):
        pg = P.paged(c, 16, kind, order, bt_pad=pad, seed=pad)
        assert (pg.table.stride(0) == 13 + pad) and pg.k_pool.levels.is_contiguous() == (order == "hsd")
        _equals(c, pg, 4, (order, kind, pad))
    _equals(c, P.paged(c, 16, "rev", order), 0, "the library's chunk")


@pytest.mark.parametrize("ps", [16, 64])
def test_key_counts_in_one_call(ps):
    """B = 15 over 256 keys (208 at ps 16) in four chunks of 64: chunks wholly beyond nmax, n = 0, a count on both sides of every chunk
    and page border"""
    Tk = 208 if ps == 16 else 256
    c = C.case(15, 1, 2, 1, Tk, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, LENGTHS)
    zero = c.want[1, 0, 0]
    assert bool((c.want[0] == zero).all()) and bool((c.want[1] == zero).all()) and len(c.want[2:].unique()) > 16
    _equals(c, P.paged(c, ps), 4, "lengths")
    d = C.case(15, 1, 2, 2, Tk, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, LENGTHS)
    _equals(d, P.paged(d, ps, "rev"), 4, "lengths, Tq 2")
    d = C.case(15, 1, 2, 2, Tk, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, 5, LENGTHS)
    _equals(d, P.paged(d, ps, "perm", "shd"), 4, "lengths, Tq 2, offset 5")


def _poisoned(c, ps, fill):
    """the case's pools with every slot at or beyond the batch entry's key count filled with `fill`, the table's entries at logical
    pages beyond the live count naming a VALID page that holds `fill` alone"""
    B, H, Hkv, Tq, Tk, D = c.shape
    n = C.key_counts(B, Tq, Tk, c.causal, c.lengths.tolist())
    k, v = C.poisoned(c, fill)
    d = C.Case()
    d.shape, d.G, d.mid, d.causal, d.lengths, d.table, d.sides, d.q, d.k, d.v = c.shape, c.G, c.mid, c.causal, c.lengths, c.table, c.sides, c.q, k, v
    pg = P.paged(d, ps, "perm", extra=2, fill=fill)
    poison_page = [p for p in range(pg.Np) if p not in set(pg.table.reshape(-1).tolist())][0]
    for b in range(B):
        live = -(-max(n[b]) // ps)
        pg.table[b, live:] = poison_page
    return pg


def test_poisoned_slots_and_dead_entries_do_not_reach_the_result():
    c = C.case(15, 1, 2, 1, 208, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, LENGTHS)
    for fill in (0x00, 0xFF):
        pg = _poisoned(c, 16, fill)
        assert int((pg.table == pg.table[0, 0]).sum()) > 20
        _equals(c, pg, 4, fill)
    # the probabilities quantizer with quant_min = 5: its level of 0.0 is not its z_p, and still nothing beyond n is read
    d = C.Case()
    d.shape, d.G, d.mid, d.causal, d.lengths, d.table = c.shape, c.G, c.mid, c.causal, c.lengths, c.table
    d.q, d.k, d.v = c.q, c.k, c.v
    p = c.sides[1]
    d.sides = (c.sides[0], (p[0], p[1], 5) + tuple(p[3:]), c.sides[2])
    C.finish(d)
    assert not torch.equal(d.want, c.want)
    for fill in (0x00, 0xFF):
        _equals(d, _poisoned(d, 16, fill), 4, ("quant_min 5", fill))


def test_the_clamp_stays_inside_memory_the_test_owns():
    """the pools are the views big[1 : 1 + Np] of allocations with a poison page at each end; a live entry is -1 in one call and Np in
    another: the definition on the clamped table.  No entry could leave the allocation whatever a kernel did with it"""
    from torchlsq.functional import LevelsTensor
    c = C.case(2, 2, 4, 1, 208, 32, 3, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (200, 37))
    pg = P.paged(c, 16, "perm")
    Np = pg.Np

    def framed(pool):
        big = torch.full((Np + 2,) + tuple(pool.shape[1:]), 0xEE, dtype=U8, device=DEV).view(pool.levels.dtype)
        big[1:1 + Np] = pool.levels.to(DEV)
        return big, LevelsTensor(big[1:1 + Np], pool.scale.to(DEV), pool.zero_point.to(DEV), pool.quant_min, pool.quant_max)
    (bk, kp), (bv, vp) = framed(pg.k_pool), framed(pg.v_pool)
    assert kp.levels.data_ptr() % 16 == 0 and P.plan_of(c, pg, 4)["family"] == "paged"
    for where, bad, to in (((0, 5), -1, 0), ((0, 5), Np, Np - 1), ((1, 2), -1, 0), ((1, 0), Np, Np - 1)):
        t, want_t = pg.table.clone(), pg.table.clone()
        t[where], want_t[where] = bad, to
        k, v = P.gathered(pg, want_t)
        want = C.definition(c, k=k, v=v)
        assert not torch.equal(want, c.want)
        rc, y, _, _ = P.c_entry(c, pg, DEV, 4, operands=(kp, vp, t.to(DEV)))
        assert rc == 0 and torch.equal(y.cpu(), want), (where, bad)
        assert torch.equal(P.run(c, pg, DEV, 4, operands=(kp, vp, t.to(DEV))).cpu(), want)
    for big in (bk, bv):
        assert bool((big[0].view(U8) == 0xEE).all()) and bool((big[-1].view(U8) == 0xEE).all())


def test_the_result_does_not_depend_on_the_workspace():
    c = C.case(2, 2, 4, 1, 208, 32, 4, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (200, 70))
    pg = P.paged(c, 16)
    for fill in (0x00, 0xFF):
        rc, y, ws, need = P.c_entry(c, pg, DEV, 4, fill=fill)
        assert rc == 0 and torch.equal(y.cpu(), c.want), fill
        assert need == 2 * 2 * 4 * 208 + 8 * 2 * 2 * 4 * 4 * 32
    # a long call fills the workspace, shorter ones (n = 0 among them) run in the same bytes
    long = C.case(1, 1, 16, 1, 1024, 64, 4, C.ALL_U8, SIGNED_PV)
    rc, y, ws, need = P.c_entry(long, P.paged(long, 64), DEV, 16)
    assert rc == 0 and torch.equal(y.cpu(), long.want)
    for shape, ps, splits, lengths in (((1, 1, 3, 1, 208, 64), 16, 4, (100,)), ((1, 1, 16, 1, 192, 64), 64, 3, (0,)), ((1, 1, 1, 1, 128, 64), 32, 2, (64,)),
                                       ((1, 1, 16, 1, 1024, 64), 128, 4, (3,))):
        d = C.case(*shape, 4, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, lengths)
        dp = P.paged(d, ps)
        assert P.plan_of(d, dp, splits)["workspace_bytes"] <= need
        rc, y, _, _ = P.c_entry(d, dp, DEV, splits, ws=ws)
        assert rc == 0 and torch.equal(y.cpu(), d.want), shape
    assert bool((ws[need:] == GUARD).all())


@pytest.mark.parametrize("mid", A.MIDS, ids=str)
def test_dtypes(mid):
    for dtypes, unsigned in C.COMBOS + (((U8, U8, I8), (False, False, True)),):
        c = C.case(2, 2, 4, 1, 208, 32, 5, dtypes, unsigned, mid, Z3, None, True, (200, 131))
        _equals(c, P.paged(c, 16, "perm", "shd"), 4, (dtypes, unsigned, mid))


def test_zero_points_far_from_the_middle():
    for dtypes in (C.ALL_U8, (I8, I8, I8), (U8, I8, U8)):
        c = C.case(2, 2, 4, 1, 208, 32, 6, dtypes, C.ALL_UNSIGNED, BF16, (3, 140, 250), None, True, (190, 66))
        _equals(c, P.paged(c, 16), 4, dtypes)


@pytest.mark.parametrize("Tk,ps", [(256, 16), (1024, 128)])
def test_the_full_table(Tk, ps):
    """every table entry 2^24: S = 2^32 at 256 keys and 2^34 at 1024, summed over the whole prefix by every split"""
    c = C.case(1, 2, 1, 1, Tk, 64, 3, C.ALL_U8, SIGNED_PV, BF16, Z3, "full", True, None)
    assert len(c.want.unique()) > 16
    _equals(c, P.paged(c, ps), 4, ("full table", Tk))


def test_composition_and_misaligned_operands():
    from torchlsq import extension as E
    # ps 8 and ps 24: legal, not served
    c = C.case(2, 2, 3, 1, 192, 32, 8, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (190, 110))
    _equals(c, P.paged(c, 8), 3, "ps 8", "composition")
    _equals(c, P.paged(c, 24), 3, "ps 24", "composition")
    # R 17 and D 24
    d = C.case(1, 1, 17, 1, 128, 32, 8, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (127,))
    _equals(d, P.paged(d, 16), 2, "R 17", "composition")
    d = C.case(1, 2, 2, 1, 128, 24, 8, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (100,))
    _equals(d, P.paged(d, 16), 2, "D 24", "composition")
    # a pool one byte off, a q one byte off: the composition, the same bytes
    pg = P.paged(c, 16)
    _equals(c, pg, 3, "k_pool one byte off", "composition", (1, 0))
    _equals(c, pg, 3, "v_pool one byte off", "composition", (0, 1))
    _equals(c, pg, 3, "q one byte off", "composition", q_shift=1)
    # a y one byte off: still the paged kernels, with the byte store -- through the C entry and through the host's `out`
    B, H, Hkv, T, Tk, D = c.shape
    pl = P.plan_of(c, pg, 3, y_aligned=False)
    assert pl["family"] == "paged" and pl["store"] == "elements" and P.plan_of(c, pg, 3)["store"] == "packets"
    rc, y, _, _ = P.c_entry(c, pg, DEV, 3, y_shift=1)
    assert rc == 0 and y.data_ptr() % 16 == 1 and torch.equal(y.cpu(), c.want)
    raw = torch.full((B * T * H * D + 2,), GUARD, dtype=U8, device=DEV)
    yv = raw[1:-1].view(B, T, H, D).permute(0, 2, 1, 3)
    kp, vp, bt = P.on(DEV, pg)
    q, sides = C.moved(c.q, DEV), C.F.sides_on(c.sides, DEV)
    E.attn_paged_w8_q(q.levels, q.scale, q.zero_point, kp.levels, kp.scale, kp.zero_point, vp.levels, vp.scale, vp.zero_point, bt,
                      c.table.to(DEV), *sides[0], *sides[1], *sides[2], c.mid, True, Tk - T, c.lengths.to(DEV), splits=3, out=yv)
    assert torch.equal(raw[1:-1].view(B, T, H * D).cpu(), c.want) and int(raw[0]) == GUARD and int(raw[-1]) == GUARD


def test_launches_repeat_and_batches_depend_on_their_own_inputs_alone():
    from torchlsq.functional import lsq_attention_decode_paged_w8_q
    c = C.case(3, 2, 4, 1, 208, 64, 11, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (197, 60, 133))
    pg = P.paged(c, 16)
    first, second = P.run(c, pg, DEV, 4), P.run(c, pg, DEV, 4)
    assert torch.equal(first, second) and torch.equal(first.cpu(), c.want)
    assert torch.equal(P.run(c, pg, DEV, 1), first) and torch.equal(P.run(c, pg, DEV, 2), first) and torch.equal(P.run(c, pg, DEV, 0), first)
    kp, vp, bt = P.on(DEV, pg)
    q, sides, tab = C.moved(c.q, DEV), C.F.sides_on(c.sides, DEV), c.table.to(DEV)
    for b in range(3):                                              # a batch entry alone: its q, its table row, the same pools
        one = lsq_attention_decode_paged_w8_q(C.with_levels(q, q.levels[b:b + 1]), kp, vp, bt[b:b + 1], tab, *sides, c.mid, causal=True,
                                              key_lengths=c.lengths[b:b + 1].to(DEV), splits=4).levels
        assert torch.equal(one[0], first[b]), b
    h, D, G = 1, 64, 4                                              # a kv head alone: its G query heads' columns
    one = lsq_attention_decode_paged_w8_q(C.with_levels(q, q.levels[:, h * G:(h + 1) * G]), C.with_levels(kp, kp.levels[:, h:h + 1]),
                                          C.with_levels(vp, vp.levels[:, h:h + 1]), bt, tab, *sides, c.mid, causal=True,
                                          key_lengths=c.lengths.to(DEV), splits=4).levels
    assert torch.equal(one, first[:, :, h * G * D:(h + 1) * G * D])


# ---------------------------------------------------------------------------------------------------
# the append
# ---------------------------------------------------------------------------------------------------
def _append_case(T, D, positions, order, k_dtype=U8, shift=0, Np=14):
    """(k, v sources on the CPU as views of one qkv buffer, table with an entry of -1 and one of Np, positions)"""
    B, Hkv, ps, Mp = len(positions), 2, 16, 3
    qkv = A.levels((B, T, 3, Hkv, D), 9 + T, U8)
    table = P.tables(B, Mp, Np, "perm", 5).to(torch.int32)
    table[B - 1, 1] = -1
    table[0, 2] = Np
    return qkv[:, :, 1].view(k_dtype), qkv[:, :, 2], table, torch.tensor(positions, dtype=torch.int32), (B, Hkv, ps, Mp, Np)


@pytest.mark.parametrize("T,D,positions,order,k_dtype,shift,kernel", [
    (1, 32, (0, 15, 16, 47), "hsd", U8, 0, "append_packets"), (19, 32, (0, 13), "hsd", U8, 0, "append_packets"),
    (19, 32, (0, 13), "shd", I8, 0, "append_packets"), (19, 32, (40, -3), "hsd", U8, 0, "append_packets"),
    (19, 24, (0, 13), "shd", U8, 0, "append_generic"), (19, 32, (30, 13), "hsd", I8, 1, "append_generic")], ids=str)
def test_append(T, D, positions, order, k_dtype, shift, kernel):
    """T 1, and T 19 from the positions (0, 13) at ps 16 -- tokens that straddle page borders --; p >= Mp ps, p < 0, an entry of -1 and
    one of Np are skipped; packets and the byte path (D 24, a source one byte off); int8: the whole pools against the CPU path's"""
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, lsq_kv_append_paged_w8
    k, v, table, pos, (B, Hkv, ps, Mp, Np) = _append_case(T, D, positions, order, k_dtype, shift)
    consts = (A.one(A.QKV_S), A.one(A.QKV_Z, torch.int32))
    rng = (0, 255) if k_dtype == U8 else (-128, 127)

    def pools(dev):
        shape = (Np + 2, Hkv, ps, D) if order == "hsd" else (Np + 2, ps, Hkv, D)
        out = [torch.full(shape, 0x11, dtype=U8, device=dev).view(k_dtype), torch.full(shape, 0x22, dtype=U8, device=dev)]
        return out, [(p if order == "hsd" else p.permute(0, 2, 1, 3))[1:1 + Np] for p in out]          # a guard page at each end
    (_, (wk, wv)) = pools("cpu")
    lsq_kv_append_paged_w8(LevelsTensor(k, *consts, *rng), LevelsTensor(v, *consts, 0, 255), wk, wv, table, pos)
    ref = pools("cpu")[1]
    P.append_reference(k, v, ref[0], ref[1], table, pos)
    assert torch.equal(wk, ref[0]) and torch.equal(wv, ref[1]) and bool((wk.view(U8) != 0x11).any())
    big, (gk, gv) = pools(DEV)
    kd, vd = (A.place(x, DEV, shift) for x in (k, v))
    assert E.kv_append_paged_w8_plan(B, T, Hkv, D, Np, ps, Mp, k_strides=tuple(kd.stride()[:3]), v_strides=tuple(vd.stride()[:3]),
                                     k_pool_strides=P.pool_strides(gk), v_pool_strides=P.pool_strides(gv), aligned=not shift)["kernel"] == kernel
    cd = tuple(t.to(DEV) for t in consts)
    lsq_kv_append_paged_w8(LevelsTensor(kd, *cd, *rng), LevelsTensor(vd, *cd, 0, 255), gk, gv, table.to(DEV), pos.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(gk.cpu(), wk) and torch.equal(gv.cpu(), wv)
    store = [b if order == "hsd" else b.permute(0, 2, 1, 3) for b in big]
    for s, fill in zip(store, (0x11, 0x22)):
        assert bool((s[0].view(U8) == fill).all()) and bool((s[-1].view(U8) == fill).all()), "a guard page was written"


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
def test_paged_decode_step_replays_in_a_graph():
    """RotaryW8Q, PagedKVCacheW8.append and the core with decode=True and a block table captured once -- the workspace's torch.empty
    inside the capture --; seven replays with only device buffers rewritten: every step is the dense KVCacheW8 + split route's and the
    CPU run's; then the block table is overwritten in place, two pages swapped together with their contents, and the replay follows"""
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import KVCacheW8, PagedKVCacheW8, RotaryW8Q
    case = C.gqa_decode_case()
    B, H, Hkv, T, D, ps, Mp = case["B"], case["H"], case["Hkv"], case["T"], case["D"], 16, 8
    Tmax = ps * Mp
    cpu_core = copy.deepcopy(case["core"])
    cpu_core.decode = True
    cpu_rot = RotaryW8Q(A.trained(-4.0, 4.0), D, Tmax, mid_dtype=BF16)
    start = torch.tensor([60, 11], dtype=torch.int32)              # batch 0 crosses a chunk border (64), batch 1 a page border (16)

    dev_consts = {"cpu": case["consts"], DEV: tuple(c.to(DEV) for c in case["consts"])}      # on the device before the capture

    def paged_step(rot, core, cache, dev, tokens):
        qt, kvt = tokens
        consts = dev_consts[dev]
        q, k, v = LevelsTensor(qt, *consts, 0, 255), LevelsTensor(kvt[:, :, 0], *consts, 0, 255), LevelsTensor(kvt[:, :, 1], *consts, 0, 255)
        rq = rot(q, positions=cache.lengths)
        kp, vp, lens = cache.append(k, v, rotary=rot)
        return core(LevelsTensor(rq.levels.permute(0, 2, 1, 3), rq.scale, rq.zero_point, rq.quant_min, rq.quant_max), kp, vp, key_lengths=lens,
                    block_table=cache.block_table).levels

    cpu_cache = PagedKVCacheW8(2 * Mp + 1, Hkv, ps, D, B, Mp)
    cpu_cache.lengths.copy_(start)
    cpu_steps = [paged_step(cpu_rot, cpu_core, cpu_cache, "cpu", (case["q"][:, t:t + 1], case["kv"][:, t:t + 1])) for t in range(T)]
    rot, core = copy.deepcopy(cpu_rot).to(DEV), copy.deepcopy(cpu_core).to(DEV)
    core.split = 2
    dense_core = copy.deepcopy(core)
    dense = KVCacheW8(B, Hkv, Tmax, D, device=DEV)
    dense.lengths.copy_(start.to(DEV))
    cache = PagedKVCacheW8(2 * Mp + 1, Hkv, ps, D, B, Mp, device=DEV)
    qt, kvt = case["q"][:, :1].to(DEV), case["kv"][:, :1].to(DEV)
    pl = E.attn_paged_w8_plan(B, H, Hkv, 1, D, 2 * Mp + 1, ps, Mp, 2, causal=True, causal_offset=Tmax - 1)
    assert pl["family"] == "paged" and pl["splits"] == 2 and pl["chunk"] == 64
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        paged_step(rot, core, cache, DEV, (qt, kvt))
    torch.cuda.current_stream().wait_stream(side)

    def clear():
        cache.lengths.copy_(start.to(DEV))
        cache.k_pool.zero_()
        cache.v_pool.zero_()
    clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = paged_step(rot, core, cache, DEV, (qt, kvt))
    clear()
    gcase = dict(case, consts=tuple(c.to(DEV) for c in case["consts"]))
    for t in range(T):
        qt.copy_(case["q"][:, t:t + 1])
        kvt.copy_(case["kv"][:, t:t + 1])
        graph.replay()
        want = C.gqa_decode_step(gcase, rot, dense_core, dense, t, DEV, (qt, kvt))
        assert cache.lengths.tolist() == [61 + t, 12 + t]
        assert torch.equal(out, want) and torch.equal(out.cpu(), cpu_steps[t]), t
    assert torch.equal(cache.k_pool.cpu(), cpu_cache.k_pool) and torch.equal(cache.v_pool.cpu(), cpu_cache.v_pool)
    # pages swapped together with their contents: batch 0's live page 3 (keys 48 .. 63) and the spare page 2 Mp
    for cch in (cache, cpu_cache):
        a, b = int(cch.block_table[0, 3]), 2 * Mp
        for pool in (cch.k_pool, cch.v_pool):
            pool[b] = pool[a]
            pool[a] = 0x77
        cch.block_table[0, 3] = b
    qt.copy_(case["q"][:, 5:6])
    kvt.copy_(case["kv"][:, 5:6])
    graph.replay()
    want = C.gqa_decode_step(gcase, rot, dense_core, dense, 5, DEV, (qt, kvt))
    want_cpu = paged_step(cpu_rot, cpu_core, cpu_cache, "cpu", (case["q"][:, 5:6], case["kv"][:, 5:6]))
    assert cache.lengths.tolist() == [68, 19] and torch.equal(out, want) and torch.equal(out.cpu(), want_cpu)
    assert torch.equal(cache.k_pool.cpu(), cpu_cache.k_pool) and torch.equal(cache.v_pool.cpu(), cpu_cache.v_pool)
