"""Chunked prefill attention on 8-bit levels on the GPU (liblsq_hip_attn_chunk_w8.so): every comparison is torch.equal against
`attn_decode_w8_cases.definition` (the parent commit's code) or, for causal="lengths", the per-entry construction from it
(`attn_chunk_w8_cases.want_lengths`).  Before each comparison the plan's family and the forced split count are asserted, and beside
the op the C entry is called directly with a workspace the test made and guard bytes around it and around y
(`attn_chunk_w8_cases.check`).  Shapes are (B, Hkv, G, Tq, Tk, D), the smallest at which each mechanism can fail.
"""
import pytest
import torch

import attn_chunk_w8_cases as K
import attn_decode_w8_cases as C
import attn_paged_w8_cases as P
import attn_w8_cases as A
import decoder_w8_cases as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
Z3 = (A.QKV_Z,) * 3


def case(shape, causal, lengths=None, seed=70, **kw):
    args = dict(dtypes=C.ALL_U8, unsigned=C.ALL_UNSIGNED, mid=BF16, zeros=Z3, table=None)
    args.update(kw)
    c = C.case(*shape, seed, args["dtypes"], args["unsigned"], args["mid"], args["zeros"], args["table"], causal, lengths)
    C.check_not_degenerate(c)
    return c


# ---------------------------------------------------------------------------------------------------
# row tiles
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,causal,tiles", [((1, 1, 1, 17, 17, 16), True, 2), ((1, 2, 3, 21, 40, 32), 19, 4), ((1, 1, 16, 2, 65, 64), True, 2),
                                                ((1, 1, 16, 2, 65, 64), 61, 2)], ids=str)
def test_row_tiles(shape, causal, tiles):
    """two tiles, the second with one live row; R 63: tiles that straddle head borders and a last tile of 15 rows; R 32 with two keys
    either side of a chunk border"""
    c = case(shape, causal)
    assert K.plan_of(c)["tiles"] == tiles
    K.check(c, DEV, c.want)
    if shape[4] > 64:
        K.check(c, DEV, c.want, splits=2, forced=2)


# ---------------------------------------------------------------------------------------------------
# tile and chunk skipping
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,causal,splits", [((1, 1, 1, 130, 130, 16), True, 3), ((1, 1, 2, 70, 200, 32), 130, 4)], ids=str)
def test_tile_and_chunk_skipping(shape, causal, splits):
    """chunks of 64: tile 0 needs chunk 0 only, later tiles more, the last chunk holds 2 (8) keys; 1 split and the library's choice give
    the same bytes"""
    c = case(shape, causal)
    pl = K.plan_of(c, splits=splits)
    assert pl["chunk"] == 64 and pl["splits"] == splits and pl["grid"] == pl["tiles"] * splits * shape[1]
    got = K.check(c, DEV, c.want, splits=splits, forced=splits)
    assert torch.equal(K.check(c, DEV, c.want, splits=1, forced=1), got)
    assert torch.equal(K.check(c, DEV, c.want, splits=0), got)


# ---------------------------------------------------------------------------------------------------
# lengths
# ---------------------------------------------------------------------------------------------------
LENS15 = (-3, 0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 199, 200, 205)


@pytest.mark.parametrize("causal", [0, 5, True, None, "lengths"], ids=str)       # (None: not causal)
def test_key_lengths_in_every_mode(causal):
    shape = (15, 1, 2, 70, 200, 32)
    if causal == "lengths":
        c = case(shape, True)
        want = K.want_lengths(c, LENS15)
        assert bool((want[2, :69] == K.level_of_zero(c)).all()) and len(want.unique()) > 16          # rows with n = 0 below a length of 70
        K.check(c, DEV, want, "lengths", 4, lengths=LENS15, forced=4)
        K.check(c, DEV, want, "lengths", 0, lengths=LENS15)
    else:
        c = case(shape, causal, LENS15)
        K.check(c, DEV, c.want, splits=4, forced=4)


# ---------------------------------------------------------------------------------------------------
# beyond the prefill kernel
# ---------------------------------------------------------------------------------------------------
def test_beyond_the_prefill_kernels_keys():
    from torchlsq import extension as E
    c = case((1, 1, 1, 33, 2100, 16), True, unsigned=P.SIGNED_PV)
    assert E.attn_prefill_w8_plan(1, 1, 1, 33, 2100, 16, causal=True, causal_offset=2100 - 33)["family"] == "composition"
    K.check(c, DEV, c.want)


def test_65536_keys():
    """the chunk's raw sums pass 2^31 with one split of 65530 keys"""
    c = case((1, 1, 1, 17, 65536, 16), True, unsigned=P.SIGNED_PV)
    want = K.want_lengths(c, (65530,))
    pl = K.plan_of(c, "lengths", 0, lengths=(65530,))
    assert pl["family"] == "chunk" and pl["splits"] == 64 and pl["tiles"] == 2
    K.check(c, DEV, want, "lengths", 0, lengths=(65530,))
    K.check(c, DEV, want, "lengths", 1, lengths=(65530,), forced=1)


# ---------------------------------------------------------------------------------------------------
# paged
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["hsd", "shd"])
def test_paged_across_a_page_and_a_chunk_border(order):
    c = case((2, 2, 4, 20, 128, 64), True, unsigned=P.SIGNED_PV)
    lens = (61, 128)
    want = K.want_lengths(c, lens)
    pg = P.paged(c, 16, "perm", order, bt_pad=3)
    assert pg.Mp == 8
    K.check(c, DEV, want, "lengths", 2, pg, lens, forced=2)
    K.check(c, DEV, want, "lengths", 0, pg, lens)
    K.check(c, DEV, c.want, True, 2, pg, None, forced=2)


def test_paged_page_sizes_and_table_entries():
    c = case((2, 2, 4, 20, 256, 64), True, unsigned=P.SIGNED_PV)
    lens = (61, 140)
    want = K.want_lengths(c, lens)
    K.check(c, DEV, want, "lengths", 0, P.paged(c, 128), lens)                                 # ps 128, Mp 2
    K.check(c, DEV, want, "lengths", 0, P.paged(c, 8), lens, family="composition")             # ps 8: the gather and the composition
    pg = P.paged(c, 16)
    kp, vp, bt = P.on(DEV, pg)
    for wild in (2 ** 31 - 1, -1):                      # entries at logical pages >= ceil(nmax(b) / ps) are never read
        t = bt.clone()
        t[0, 4:] = wild                                 # nmax(0) = 61: pages 0 .. 3
        t[1, 9:] = wild                                 # nmax(1) = 140: pages 0 .. 8
        K.check(c, DEV, want, "lengths", 2, pg, lens, operands=(kp, vp, t), forced=2)
    t = pg.table.clone()
    t[0, 1], t[1, 2] = pg.Np + 5, -9                    # below that bound: READS CLAMP, the bytes are the gather's
    clamped = K.run(c, "cpu", "lengths", pg=pg, lengths=lens, operands=(pg.k_pool, pg.v_pool, t))
    assert not torch.equal(clamped, want)
    K.check(c, DEV, clamped, "lengths", 2, pg, lens, operands=(kp, vp, t.to(DEV)), forced=2)


# ---------------------------------------------------------------------------------------------------
# never read, never depended on
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quant_min", [None, 5])
def test_slots_beyond_nmax_are_never_read(quant_min):
    c = case((3, 2, 2, 20, 128, 32), True)
    lens = (128, 70, 9)
    if quant_min is not None:                           # the probabilities' level of 0.0 is 5, their z_p is 0: the byte z_p fills [n_r, chunk end)
        d = C.Case()
        d.shape, d.G, d.mid, d.causal, d.lengths, d.table, d.q, d.k, d.v = c.shape, c.G, c.mid, c.causal, c.lengths, c.table, c.q, c.k, c.v
        p = c.sides[1]
        d.sides = (c.sides[0], (p[0], p[1], quant_min) + tuple(p[3:]), c.sides[2])
        c = C.finish(d)
    want = K.want_lengths(c, lens)
    k, v = K.poisoned(c, "lengths", lens, 0xFF)
    assert torch.equal(K.run(c, DEV, "lengths", 2, lengths=lens, operands=(C.moved(k, DEV), C.moved(v, DEV))).cpu(), want)
    pg = P.paged(c, 16)
    K.check(c, DEV, want, "lengths", 2, pg, lens, operands=P.on(DEV, K.poisoned(c, "lengths", lens, 0xFF, pg)), forced=2)


def test_the_workspace_is_never_depended_on():
    c = case((2, 1, 2, 70, 200, 32), True)
    want = {}
    for fill in (0x00, 0xFF):
        for lens in ((200, 131), (70, 5)):
            want[lens] = K.want_lengths(c, lens)
            K.check(c, DEV, want[lens], "lengths", 4, lengths=lens, fill=fill, forced=4)
    # three shorter calls, n = 0 among them, in the workspace a longer call left
    rc, y, ws, need = K.c_entry(c, DEV, "lengths", 4, lengths=(200, 200))
    assert rc == 0 and torch.equal(y.cpu(), K.want_lengths(c, (200, 200)))
    for lens in ((131, 64), (70, 0), (1, -2)):
        rc, y, _, _ = K.c_entry(c, DEV, "lengths", 4, lengths=lens, ws=ws)
        assert rc == 0 and torch.equal(y.cpu(), K.want_lengths(c, lens)), lens
        assert bool((ws[need:] == K.GUARD).all())


# ---------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", [F32, BF16, F16], ids=lambda m: str(m).replace("torch.", ""))
@pytest.mark.parametrize("combo", [0, 1, 2])
def test_level_dtypes_and_mid_dtypes(combo, mid):
    dtypes, unsigned = (((C.ALL_U8, C.ALL_UNSIGNED),) + tuple(C.COMBOS))[combo]       # all uint8, and the two mixed combinations
    c = case((1, 2, 2, 33, 65, 64), True, dtypes=dtypes, unsigned=unsigned, mid=mid)
    K.check(c, DEV, K.want_lengths(c, (50,)), "lengths", 2, lengths=(50,), forced=2)


def test_zero_points_and_the_full_table():
    c = case((1, 2, 2, 33, 65, 64), True, zeros=(3, 140, 250))
    K.check(c, DEV, c.want, splits=2, forced=2)
    for Tk in (256, 1024):                              # every table entry 2^24: S = 2^32 and 2^34
        c = case((1, 1, 1, 17, Tk, 16), True, table="full", unsigned=P.SIGNED_PV)
        K.check(c, DEV, c.want, splits=2, forced=2)


def test_alignment_routes():
    c = case((1, 2, 2, 33, 65, 64), True)
    want = K.want_lengths(c, (50,))
    K.check(c, DEV, want, "lengths", 2, lengths=(50,), y_shift=1, y_aligned=False, forced=2)           # the byte store, still "chunk"
    assert K.plan_of(c, "lengths", 2, lengths=(50,), y_aligned=False)["store"] == "elements"
    for shift in ((1, 0, 0), (0, 1, 0)):                # q or k one byte off: the composition, the same bytes
        K.check(c, DEV, want, "lengths", 2, lengths=(50,), shift=shift, qkv_aligned=False, family="composition")
    c = case((1, 2, 2, 33, 65, 24), True)
    K.check(c, DEV, K.want_lengths(c, (50,)), "lengths", 0, lengths=(50,), family="composition")


# ---------------------------------------------------------------------------------------------------
# against the existing kernels
# ---------------------------------------------------------------------------------------------------
def test_against_the_prefill_and_the_decode_kernels():
    from torchlsq import extension as E
    from torchlsq.functional import lsq_attention_decode_w8_q, lsq_attention_prefill_w8_q
    c = case((2, 2, 2, 21, 96, 32), True, (96, 50))
    B, H, Hkv, Tq, Tk, D = c.shape
    assert E.attn_prefill_w8_plan(B, H, Hkv, Tq, Tk, D, causal=True, causal_offset=Tk - Tq)["family"] == "prefill"
    q, k, v = (C.moved(x, DEV) for x in (c.q, c.k, c.v))
    sides, tab, lens = C.F.sides_on(c.sides, DEV), c.table.to(DEV), c.lengths.to(DEV)
    pre = lsq_attention_prefill_w8_q(q, k, v, tab, *sides, c.mid, causal=True, key_lengths=lens).levels
    got = K.check(c, DEV, c.want, splits=2, forced=2)
    assert torch.equal(got, pre)
    assert torch.equal(K.run(c, DEV, splits=2), got)                                           # calls repeat bit for bit
    # every row of the chunk: the decode op's Tq = 1 call at that row's key count
    n = K.key_counts(c, True, (96, 50))
    for t in range(Tq):                                 # rows 15 / 16 and 31 / 32 lie on tile borders, 20 / 21 on the head border
        row = lsq_attention_decode_w8_q(C.with_levels(q, q.levels[:, :, t:t + 1]), k, v, tab, *sides, c.mid, causal=None,
                                        key_lengths=torch.tensor([n[0][t], n[1][t]], dtype=torch.int32, device=DEV)).levels
        assert torch.equal(row, got[:, t:t + 1]), t
    # a batch entry alone and a kv head alone
    one = C.Case()
    one.shape, one.G, one.table, one.sides, one.mid, one.causal = (1, H, Hkv, Tq, Tk, D), c.G, c.table, c.sides, c.mid, True
    one.q, one.k, one.v = (C.with_levels(x, x.levels[1:2]) for x in (c.q, c.k, c.v))
    one.lengths, one.want = c.lengths[1:2], c.want[1:2]
    assert torch.equal(K.run(one, DEV, splits=2), got[1:2])
    G = c.G
    head = C.Case()
    head.shape, head.G, head.table, head.sides, head.mid, head.causal, head.lengths = (B, G, 1, Tq, Tk, D), G, c.table, c.sides, c.mid, True, c.lengths
    head.q = C.with_levels(c.q, c.q.levels[:, G:2 * G])
    head.k, head.v = (C.with_levels(x, x.levels[:, 1:2]) for x in (c.k, c.v))
    assert torch.equal(K.run(head, DEV, splits=2), got.view(B, Tq, H, D)[:, :, G:2 * G].reshape(B, Tq, G * D))


# ---------------------------------------------------------------------------------------------------
# the layer, and a graph
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", list(K.CHUNKINGS))
@pytest.mark.parametrize("route", ["dense", "paged"])
def test_the_decoder_layer_in_chunks(route, how):
    want = L.cpu_run("long", BF16, "whole")
    xl = L.input_levels("long")
    xg = type(xl)(xl.levels.to(DEV), xl.scale.to(DEV), xl.zero_point.to(DEV), xl.quant_min, xl.quant_max, xl.type_min, xl.type_max)
    layer = K.chunk_layer("long", BF16, DEV)
    with torch.no_grad():
        got = K.layer_sequence(layer, xg, L.make_cache("long", route, DEV), K.CHUNKINGS[how])
    assert L.differing(got, want) == [], (route, how, L.differing(got, want))


@pytest.mark.parametrize("route", ["dense", "paged"])
def test_a_prompt_chunk_replays_in_a_graph(route):
    """ONE prompt chunk of 8 tokens of the whole layer -- rotary, append, the core with chunk=True and causal="lengths", the workspace
    allocated inside -- captured once and replayed for eight successive chunks with only device buffers rewritten (the token levels;
    `lengths` follows by itself), then once with the two batch entries' lengths made different in place: each replay is the CPU run"""
    T = 8
    cpu = L.cpu_run("long", BF16, "whole")
    xl = L.input_levels("long")
    xs = xl.levels.to(DEV)
    consts = (xl.scale.to(DEV), xl.zero_point.to(DEV), xl.quant_min, xl.quant_max, xl.type_min, xl.type_max)
    layer = K.chunk_layer("long", BF16, DEV)
    cache = L.make_cache("long", route, DEV)
    B = int(xs.shape[0])
    token = type(xl)(xs[:, :T].contiguous(), *consts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        K.layer_run(layer, token, cache)
    torch.cuda.current_stream().wait_stream(side)
    cache.lengths.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        _, held = K.layer_run(layer, token, cache)
    cache.lengths.zero_()

    def compare(starts):
        for s in L.STAGES:
            got = held[s].levels.reshape(B, T, -1).cpu()
            for b, st in enumerate(starts):
                assert torch.equal(got[b], cpu[s][b, st:st + T]), (route, starts, s, b)
    for i in range(8):
        token.levels.copy_(xs[:, i * T:(i + 1) * T])
        graph.replay()
        compare([i * T] * B)
        assert cache.lengths.tolist() == [(i + 1) * T] * B
    for got, want in zip(L.cached(cache, held["k_cache"], held["v_cache"], 8 * T), (cpu["k"], cpu["v"])):
        assert torch.equal(got.cpu(), want[:, :, :8 * T])
    starts = [16, 40]                                   # a ragged batch: the same graph, the lengths rewritten in place
    cache.lengths.copy_(torch.tensor(starts, dtype=torch.int32))
    for b, st in enumerate(starts):
        token.levels[b].copy_(xs[b, st:st + T])
    graph.replay()
    compare(starts)
    assert cache.lengths.tolist() == [st + T for st in starts]
