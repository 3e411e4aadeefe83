"""The paged KV cache on 8-bit levels without a GPU: the plan (host only) -- its formulas, the two families on both sides of every
bound, every refusal with its message --, the CPU path of the paged decode against the dense decode op on the same logical keys
(`attn_decode_w8_cases.definition`, the parent commit's code) under different block tables and pool orders, shared pages, a padded
table, clamped entries, the append with skipped tokens against plain loops (whole pools compared), `PagedKVCacheW8` against `KVCacheW8`
over seven decode steps, and `AttentionCoreW8Q` without a block table.  Every comparison is torch.equal.
"""
import copy
import ctypes

import pytest
import torch

import attn_decode_w8_cases as C
import attn_paged_w8_cases as P
import attn_w8_cases as A

U8, I8, BF16 = A.U8, A.I8, A.BF16
Z3 = P.Z3


def E():
    from torchlsq import extension
    return extension


# ---------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Hkv,G,Tq,D,ps,Mp,splits", [(1, 1, 1, 1, 16, 16, 1, 0), (2, 2, 4, 1, 32, 16, 13, 2), (2, 2, 4, 1, 32, 16, 13, 4),
                                                       (1, 1, 8, 2, 128, 128, 2, 0), (1, 1, 4, 1, 64, 256, 4, 16), (4, 8, 4, 1, 128, 16, 512, 0),
                                                       (1, 8, 4, 1, 128, 128, 256, 0), (1, 1, 1, 1, 128, 256, 256, 0)])
def test_plan_formulas(B, Hkv, G, Tq, D, ps, Mp, splits):
    Tk, R, heads = Mp * ps, G * Tq, B * Hkv
    pl = E().attn_paged_w8_plan(B, Hkv * G, Hkv, Tq, D, B * Mp + 1, ps, Mp, splits)
    units = -(-Tk // 64)
    if splits:
        chunk = 64 * -(-units // splits)
    else:                                               # the split library's rule and constants
        fewest = min(-(-4 * 256 // heads), 64)
        chunk = min(max(64 * -(-units // fewest), 256), 2048)
    S = -(-Tk // chunk)
    assert pl == dict(family="paged", grid=heads * S, reduce_grid=heads, threads=256, rows=R, chunk=chunk, splits=S, lds_bytes=3840 + 160 * D,
                      store="packets", workspace_bytes=heads * R * Tk + 8 * heads * S * R * D), pl
    sp = E().attn_decode_split_w8_plan(B, Hkv * G, Hkv, Tq, Tk, D, splits)
    assert (sp["chunk"], sp["splits"], sp["workspace_bytes"]) == (pl["chunk"], pl["splits"], pl["workspace_bytes"])


def test_families_on_both_sides_of_each_bound():
    plan = E().attn_paged_w8_plan

    def fam(**kw):
        a = dict(B=2, H=8, Hkv=2, Tq=1, D=64, num_pages=9, page_size=16, max_pages=4)
        a.update(kw)
        return plan(**a)["family"]
    assert fam() == "paged"
    assert fam(H=32) == "paged" and fam(H=34) == "composition"                  # R 16 | 17
    assert fam(H=16, Tq=2) == "paged" and fam(H=16, Tq=3) == "composition"      # R 16 | 24
    assert fam(D=16) == "paged" and fam(D=128) == "paged"
    for D in (8, 24, 144):
        assert fam(D=D) == "composition", D
    for ps in (16, 32, 1024):
        assert fam(page_size=ps) == "paged", ps
    for ps in (1, 8, 24, 48):
        assert fam(page_size=ps) == "composition", ps
    assert fam(page_size=256, max_pages=256) == "paged"                         # the capacity
    assert fam(qkv_aligned=False) == "composition"
    assert fam(k_strides=(2 * 16 * 64 + 8, 16 * 64, 64)) == "composition" and fam(k_strides=(2 * 16 * 64 + 16, 16 * 64, 64)) == "paged"
    assert fam(v_strides=(2 * 16 * 72, 16 * 72, 72)) == "composition" and fam(v_strides=(2 * 16 * 80, 16 * 80, 80)) == "paged"
    assert fam(k_strides=(2 * 16 * 64, 64, 2 * 64), v_strides=(2 * 16 * 64, 64, 2 * 64)) == "paged"         # [Np, ps, Hkv, D]
    assert fam(q_strides=(8 * 64 + 4, 64, 64)) == "composition"
    pl = plan(2, 8, 2, 1, 64, 9, 16, 4, y_aligned=False)
    assert pl["family"] == "paged" and pl["store"] == "elements"
    assert fam(bt_ld=7) == "paged"


def test_plan_refusals():
    plan = E().attn_paged_w8_plan

    def refused(msg, **kw):
        a = dict(B=2, H=8, Hkv=2, Tq=1, D=64, num_pages=9, page_size=16, max_pages=4)
        a.update(kw)
        with pytest.raises(RuntimeError, match=msg):
            plan(**a)
    refused("every extent must be at least 1", page_size=0)
    refused("every extent must be at least 1", max_pages=0)
    refused("every extent must be at least 1", num_pages=0)
    refused("at most 65536 are served", page_size=256, max_pages=257)
    refused("at most 65536 are served", page_size=16, max_pages=4097)
    refused("row stride bt_ld = 3 is smaller than its row of Mp = 4", bt_ld=3)
    refused("pages, heads or slots of a pool overlap each other", k_strides=(16 * 64, 16 * 64, 64))
    refused("pages, heads or slots of a pool overlap each other", v_strides=(2 * 16 * 64, 16 * 64, 64 * 16))
    refused("k_pool's row stride 32 is smaller than its row of 64", k_strides=(2 * 16 * 64, 16 * 64, 32))
    refused("not a multiple of Hkv", H=7)
    refused("causal_offset = -1 must be at least 0", causal=True, causal_offset=-1)
    refused(r"splits = 2 must be 0 \(the library's choice\) or 1 .. ceil\(Tk / 64\) = 1", splits=2)
    refused("beyond 2\\^31 - 1", num_pages=2 ** 31)
    refused("y's rows or batches overlap", y_strides=(0, 64, 512))
    with pytest.raises(RuntimeError, match="splits must be an int"):
        plan(2, 8, 2, 1, 64, 9, 16, 4, splits=-1)


def test_c_entry_refusals_without_a_gpu():
    """the structs straight into the library: NULL pages, Tk that is not Mp ps, a NULL and a misaligned block table -- all before
    anything could be enqueued"""
    ext = E()
    lib = ext.attn_paged_w8_library()
    S = ext.LsqAttnW8Strides
    geom = ext.LsqAttnDecodeW8Geom(1, 1, 1, 1, 64, 16, 0, 0, 0, 0, 0, 0, S(16, 16, 16), S(256, 256, 16), S(256, 256, 16), S(16, 16, 16))
    pages = ext.LsqAttnPagedW8Pages(2, 16, 4, 4)
    out, ws = (ctypes.c_int32 * 8)(), ctypes.c_int64(-1)

    def err():
        return lib.lsq_attn_paged_w8_last_error().decode()
    assert lib.lsq_attn_paged_w8_abi_version() == 1
    assert lib.lsq_attn_paged_w8_plan(ctypes.byref(geom), None, 1, 1, 0, ctypes.byref(out)) == -1 and "NULL pages" in err()
    assert lib.lsq_attn_paged_w8_plan(ctypes.byref(geom), ctypes.byref(pages), 1, 1, 0, None) == -1 and "NULL output" in err()
    assert lib.lsq_attn_paged_w8_workspace(ctypes.byref(geom), ctypes.byref(pages), 0, None) == -1 and "NULL bytes" in err()
    assert lib.lsq_attn_paged_w8_workspace(ctypes.byref(geom), ctypes.byref(pages), 0, ctypes.byref(ws)) == 0 and ws.value == 64 + 8 * 16
    geom.Tk = 65
    assert lib.lsq_attn_paged_w8_plan(ctypes.byref(geom), ctypes.byref(pages), 1, 1, 0, ctypes.byref(out)) == -1
    assert "Tk = 65 is not the table's capacity Mp ps = 4 x 16" in err()
    geom.Tk = 64
    # the decode entry: every pointer check comes before a launch (the buffers are host memory that is never touched)
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    f, z = ctypes.c_float(1.0), ctypes.c_int32(0)
    fa, za = ctypes.addressof(f), ctypes.addressof(z)
    consts = ext.LsqAttnDecodeW8Consts(fa, za, fa, za, fa, za, fa, za)
    o = ext.LsqAttnW8Out(fa, fa, 0, 255, 0, 255, 0)

    def decode(bt, k=base + 1024, y=base, ws_ptr=base + 3072, ws_bytes=4096):
        return lib.lsq_attn_paged_w8_decode(ctypes.byref(geom), ctypes.byref(pages), ctypes.byref(consts), ctypes.byref(o), ctypes.byref(o),
                                            ctypes.byref(o), base + 64, None, bt, base + 32, k, base + 2048, y, ws_ptr, ws_bytes, 0, None)
    assert decode(None) == -1 and "NULL block table" in err()
    assert decode(base + 17) == -1 and "the block table must be 4-byte aligned" in err()
    assert decode(base + 3000, k=base + 1025) == -1 and "is not served by the paged kernels" in err() and "gather the pages" in err()
    assert decode(base + 3000, ws_ptr=None) == -1 and "NULL workspace (192 bytes are needed" in err()
    assert decode(base + 3000, ws_bytes=191) == -1 and "the workspace has 191 bytes, 192 are needed" in err()
    assert decode(base + 3000, ws_ptr=base + 3072 + 8) == -1 and "the workspace must be 16-byte aligned" in err()
    assert decode(base + 3000, y=base + 1024 + 16) == -1 and "y's 16 bytes overlap" in err()
    assert decode(base + 1024 + 40) == -1 and "the block table's 16 bytes overlap a pool" in err()
    assert decode(base + 3000, ws_ptr=base + 2992) == -1 and "the workspace's 192 bytes overlap" in err()


def test_append_plan_and_refusals():
    plan = E().kv_append_paged_w8_plan
    assert plan(2, 19, 2, 32, 10, 16, 4) == dict(family="packets", grid=-(-2 * 2 * 19 * 2 * 2 // 256), threads=256, units=2, kernel="append_packets")
    assert plan(2, 19, 2, 24, 10, 16, 4) == dict(family="generic", grid=-(-2 * 2 * 19 * 2 * 24 // 256), threads=256, units=24, kernel="append_generic")
    assert plan(2, 1, 2, 32, 10, 16, 4, aligned=False)["kernel"] == "append_generic"
    assert plan(2, 1, 2, 32, 10, 24, 4)["kernel"] == "append_packets"                       # any page size
    assert plan(2, 1, 2, 32, 10, 16, 4, k_strides=(3 * 64, 3 * 64, 32))["kernel"] == "append_packets"      # a view of a qkv buffer
    assert plan(2, 1, 2, 32, 10, 16, 4, v_strides=(200, 200, 40))["kernel"] == "append_generic"
    assert plan(2, 1, 2, 32, 10, 16, 4, k_pool_strides=(1024, 32, 64), v_pool_strides=(1024, 32, 64))["kernel"] == "append_packets"
    for msg, kw in (("every extent must be at least 1", dict(page_size=0)), ("bt_ld = 3 is smaller", dict(bt_ld=3)),
                    ("pages, heads or slots of a pool overlap", dict(k_pool_strides=(512, 512, 32))),
                    ("a pool's slot stride", dict(v_pool_strides=(1024, 512, 16))), ("negative", dict(k_strides=(-1, 64, 32))),
                    ("are more than 2\\^40 elements", dict(B=2 ** 20, T=2 ** 20, k_strides=(0, 0, 32), v_strides=(0, 0, 32)))):
        a = dict(B=2, T=1, Hkv=2, D=32, num_pages=10, page_size=16, max_pages=4)
        a.update(kw)
        with pytest.raises(RuntimeError, match=msg):
            plan(**a)


# ---------------------------------------------------------------------------------------------------
# the CPU path of the decode
# ---------------------------------------------------------------------------------------------------
def test_the_gather_is_the_definition_of_the_layout():
    from torchlsq.functional import lsq_kv_gather_paged_w8
    c = C.case(2, 2, 2, 1, 48, 32, 0, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (40, 9))
    for order in ("hsd", "shd"):
        pg = P.paged(c, 16, "perm", order)
        k, v = P.gathered(pg)
        assert torch.equal(k.levels, c.k.levels) and torch.equal(v.levels, c.v.levels) and k.levels.is_contiguous()
        assert torch.equal(k.scale, pg.k_pool.scale) and (k.quant_min, k.quant_max) == (0, 255)
        for b in range(2):
            for j in (0, 15, 16, 47):
                assert torch.equal(k.levels[b, :, j], pg.k_pool.levels[int(pg.table[b, j // 16]), :, j % 16])
    # entries outside 0 .. Np - 1 are clamped
    t = pg.table.clone()
    t[0, 1], t[1, 2] = -5, 1000
    want = pg.table.clone()
    want[0, 1], want[1, 2] = 0, pg.Np - 1
    assert torch.equal(lsq_kv_gather_paged_w8(pg.k_pool, t).levels, lsq_kv_gather_paged_w8(pg.k_pool, want).levels)


@pytest.mark.parametrize("ps", [16, 8, 24])
def test_cpu_path_equals_the_dense_decode_op(ps):
    """two block tables and both pool orders, served and composition page sizes: the dense op on a contiguous cache of the same keys"""
    for dtypes, unsigned in C.COMBOS:
        c = C.case(2, 2, 2, 1, 48, 32, 1, dtypes, unsigned, BF16, Z3, None, True, (41, 17))
        for kind, order in (("perm", "hsd"), ("rev", "shd")):
            pg = P.paged(c, ps, kind, order, seed=ps)
            assert not torch.equal(pg.table, P.tables(2, 48 // ps, pg.Np, "ident").to(torch.int32))
            assert torch.equal(P.run(c, pg, "cpu"), c.want), (ps, kind, order)
            assert torch.equal(P.run(c, pg, "cpu", splits=1), c.want)
    # Tq 2 with a causal offset, no lengths
    c = C.case(1, 2, 2, 2, 48, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, 20, None)
    assert torch.equal(P.run(c, P.paged(c, ps, "perm", "shd"), "cpu"), c.want)


def test_pages_shared_between_two_batch_entries():
    """both batch entries name the SAME first two pages (a shared prompt) and own their last: the definition on the gathered keys"""
    c = C.case(2, 2, 2, 1, 48, 32, 3, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (45, 38))
    k, v = c.k.levels.clone(), c.v.levels.clone()
    k[1, :, :32], v[1, :, :32] = k[0, :, :32], v[0, :, :32]
    d = C.Case()
    d.shape, d.G, d.mid, d.causal, d.lengths, d.table, d.sides, d.q = c.shape, c.G, c.mid, c.causal, c.lengths, c.table, c.sides, c.q
    d.k, d.v = C.with_levels(c.k, k), C.with_levels(c.v, v)
    C.finish(d)
    table = torch.tensor([[4, 1, 3], [4, 1, 0]], dtype=torch.int64)
    pg = P.paged(d, 16, table=table, extra=0)
    assert pg.Np == 6 and torch.equal(P.gathered(pg)[0].levels, k)
    assert torch.equal(P.run(d, pg, "cpu"), d.want) and not torch.equal(d.want[0], d.want[1])


def test_a_padded_table_and_clamped_entries():
    c = C.case(2, 2, 2, 1, 48, 32, 4, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (48, 33))
    pg = P.paged(c, 16, "perm", bt_pad=5)
    assert pg.table.stride(0) == 8 and not pg.table.is_contiguous()
    assert P.plan_of(c, pg)["family"] == "paged"
    assert torch.equal(P.run(c, pg, "cpu"), c.want)
    # a live entry below 0 reads page 0, one at Np reads page Np - 1: the definition on the clamped table
    for bad, to in ((-1, 0), (pg.Np, pg.Np - 1), (2 ** 31 - 1, pg.Np - 1)):
        t, want_t = pg.table.clone(), pg.table.clone()
        t[1, 1], want_t[1, 1] = bad, to
        k, v = P.gathered(pg, want_t)
        want = C.definition(c, k=k, v=v)
        assert not torch.equal(want, c.want)
        assert torch.equal(P.run(c, pg, "cpu", table=t), want), bad


def test_operand_checks():
    from torchlsq.functional import lsq_attention_decode_paged_w8_q
    c = C.case(2, 2, 2, 1, 48, 32, 4, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (48, 33))
    pg = P.paged(c, 16)

    def call(kp=pg.k_pool, vp=pg.v_pool, bt=pg.table, **kw):
        return lsq_attention_decode_paged_w8_q(c.q, kp, vp, bt, c.table, *c.sides, c.mid, causal=True, key_lengths=c.lengths, **kw)
    with pytest.raises(RuntimeError, match="block_table must be an int32 tensor"):
        call(bt=pg.table.to(torch.int64))
    with pytest.raises(RuntimeError, match="block_table must be an int32 tensor"):
        call(bt=pg.table[:1])
    with pytest.raises(RuntimeError, match="the pools must have one shape"):
        call(vp=C.with_levels(pg.v_pool, pg.v_pool.levels[:, :, :8]))
    with pytest.raises(RuntimeError, match="innermost stride is 1"):
        call(kp=C.with_levels(pg.k_pool, pg.k_pool.levels.transpose(2, 3).contiguous().transpose(2, 3)))
    with pytest.raises(AssertionError, match="splits must be an int >= 0"):
        call(splits=-1)
    assert torch.equal(call(splits=1000).levels, c.want)          # clamped to one split per 64 keys
    # the op itself, its fake kernel and the refusal of grad
    args = (c.q.levels, c.q.scale, c.q.zero_point, pg.k_pool.levels, pg.k_pool.scale, pg.k_pool.zero_point, pg.v_pool.levels, pg.v_pool.scale,
            pg.v_pool.zero_point, pg.table, c.table, *c.sides[0], *c.sides[1], *c.sides[2], c.mid, True, 47, c.lengths, 0)
    assert torch.equal(torch.ops.torchlsq.lsq_attention_decode_paged_w8_q8_q(*args), c.want)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=True):
        fake = torch.ops.torchlsq.lsq_attention_decode_paged_w8_q8_q(*args)
    assert fake.shape == c.want.shape and fake.dtype == c.want.dtype
    with pytest.raises(RuntimeError):
        torch.ops.torchlsq.lsq_attention_decode_paged_w8_q8_q(*args[:1], args[1].clone().requires_grad_(), *args[2:])


# ---------------------------------------------------------------------------------------------------
# the append
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["hsd", "shd"])
def test_append_with_skipped_tokens(order):
    """T 19 from the positions (0, 13, 40, -3) at ps 16 and Mp 3: tokens that straddle page borders, tokens at and beyond the capacity
    of 48, tokens below 0, an entry of -1 and one of Np: the whole pools against plain loops"""
    from torchlsq.functional import LevelsTensor, lsq_kv_append_paged_w8
    B, T, Hkv, D, ps, Mp, Np = 4, 19, 2, 32, 16, 3, 14
    qkv = A.levels((B, T, 3, Hkv, D), 7, U8)
    consts = (A.one(A.QKV_S), A.one(A.QKV_Z, torch.int32))
    k, v = LevelsTensor(qkv[:, :, 1], *consts, 0, 255), LevelsTensor(qkv[:, :, 2].view(I8), *consts, -128, 127)
    table = P.tables(B, Mp, Np, "perm", 5).to(torch.int32)
    table[1, 1], table[2, 2] = -1, Np
    pos = torch.tensor([0, 13, 40, -3], dtype=torch.int32)

    def pools():
        shape = (Np, Hkv, ps, D) if order == "hsd" else (Np, ps, Hkv, D)
        out = [torch.full(shape, 0x11, dtype=U8), torch.full(shape, 0x22, dtype=U8).view(I8)]
        return [p if order == "hsd" else p.permute(0, 2, 1, 3) for p in out]
    wk, wv = pools()
    P.append_reference(k.levels, v.levels, wk, wv, table, pos)
    gk, gv = pools()
    rk, rv = lsq_kv_append_paged_w8(k, v, gk, gv, table, pos)
    assert rk.levels is gk and rv.levels is gv and rv.quant_min == -128 and torch.equal(rk.scale, k.scale)
    assert torch.equal(gk, wk) and torch.equal(gv, wv)
    # batch 0 writes 19 slots; batch 1 the slots 13 .. 15 and, its page 1 being -1, none of 16 .. 31; batch 2 the slots 40 .. 47 of a
    # page named Np: none; batch 3 the tokens 3 .. 18 at the slots 0 .. 15
    assert int((gk != 0x11).any(-1).any(1).sum()) == 19 + 3 + 0 + 16
    # positions None: zeros
    wk, wv = pools()
    P.append_reference(k.levels, v.levels, wk, wv, table, None)
    gk, gv = pools()
    lsq_kv_append_paged_w8(k, v, gk, gv, table)
    assert torch.equal(gk, wk) and torch.equal(gv, wv)
    with pytest.raises(RuntimeError, match="must have their pools' level dtypes"):
        lsq_kv_append_paged_w8(v, v, gk, gv, table)
    with pytest.raises(RuntimeError, match="k_pool overlaps k"):
        lsq_kv_append_paged_w8(LevelsTensor(gk[:4, :, :1].permute(0, 2, 1, 3), *consts, 0, 255), LevelsTensor(v.levels[:, :1], *consts, -128, 127),
                               gk, gv, table)


# ---------------------------------------------------------------------------------------------------
# the modules
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_major", [True, False])
def test_paged_cache_seven_decode_steps_equal_the_dense_cache(page_major):
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import KVCacheW8, PagedKVCacheW8, RotaryW8Q
    case = C.gqa_decode_case()
    B, H, Hkv, T, D = case["B"], case["H"], case["Hkv"], case["T"], case["D"]
    rot = RotaryW8Q(A.trained(-4.0, 4.0), D, 32, mid_dtype=BF16)
    core = copy.deepcopy(case["core"])
    core.decode = True
    dense, paged = KVCacheW8(B, Hkv, 32, D), PagedKVCacheW8(5, Hkv, 16, D, B, 2, page_major=page_major)
    assert paged.block_table.tolist() == [[0, 2], [1, 3]] and paged.block_table.dtype == torch.int32
    assert tuple(paged.k_pool.shape) == (5, Hkv, 16, D) and paged.k_pool.is_contiguous() == page_major
    start = torch.tensor([11, 14], dtype=torch.int32)              # batch 1 crosses into its second page at step 2
    dense.lengths.copy_(start)
    paged.lengths.copy_(start)
    consts = case["consts"]
    for t in range(T):
        want = C.gqa_decode_step(case, rot, core, dense, t)
        qt, kvt = case["q"][:, t:t + 1], case["kv"][:, t:t + 1]
        q, k, v = LevelsTensor(qt, *consts, 0, 255), LevelsTensor(kvt[:, :, 0], *consts, 0, 255), LevelsTensor(kvt[:, :, 1], *consts, 0, 255)
        rq = rot(q, positions=paged.lengths)
        kp, vp, lens = paged.append(k, v, rotary=rot)
        got = core(LevelsTensor(rq.levels.permute(0, 2, 1, 3), rq.scale, rq.zero_point, rq.quant_min, rq.quant_max), kp, vp, key_lengths=lens,
                   block_table=paged.block_table).levels
        assert torch.equal(got, want), t
        assert lens is paged.lengths and lens.tolist() == dense.lengths.tolist()
    from torchlsq.functional import lsq_kv_gather_paged_w8
    for pool, cache in ((kp, dense.k), (vp, dense.v)):
        g = lsq_kv_gather_paged_w8(pool, paged.block_table).levels
        for b in range(B):
            lo, hi = int(start[b]), int(start[b]) + T
            assert torch.equal(g[b, :, lo:hi], cache[b, :, lo:hi]) and not bool(g[b, :, hi:].any()) and not bool(g[b, :, :lo].any())
    assert not bool(paged.k_pool[4].any())                          # the page no table names
    paged.reset()
    assert paged.lengths.tolist() == [0, 0]
    # split as an int gives splits, "auto" the library's choice: the same bytes
    for split in (1, "auto"):
        core.split = split
        assert torch.equal(core(LevelsTensor(rq.levels.permute(0, 2, 1, 3), rq.scale, rq.zero_point, 0, 255), kp, vp,
                                key_lengths=dense.lengths, block_table=paged.block_table).levels, want)
    core.split, core.decode = None, False
    with pytest.raises(AssertionError, match="needs decode=True or prefill=True"):
        core(LevelsTensor(rq.levels.permute(0, 2, 1, 3), rq.scale, rq.zero_point, 0, 255), kp, vp, key_lengths=lens, block_table=paged.block_table)


def test_the_core_without_a_block_table_is_untouched(monkeypatch):
    """no block table: the paged functional is never reached, and the result is the one of the positional call"""
    import torchlsq.quantized.modules.attn_w8 as M
    from torchlsq.functional import LevelsTensor

    def boom(*a, **k):
        raise AssertionError("the paged functional was called without a block table")
    monkeypatch.setattr(M, "lsq_attention_decode_paged_w8_q", boom)
    case = C.gqa_decode_case()
    consts = case["consts"]
    q = LevelsTensor(case["q"].permute(0, 2, 1, 3), *consts, 0, 255)
    k, v = (LevelsTensor(case["kv"][:, :, i].permute(0, 2, 1, 3), *consts, 0, 255) for i in (0, 1))
    lens = torch.tensor([7, 4], dtype=torch.int32)
    for attrs in (dict(decode=True), dict(prefill=True), dict(decode=True, split=1)):
        core = copy.deepcopy(case["core"])
        for n, val in attrs.items():
            setattr(core, n, val)
        a, b = core(q, k, v, lens).levels, core(q, k, v, key_lengths=lens, block_table=None).levels
        assert torch.equal(a, b) and torch.equal(a, C.definition(_as_case(case, q, k, v, core, lens)))
    core = copy.deepcopy(case["core"])
    kk, vv = (C.with_levels(x, x.levels.repeat_interleave(2, dim=1)) for x in (k, v))
    assert torch.equal(core(q, kk, vv).levels, core(q, kk, vv, None, None).levels)


def _as_case(case, q, k, v, core, lens):
    c = C.Case()
    c.q, c.k, c.v, c.table, c.mid, c.causal, c.lengths = q, k, v, core.softmax.table, core.scores.mid_dtype, True, lens
    c.sides = (core.scores._out("output"), core.softmax._out("output"), core.context._out("output"))
    return c
