"""Chunked prefill attention on 8-bit levels without a GPU (include/lsq_hip_attn_chunk_w8.h): the tiled three launches emulated in int64
torch ops and held to the definition for the three mask modes, the plan and workspace functions, the refusals, the CPU path against
the parent's ops and against the per-entry construction of causal="lengths", chunked equals whole for the decoder layer, the
dispatch, the module's flag and the ABI table.  Every comparison is torch.equal.
"""
import copy
import ctypes
import os
import pickle
import re
import subprocess

import pytest
import torch

import attn_chunk_w8_cases as K
import attn_decode_w8_cases as C
import attn_paged_w8_cases as P
import attn_w8_cases as A
import decoder_w8_cases as L
from helpers import demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_attn_chunk_w8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_attn_chunk_w8.so")
NAMES = sorted(["lsq_attn_chunk_w8_abi_version", "lsq_attn_chunk_w8_last_error", "lsq_attn_chunk_w8", "lsq_attn_chunk_paged_w8",
                "lsq_attn_chunk_w8_plan", "lsq_attn_chunk_paged_w8_plan", "lsq_attn_chunk_w8_workspace", "lsq_attn_chunk_paged_w8_workspace"])
OPS = torch.ops.torchlsq
U8, I8, BF16 = A.U8, A.I8, A.BF16
Z3 = (A.QKV_Z,) * 3
SENTINEL = -(1 << 40)
NOTHING = dict(family="composition", grid=0, reduce_grid=0, threads=0, rows=0, tiles=0, chunk=0, splits=0, lds_bytes=0, store="elements",
               workspace_bytes=0)
STATE_KEYS = ["scores.output_scale", "scores.output_shift", "softmax.table", "softmax.output_scale", "softmax.output_shift",
              "context.output_scale", "context.output_shift"]


def test_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_attn_chunk\w*)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_ATTN_CHUNK_W8) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_"))) == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "hipMalloc", "Synchronize", "lsq_hip_", "lsq_group_", "lsq_attn_", "lsq_bmm_", "lsq_softmax_", "lsq_rope_"):
        assert other not in und, other
    assert E.attn_chunk_w8_library().lsq_attn_chunk_w8_abi_version() == E.ATTN_CHUNK_W8_ABI_VERSION == 1
    for name, value in (("ABI_VERSION", 1), ("CAUSAL_LENGTHS", 2), ("ROW_TILE", 16), ("MIN_CHUNK", 512), ("WG_PER_CU", 4), ("MAX_SPLITS", 64),
                        ("CUS", 256), ("MAX_TK", 65536)):
        assert int(re.search(r"#define LSQ_ATTN_CHUNK_W8_%s (\d+)" % name, raw).group(1)) == value, name
    # the argument lists are the split and the paged entries'
    assert E.C_ABI_ATTN_CHUNK_W8["lsq_attn_chunk_w8"] == E.C_ABI_ATTN_DECODE_SPLIT_W8["lsq_attn_decode_split_w8"]
    assert E.C_ABI_ATTN_CHUNK_W8["lsq_attn_chunk_paged_w8"] == E.C_ABI_ATTN_PAGED_W8["lsq_attn_paged_w8_decode"]


def test_the_kernels(tmp_path):
    """five kernels (launch 3 reads no key: one for both), no scratch, no atomics, LDS that does not scale with Tk or Tq"""
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    short = sorted(re.search(r"lsq::(\w+)\(", n).group(1) for n in names.values())
    assert short == ["attn_chunk_context_kernel", "attn_chunk_paged_context_kernel", "attn_chunk_paged_scores_kernel",
                     "attn_chunk_reduce_kernel", "attn_chunk_scores_kernel"], names
    for mangled, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0, "%s uses %d bytes of scratch" % (names[mangled], scratch)
        assert not any("atomic" in o for o in ops), names[mangled]
        if "reduce" not in names[mangled]:
            assert ops.count("v_mfma_i32_16x16x64_i8") >= 5 and "s_barrier" in ops, names[mangled]


# ---------------------------------------------------------------------------------------------------
# the plan and the workspace
# ---------------------------------------------------------------------------------------------------
def _auto_chunk(B, Hkv, R, Tk):
    """the split rule's constants, spelled out: the fewest splits s with B Hkv NT s >= 4 x 256, at most 64, the chunk at least 512 keys
    and without an upper bound"""
    tiles = B * Hkv * -(-R // 16)
    fewest = min(-(-4 * 256 // tiles), 64)
    return max(64 * -(-(-(-Tk // 64)) // fewest), 512)


@pytest.mark.parametrize("B,Hkv,G,Tq,Tk,D,splits", [(1, 1, 1, 17, 17, 16, 0), (1, 2, 3, 21, 40, 32, 1), (1, 8, 4, 512, 32768, 128, 0),
                                                    (4, 8, 4, 512, 4096, 128, 0), (1, 1, 1, 130, 130, 16, 3), (1, 1, 2, 70, 200, 32, 4),
                                                    (1, 1, 1, 17, 65536, 16, 0), (2, 2, 4, 1, 200, 32, 2), (1, 1, 1, 16, 65536, 16, 0)], ids=str)
def test_plan_formulas(B, Hkv, G, Tq, Tk, D, splits):
    from torchlsq import extension as E
    R, H = G * Tq, G * Hkv
    pl = E.attn_chunk_w8_plan(B, H, Hkv, Tq, Tk, D, splits)
    chunk = 64 * -(-(-(-Tk // 64)) // splits) if splits else _auto_chunk(B, Hkv, R, Tk)
    S, NT = -(-Tk // chunk), -(-R // 16)
    assert pl == dict(family="chunk", grid=B * Hkv * NT * S, reduce_grid=B * Hkv * NT, threads=256, rows=R, tiles=NT, chunk=chunk, splits=S,
                      lds_bytes=3840 + 160 * D, store="packets", workspace_bytes=B * Hkv * R * 16 * (-(-Tk // 16)) + 8 * B * Hkv * S * R * D)
    if Tk % 16 == 0 and Tk >= 16:
        ps = 16
        pg = E.attn_chunk_paged_w8_plan(B, H, Hkv, Tq, D, B * (Tk // ps) + 1, ps, Tk // ps, splits)
        assert pg == dict(pl, workspace_bytes=B * Hkv * R * Tk + 8 * B * Hkv * S * R * D)


def test_the_split_rule():
    from torchlsq import extension as E
    # one tile per head: 1024 workgroups asked for, at most 64 splits -> 65536 keys in chunks of 1024
    assert E.attn_chunk_w8_plan(1, 1, 1, 16, 65536, 16)["splits"] == 64
    # a real prompt chunk fills the part with its tiles: S = 1 and a chunk of the whole cache, beyond the decode library's 2048
    pl = E.attn_chunk_w8_plan(1, 32, 8, 512, 32768, 128)
    assert (pl["tiles"], pl["splits"], pl["chunk"], pl["grid"]) == (128, 1, 32768, 1024)
    # never below 512 keys a chunk: the floor the sweep gave (256 was the design's starting value)
    assert E.attn_chunk_w8_plan(1, 1, 1, 16, 1024, 16)["chunk"] == 512 and E.attn_chunk_w8_plan(1, 1, 1, 16, 1024, 16)["splits"] == 2
    assert E.attn_chunk_w8_plan(1, 1, 1, 17, 200, 16)["chunk"] == 512 and E.attn_chunk_w8_plan(1, 1, 1, 17, 200, 16)["splits"] == 1
    pl = E.attn_chunk_w8_plan(1, 32, 8, 16, 8192, 128)                         # 32 tile workgroups: 32 splits asked for, the floor gives 16
    assert (pl["tiles"], pl["chunk"], pl["splits"]) == (4, 512, 16)
    pl = E.attn_chunk_w8_plan(1, 32, 8, 16, 32768, 128)
    assert (pl["tiles"], pl["chunk"], pl["splits"]) == (4, 1024, 32)
    # 512 tiles: two splits
    assert E.attn_chunk_w8_plan(1, 32, 8, 256, 8192, 128)["splits"] == 2


def test_families_on_both_sides_of_each_bound():
    from torchlsq import extension as E
    ok = dict(B=1, H=4, Hkv=2, Tq=33, Tk=100, D=32)

    def fam(**kw):
        return E.attn_chunk_w8_plan(**dict(ok, **kw))["family"]
    assert fam() == "chunk" and fam(Tq=1) == "chunk" and fam(Tq=16) == "chunk" and fam(Tq=4096, Tk=8) == "chunk"     # any R >= 1
    assert fam(D=16) == "chunk" and fam(D=128) == "chunk" and fam(D=24) == "composition" and fam(D=144) == "composition" and fam(D=8) == "composition"
    assert fam(Tk=65536) == "chunk"
    with pytest.raises(RuntimeError, match="at most 65536 are served"):
        fam(Tk=65537)
    assert fam(qkv_aligned=False) == "composition" and fam(y_aligned=False) == "chunk"
    assert E.attn_chunk_w8_plan(**dict(ok, y_aligned=False))["store"] == "elements"
    assert fam(q_strides=(4 * 33 * 32 + 8, 33 * 32, 32)) == "composition" and fam(k_strides=(2 * 100 * 40, 100 * 40, 40)) == "composition"
    assert E.attn_chunk_w8_plan(**dict(ok, D=24)) == NOTHING
    pk = dict(B=1, H=4, Hkv=2, Tq=33, D=32, num_pages=9, page_size=16, max_pages=8)

    def pfam(**kw):
        return E.attn_chunk_paged_w8_plan(**dict(pk, **kw))["family"]
    assert pfam() == "chunk" and pfam(page_size=8) == "composition" and pfam(page_size=24) == "composition" and pfam(page_size=128) == "chunk"
    assert pfam(page_size=16, max_pages=4096) == "chunk"
    with pytest.raises(RuntimeError, match="at most 65536 are served"):
        pfam(page_size=16, max_pages=4097)
    # the grid: at most 2^24 - 1 = 4097 x 4095 workgroups is served (4097 kv heads of 4095 row tiles, one split), 2^24 is refused
    pl = E.attn_chunk_w8_plan(1, 4097, 4097, 16 * 4095, 64, 16, 1)
    assert pl["family"] == "chunk" and pl["grid"] == 2 ** 24 - 1 and pl["tiles"] == 4095
    assert E.attn_chunk_w8_plan(1, 1, 1, 16 * (2 ** 20 - 1) // 16, 64, 16, 1)["family"] == "chunk"
    with pytest.raises(RuntimeError, match="workgroups"):
        E.attn_chunk_w8_plan(16, 2 ** 16, 1, 2 ** 8, 64, 16, 1)


def test_new_refusals():
    from torchlsq import extension as E
    for plan, args in ((E.attn_chunk_w8_plan, (1, 2, 2, 8, 64, 16)), (E.attn_chunk_paged_w8_plan, (1, 2, 2, 8, 16, 5, 16, 4))):
        with pytest.raises(RuntimeError, match=r"causal = 2 counts every row's keys back from key_lengths and needs them \(has_lengths = 0\)"):
            plan(*args, causal="lengths", has_lengths=False)
        with pytest.raises(RuntimeError, match="causal = 2 takes no offset, causal_offset = 3 must be 0"):
            plan(*args, causal=2, causal_offset=3)
        for bad in (3, -1):
            with pytest.raises(RuntimeError, match=r"causal = %d must be 0 \(off\), 1 \(t \+ 1 \+ causal_offset keys\) or 2" % bad):
                plan(*args, causal=bad)
        with pytest.raises(RuntimeError, match=r"splits = 2 must be 0 \(the library's choice\) or 1 .. ceil\(Tk / 64\) = 1"):
            plan(*args, 2)
        with pytest.raises(RuntimeError, match="causal_offset = -1 must be at least 0"):
            plan(*args, causal=1, causal_offset=-1)
        assert plan(*args, causal="lengths")["family"] == "chunk"
    with pytest.raises(RuntimeError, match="every extent must be at least 1"):
        E.attn_chunk_paged_w8_plan(1, 2, 2, 8, 16, 5, 16, 0)
    # the C entries refuse before anything is enqueued (no GPU here): NULL buffers after a good geometry, a NULL geometry
    lib = E.attn_chunk_w8_library()
    assert lib.lsq_attn_chunk_w8(*([None] * 12), 0, 0, None) == -1 and b"NULL geometry" in lib.lsq_attn_chunk_w8_last_error()
    assert lib.lsq_attn_chunk_paged_w8(*([None] * 14), 0, 0, None) == -1 and b"NULL geometry" in lib.lsq_attn_chunk_w8_last_error()
    ws = ctypes.c_int64(-1)
    assert lib.lsq_attn_chunk_w8_workspace(None, 0, ctypes.byref(ws)) == -1 and ws.value == -1
    # the functional's and the op's own messages
    c = C.case(1, 1, 2, 5, 20, 16, 60, causal=True)
    with pytest.raises(AssertionError, match="needs them"):
        K.run(c, "cpu", "lengths")
    with pytest.raises(AssertionError, match="causal must be None, a bool, an offset >= 0 or \"lengths\""):
        K.run(c, "cpu", "diagonal")
    args = C.flat_args(c, "cpu")
    with pytest.raises(RuntimeError, match="causal must be the int 0"):
        OPS.lsq_attention_chunk_w8_q8_q(*args[:-3], 3, 0, None)
    with pytest.raises(RuntimeError, match="causal = 2 takes no offset"):
        OPS.lsq_attention_chunk_w8_q8_q(*args[:-3], 2, 4, torch.tensor([7], dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------
# the tiled three launches in int64 torch ops
# ---------------------------------------------------------------------------------------------------
def _levels(u, side):
    lv = OPS.lsq_levels_per_tensor(u.contiguous(), *side, 0)
    return lv.view(I8 if max(side[3], side[5]) <= 127 else U8).to(torch.int64)


def _emulate(c, causal, lengths, chunk):
    """the tiled launches as the kernels make them -> (the levels [B, Tq, H D], the skipped (tile, chunk) pairs).  Both workspaces
    start as a sentinel; every read asserts that it meets none.  Per workgroup ((b, kv head), tile, split): the score bytes of the
    tile's rows for the chunk's keys below nmax_tile; then m and S of every row over its whole prefix and the chunk's I_c with the
    chunk's own key count; then the sum over the chunks that start below nmax_tile."""
    from torchlsq.functional import _act_constants
    B, H, Hkv, Tq, Tk, D = c.shape
    G, S, R = c.G, -(-Tk // chunk), c.G * Tq
    NT = -(-R // 16)
    i64, f32 = torch.int64, torch.float32
    n = K.key_counts(c, causal, lengths)
    zq, zk, zv = (int(x.zero_point) for x in (c.q, c.k, c.v))
    sq, sk, sv = (x.scale.to(f32) for x in (c.q, c.k, c.v))
    p_s, p_z = _act_constants(c.sides[1][0], c.sides[1][1], c.sides[1][4], c.sides[1][5])
    zp = int(p_z)
    q = (c.q.levels.to(i64) - zq).reshape(B, Hkv, R, D)                       # row r = g Tq + t of kv head hkv
    k = c.k.levels.to(i64) - zk
    v = c.v.levels.to(i64)
    tab = c.table.to(i64)
    ws = torch.full((B, Hkv, R, Tk), SENTINEL, dtype=i64)
    wi = torch.full((B, Hkv, S, R, D), SENTINEL, dtype=i64)
    total = torch.zeros((B, Hkv, R, D), dtype=i64)
    skipped = []

    def tile_of(b, tile):
        row0 = 16 * tile
        last = min(row0 + 16, R) - 1
        nrow = [n[b][r % Tq] for r in range(row0, last + 1)]
        nmax = n[b][Tq - 1] if row0 // Tq != last // Tq else n[b][last % Tq]
        assert nmax == max(nrow), "nmax_tile is the largest n of the tile's live rows"
        return row0, last, nrow, nmax
    for b in range(B):
        for h in range(Hkv):
            for tile in range(NT):
                row0, last, nrow, nmax = tile_of(b, tile)
                for s in range(S):                                         # launch 1
                    c0, c1 = s * chunk, min((s + 1) * chunk, nmax)
                    if c0 >= nmax:
                        skipped.append((tile, s))
                        continue
                    I = q[b, h, row0:last + 1] @ k[b, h, c0:c1].t()
                    ws[b, h, row0:last + 1, c0:c1] = _levels(((sk * I.to(f32)) * sq).to(c.mid), c.sides[0])
    for b in range(B):
        for h in range(Hkv):
            for tile in range(NT):
                row0, last, nrow, nmax = tile_of(b, tile)
                for s in range(S):                                         # launch 2
                    c0, c1 = s * chunk, min((s + 1) * chunk, nmax)
                    if c0 >= nmax:
                        continue
                    p = torch.full((last + 1 - row0, c1 - c0), zp, dtype=i64)       # the byte z_p from n_r on
                    for i, nr in enumerate(nrow):
                        if nr == 0:
                            continue
                        row = ws[b, h, row0 + i, :nr]
                        assert bool((row != SENTINEL).all()), "a row's prefix reads a score nobody wrote"
                        E = tab[row.max() - row]
                        rcp = 1.0 / E.sum().to(f32)
                        if nr > c0:
                            p[i, :min(nr, c1) - c0] = _levels((E[c0:min(nr, c1)].to(f32) * rcp).to(c.mid), c.sides[1])
                    vc = v[b, h, c0:c1]
                    wi[b, h, s, row0:last + 1] = p @ vc - zp * vc.sum(0, keepdim=True) - zv * p.sum(1, keepdim=True) + (c1 - c0) * zp * zv
    for b in range(B):
        for h in range(Hkv):
            for tile in range(NT):
                row0, last, nrow, nmax = tile_of(b, tile)
                part = wi[b, h, :-(-nmax // chunk), row0:last + 1]          # launch 3: the chunks that start below nmax_tile
                assert bool((part != SENTINEL).all()), "launch 3 reads an integer nobody wrote"
                total[b, h, row0:last + 1] = part.sum(0)
    u = ((sv * total.to(f32)) * p_s.to(f32)).to(c.mid)
    return _levels(u, c.sides[2]).reshape(B, H, Tq, D).permute(0, 2, 1, 3).reshape(B, Tq, H * D), skipped


EMULATED = [((1, 2, 3, 21, 40, 32), 64, 19, None), ((1, 1, 1, 130, 130, 16), 64, True, None), ((1, 1, 2, 70, 200, 32), 64, 130, None),
            ((2, 1, 2, 20, 200, 32), 128, False, (129, 64)), ((3, 1, 2, 20, 200, 32), 64, "lengths", (200, 70, 9)),
            ((2, 1, 2, 20, 200, 32), 128, "lengths", (0, -4))]


@pytest.mark.parametrize("shape,chunk,causal,lengths", EMULATED, ids=str)
def test_the_tiled_launches_in_integers_equal_the_definition(shape, chunk, causal, lengths):
    """tiles that straddle a head border (Tq 21, 70, 20 are no multiples of 16), a partial last tile, rows with n = 0"""
    lengths_mode = causal == "lengths"
    c = C.case(*shape, 61, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True if lengths_mode else causal, None if lengths_mode else lengths)
    C.check_not_degenerate(c)
    want = K.want_lengths(c, lengths) if lengths_mode else c.want
    got, skipped = _emulate(c, causal, lengths, chunk)
    assert torch.equal(got, want.to(torch.int64))
    assert torch.equal(_emulate(c, causal, lengths, 256)[0], got)               # the chunk does not move a byte
    B, H, Hkv, Tq, Tk, D = shape[0], shape[1] * shape[2], shape[1], shape[3], shape[4], shape[5]
    assert (c.G * Tq) % 16 != 0 and (Tq % 16 != 0 or c.G == 1)
    if shape == (1, 1, 1, 130, 130, 16):
        # tile 0 (rows 0 .. 15) needs chunk 0 only, the tile of rows 64 .. 79 chunks 0 and 1, the last tile all three
        assert (0, 1) in skipped and (0, 2) in skipped and (4, 1) not in skipped and (4, 2) in skipped and (8, 2) not in skipped
    if lengths_mode and min(lengths) < Tq:
        assert bool((want[lengths.index(min(lengths)), 0] == K.level_of_zero(c)).all())


# ---------------------------------------------------------------------------------------------------
# the CPU path
# ---------------------------------------------------------------------------------------------------
OLD = [((2, 2, 3, 21, 40, 32), 19, None), ((2, 2, 3, 21, 40, 32), True, (40, 25)), ((2, 1, 2, 20, 64, 32), False, (33, 0)),
       ((1, 1, 16, 2, 65, 64), True, None), ((2, 2, 4, 1, 200, 32), True, (200, 129))]


@pytest.mark.parametrize("shape,causal,lengths", OLD, ids=str)
def test_cpu_path_equals_the_parent_ops_for_the_old_masks(shape, causal, lengths):
    c = C.case(*shape, 62, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, causal, lengths)
    C.check_not_degenerate(c)
    assert torch.equal(K.run(c, "cpu"), c.want) and torch.equal(K.run(c, "cpu", splits=1), c.want)
    mode, off = K.mode_args(c, causal)
    assert torch.equal(OPS.lsq_attention_chunk_w8_q8_q(*C.flat_args(c, "cpu")[:-3], mode, off, c.lengths, 0), c.want)
    B, H, Hkv, Tq, Tk, D = c.shape
    if Tk % 8 == 0:
        for ps in (8, 16) if Tk % 16 == 0 else (8,):
            pg = P.paged(c, ps, order="shd" if ps == 8 else "hsd", bt_pad=1)
            assert torch.equal(K.run(c, "cpu", pg=pg), c.want)
            assert torch.equal(K.run(c, "cpu", pg=pg), P.run(c, pg, "cpu"))


def test_cpu_path_of_lengths_equals_the_construction():
    lengths = (-3, 0, 1, 15, 16, 17, 21, 39, 40, 45)
    c = C.case(10, 1, 2, 21, 40, 32, 63, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, None)
    want = K.want_lengths(c, lengths)
    assert len(want.unique()) > 16 and not torch.equal(want, c.want)
    assert torch.equal(K.run(c, "cpu", "lengths", lengths=lengths), want)
    assert torch.equal(want[8], c.want[8]) and torch.equal(want[9], c.want[9])          # a full cache: causal=True
    pg = P.paged(c, 8, bt_pad=2)
    assert torch.equal(K.run(c, "cpu", "lengths", pg=pg, lengths=lengths), want)
    # Tq = 1: causal=True with key_lengths
    d = C.case(2, 2, 4, 1, 200, 32, 52, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (200, 129))
    assert torch.equal(K.run(d, "cpu", "lengths"), d.want)


@pytest.mark.parametrize("route", ["dense", "paged"])
def test_chunked_equals_whole_for_the_decoder_layer(route):
    """the `long` case, 67 tokens, fed as one prompt, in pieces and token by token through one module instance with chunk=True and
    causal="lengths": the parent's whole-prompt run at every stage and on both cache sides"""
    want = L.cpu_run("long", BF16, "whole")
    assert L.total(L.CASES["long"]) == 67
    for how, chunks in K.CHUNKINGS.items():
        assert sum(chunks) == 67
        got = K.layer_sequence(K.chunk_layer("long", BF16), L.input_levels("long"), L.make_cache("long", route), chunks)
        assert L.differing(got, want) == [], (route, how, L.differing(got, want))


# ---------------------------------------------------------------------------------------------------
# the wiring: the dispatch, the module
# ---------------------------------------------------------------------------------------------------
def _core(D, **kw):
    from torchlsq.quantized import AttentionCoreW8Q
    span = 6.0 * A.QKV_S * A.QKV_S * 74 * 74 * D ** 0.5
    return AttentionCoreW8Q(A.trained(-span, span), A.trained(0.0, 1.0), A.trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16, **kw)


def test_dispatch_order_with_a_faked_device(monkeypatch):
    """checks -> plan -> (GPU and "chunk": one torch.empty, one ctypes call) | the composition; never both, never a silent fallback"""
    import torchlsq._attn_chunk_w8_host as Hh
    c = C.case(1, 1, 2, 20, 64, 32, 64, causal=True)
    events = []
    real_checked, real_plan, real_compose = Hh._dec._checked, Hh._plan_call, Hh._compose

    def checked(*a, **kw):
        events.append("checks")
        st = real_checked(*a, **kw)
        st.on_gpu = fake_gpu[0]
        return st

    def plan(*a, **kw):
        events.append("plan")
        return dict(real_plan(*a, **kw), family=family[0])

    def compose(*a, **kw):
        events.append("compose")
        return real_compose(*a, **kw)

    def on_device(idx, fn, *a):
        events.append("entry")
        return 0
    fake_gpu, family = [False], ["chunk"]
    monkeypatch.setattr(Hh._dec, "_checked", checked)
    monkeypatch.setattr(Hh, "_plan_call", plan)
    monkeypatch.setattr(Hh, "_compose", compose)
    monkeypatch.setattr(Hh, "_on_device", on_device)
    monkeypatch.setattr(Hh, "_stream_of", lambda idx: None)
    monkeypatch.setattr(Hh._dec, "_aligned", lambda *ts: 1)
    real_empty = torch.empty

    def empty(*a, **kw):
        if kw.get("dtype") == torch.uint8 and len(a) == 1 and isinstance(a[0], int):
            events.append("workspace %d" % a[0])
        return real_empty(*a, **kw)
    monkeypatch.setattr(Hh.torch, "empty", empty)
    assert torch.equal(K.run(c, "cpu"), c.want) and events == ["checks", "plan", "compose"]
    del events[:]
    need = K.plan_of(c)["workspace_bytes"]
    del events[:]
    fake_gpu[0] = True
    K.run(c, "cpu")
    assert events == ["checks", "plan", "workspace %d" % need, "entry"]
    del events[:]
    family[0] = "composition"
    K.run(c, "cpu")
    assert events == ["checks", "plan", "compose"]


def test_module_chunk_attribute(monkeypatch):
    import torchlsq.quantized.modules.attn_w8 as W
    from torchlsq.quantized import AttentionCoreW8Q
    calls = []
    real = W.lsq_attention_chunk_w8_q

    def spy(*a, **kw):
        calls.append((kw.get("causal"), kw.get("splits"), kw.get("block_table") is not None))
        return real(*a, **kw)
    monkeypatch.setattr(W, "lsq_attention_chunk_w8_q", spy)
    c = C.case(2, 2, 3, 21, 48, 32, 65, causal=True, lengths=(48, 30))
    pre, chk = _core(32, causal=True, prefill=True), _core(32, causal=True, prefill=True, chunk=True, split=2)
    assert AttentionCoreW8Q.chunk is False and pre.chunk is False and chk.chunk is True
    assert list(pre.state_dict()) == list(chk.state_dict()) == STATE_KEYS
    want = pre(c.q, c.k, c.v, key_lengths=c.lengths).levels
    assert calls == [] and len(want.unique()) > 16
    assert torch.equal(chk(c.q, c.k, c.v, key_lengths=c.lengths).levels, want) and calls == [(True, 2, False)]
    pg = P.paged(c, 16)
    del calls[:]
    assert torch.equal(chk(c.q, pg.k_pool, pg.v_pool, key_lengths=c.lengths, block_table=pg.table).levels, want) and calls == [(True, 2, True)]
    for clone in (copy.deepcopy(chk), pickle.loads(pickle.dumps(chk))):
        assert clone.chunk is True and torch.equal(clone(c.q, c.k, c.v, key_lengths=c.lengths).levels, want)
    # a module pickled before the attribute existed reads the class default and goes where it went
    old = copy.deepcopy(chk)
    del old.__dict__["chunk"]
    old = pickle.loads(pickle.dumps(old))
    del calls[:]
    assert "chunk" not in old.__dict__ and old.chunk is False and torch.equal(old(c.q, c.k, c.v, key_lengths=c.lengths).levels, want)
    assert calls == []
    # chunk=False: the repr is the parent's, word for word; "lengths" needs chunk=True
    assert repr(pre) == repr(_core(32, causal=True, prefill=True)) and "chunk" not in repr(pre) and "chunk" not in repr(_core(32))
    assert "chunk=True" in repr(chk) and "splits=2" in repr(chk)
    pre.causal = "lengths"
    with pytest.raises(AssertionError, match="causal='lengths' .* needs chunk=True"):
        pre(c.q, c.k, c.v, key_lengths=c.lengths)
    chk.causal, chk.split = "lengths", "auto"
    del calls[:]
    lens = (40, 9)
    got = chk(c.q, c.k, c.v, key_lengths=C.lens_tensor(lens)).levels
    assert torch.equal(got, K.want_lengths(c, lens)) and calls == [("lengths", 0, False)]
