"""Split-key decode attention on 8-bit levels on the GPU (liblsq_hip_attn_decode_split_w8.so): bit for bit against the op's CPU path
(`attn_decode_w8_cases.definition`; tests/test_attn_decode_split_w8_cpu.py holds the three launches' algebra to it in integers), at the
smallest shapes at which each mechanism of the three kernels can fail.  Before every comparison the plan's family and the forced
split count are asserted, and beside the op the library's C entry is called directly with a workspace the test made -- no Python host,
no fallback --: status 0 and the same bytes are the split kernels' own, EINVAL with y's 0x5A guard bytes untouched means
"composition".  Every comparison is torch.equal; the softmax tables are built once on the CPU and moved.
"""
import copy
import ctypes

import pytest
import torch

import attn_decode_w8_cases as C
import attn_w8_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
GUARD = C.GUARD
LSQ_EINVAL = -1
Z3 = (A.QKV_Z,) * 3
SIGNED_PV = (True, False, False)       # fitted int8 probabilities and context: many keys leave a quint8 probability few levels
LENGTHS = (-3, 0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 199, 200, 205)


def plan_of(c, splits, qkv_aligned=True, y_aligned=True):
    from torchlsq import extension as E
    B, H, Hkv, Tq, Tk, D = c.shape
    on, off = C.causal_args(c)
    return E.attn_decode_split_w8_plan(B, H, Hkv, Tq, Tk, D, splits, q_strides=C.F.strides(c.q.levels), k_strides=C.F.strides(c.k.levels),
                                       v_strides=C.F.strides(c.v.levels), qkv_aligned=qkv_aligned, y_aligned=y_aligned,
                                       q_dtype=c.q.levels.dtype, k_dtype=c.k.levels.dtype, v_dtype=c.v.levels.dtype, causal=on,
                                       causal_offset=off, has_lengths=c.lengths is not None)


def run(c, split, shift=(0, 0, 0), k=None, v=None):
    """`lsq_attention_decode_w8_q(..., split=split)` of the case on the GPU -> the levels [B, Tq, H D]"""
    from torchlsq.functional import lsq_attention_decode_w8_q
    q, k, v = (C.moved(x, DEV, sh) for x, sh in zip((c.q, c.k if k is None else k, c.v if v is None else v), shift))
    return lsq_attention_decode_w8_q(q, k, v, c.table.to(DEV), *C.F.sides_on(c.sides, DEV), c.mid, causal=c.causal,
                                     key_lengths=None if c.lengths is None else c.lengths.to(DEV), split=split).levels


def workspace(c, splits, fill):
    """(the workspace tensor: the reported bytes filled with `fill` and 64 guard bytes behind them, the reported size)"""
    need = plan_of(c, splits)["workspace_bytes"]
    ws = torch.full((need + 64,), fill, dtype=U8, device=DEV)
    ws[need:] = GUARD
    assert ws.data_ptr() % 16 == 0
    return ws, need


def c_entry(c, splits, shift=(0, 0, 0), ws=None, fill=0xA5, y_shift=0):
    """`lsq_attn_decode_split_w8` called directly on the case's operands on the GPU with a caller-made workspace -> (status, the levels
    [B, Tq, H D] prefilled with 0x5A, the workspace, its reported size)"""
    from torchlsq import extension as E
    from torchlsq._attn_w8_host import _DTYPE_CODE, _LEVEL_CODE
    from torchlsq.functional import _act_constants
    B, H, Hkv, Tq, Tk, D = c.shape
    q, k, v = (C.moved(x, DEV, sh) for x, sh in zip((c.q, c.k, c.v), shift))
    sides, tab = C.F.sides_on(c.sides, DEV), c.table.to(DEV)
    lens = None if c.lengths is None else c.lengths.to(DEV)
    raw = torch.full((B * Tq * H * D + 32,), GUARD, dtype=U8, device=DEV)
    y = raw[y_shift:y_shift + B * Tq * H * D].view(B, Tq, H * D).view(c.want.dtype)
    guard_from = None                                   # a workspace the caller made: the caller checks its guard bytes
    if ws is None:
        ws, need = workspace(c, splits, fill)
        guard_from = need
    else:
        need = plan_of(c, splits)["workspace_bytes"]
    S = E.LsqAttnW8Strides
    on, off = C.causal_args(c)
    geom = E.LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, *(_LEVEL_CODE[x.levels.dtype] for x in (q, k, v)), 1 if on else 0, off,
                                 0 if lens is None else 1, *(S(*C.F.strides(x.levels)) for x in (q, k, v)),
                                 S(*C.F.strides(y.view(B, Tq, H, D).permute(0, 2, 1, 3))))
    p_s, p_z = _act_constants(sides[1][0], sides[1][1], sides[1][4], sides[1][5])
    consts = E.LsqAttnDecodeW8Consts(q.scale.data_ptr(), q.zero_point.data_ptr(), k.scale.data_ptr(), k.zero_point.data_ptr(),
                                     v.scale.data_ptr(), v.zero_point.data_ptr(), p_s.data_ptr(), p_z.data_ptr())
    outs = [E.LsqAttnW8Out(s[0].data_ptr(), s[1].data_ptr(), *s[2:], _DTYPE_CODE[c.mid]) for s in sides]
    torch.cuda.synchronize()                            # the call below goes to the default stream
    rc = E.attn_decode_split_w8_library().lsq_attn_decode_split_w8(
        ctypes.byref(geom), ctypes.byref(consts), *(ctypes.byref(o) for o in outs), tab.data_ptr(), None if lens is None else lens.data_ptr(),
        q.levels.data_ptr(), k.levels.data_ptr(), v.levels.data_ptr(), y.data_ptr(), ws.data_ptr(), need, splits, None)
    torch.cuda.synchronize()
    assert bool((raw[:y_shift] == GUARD).all()) and bool((raw[y_shift + B * Tq * H * D:] == GUARD).all()), "bytes outside y were written"
    assert guard_from is None or bool((ws[guard_from:] == GUARD).all()), "bytes behind the reported workspace were written"
    return rc, y, ws, need


def _equals_cpu(c, splits, note="", family="split", shift=(0, 0, 0), split=None):
    """`splits`: what the C entry and the plan get (0: the library's choice); `split`: what the functional gets (default: `splits`,
    "auto" for 0)"""
    pl = plan_of(c, splits, qkv_aligned=not any(shift))
    assert pl["family"] == family, (note, pl)
    if family == "split" and splits:
        assert pl["splits"] == splits and pl["grid"] == c.shape[0] * c.shape[2] * splits, (note, pl)
    C.check_not_degenerate(c)
    got = run(c, ("auto" if splits == 0 else splits) if split is None else split, shift)
    assert got.shape == c.want.shape and got.dtype == c.want.dtype, note
    assert torch.equal(got.cpu(), c.want), note
    rc, y, _, _ = c_entry(c, splits, shift)
    if family == "split":
        assert rc == 0 and torch.equal(y.cpu(), c.want), (note, rc)
    else:
        assert rc == LSQ_EINVAL and bool((y.view(U8) == GUARD).all()), (note, rc)
    return pl


# (B, Hkv, G, Tq, Tk, D), splits, key_lengths: a last chunk of 2 keys; a full row tile and a last chunk of one key; two batches and kv
# heads with a short batch; five column sub-tiles and a third partial sub-tile group; two query rows per head at D 128; 1024 keys in
# one chunk (four rounds of launch 1), in four and in sixteen
BORDERS = [((1, 1, 1, 1, 130, 16), 3, None), ((1, 1, 16, 1, 65, 64), 2, None), ((2, 2, 4, 1, 200, 32), 2, (200, 130)),
           ((2, 2, 4, 1, 200, 32), 4, (200, 130)), ((1, 1, 2, 1, 130, 80), 3, None), ((1, 1, 8, 2, 197, 128), 4, (150,)),
           ((1, 1, 4, 1, 1024, 64), 1, (1000,)), ((1, 1, 4, 1, 1024, 64), 4, (1000,)), ((1, 1, 4, 1, 1024, 64), 16, (1000,))]


@pytest.mark.parametrize("shape,splits,lengths", BORDERS, ids=str)
def test_chunk_borders(shape, splits, lengths):
    B, Hkv, G, Tq, Tk, D = shape
    for dtypes, unsigned in C.COMBOS if Tk < 1024 else ((C.ALL_U8, SIGNED_PV),):
        pl = _equals_cpu(C.case(*shape, 0, dtypes, unsigned, BF16, Z3, None, True, lengths), splits, (shape, splits))
        assert pl["reduce_grid"] == B * Hkv and pl["rows"] == G * Tq and pl["threads"] == 256 and pl["lds_bytes"] == 3840 + 160 * D
        assert pl["chunk"] % 64 == 0 and (splits - 1) * pl["chunk"] < Tk <= splits * pl["chunk"]


def test_rows_with_different_counts_across_a_chunk_border():
    """R 15, causal offset 125 over chunks of 64: the rows of t = 0, 1, 2 end at 126, 127, 128 keys inside the second chunk, those of
    t = 3, 4 at 129, 130 inside the third, and the fourth chunk starts beyond nmax"""
    c = C.case(1, 2, 3, 5, 197, 32, 1, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, 125, None)
    assert C.key_counts(1, 5, 197, 125, None) == [[126, 127, 128, 129, 130]]
    _equals_cpu(c, 4, "offset 125")
    # key_lengths cut the later rows: 126, 127, 127, 127, 127
    _equals_cpu(C.case(1, 2, 3, 5, 197, 32, 1, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, 125, (127,)), 4, "offset 125, 127 keys")
    _equals_cpu(C.case(1, 2, 3, 5, 197, 32, 1, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, None), 2, "causal=True, chunks of 128")


def test_key_counts_in_one_call():
    """B = 15, Tk = 200 over four chunks of 64: chunks wholly beyond nmax, n = 0, and a count on both sides of every chunk border"""
    c = C.case(15, 1, 2, 1, 200, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, LENGTHS)
    zero = c.want[1, 0, 0]
    assert bool((c.want[0] == zero).all()) and bool((c.want[1] == zero).all()) and len(c.want[2:].unique()) > 16
    _equals_cpu(c, 4, "lengths")
    _equals_cpu(C.case(15, 1, 2, 2, 200, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, LENGTHS), 4, "lengths, Tq 2")
    _equals_cpu(C.case(15, 1, 2, 2, 200, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, 5, LENGTHS), 4, "lengths, Tq 2, offset 5")


def _max_in_chunk(Tk, where, table, unsigned):
    """Hkv 2, one query row per kv head: the key that carries the row's largest score byte swapped to the LAST (or FIRST) slot, so
    that the chunk that holds the maximum is not the one most keys lie in"""
    from torchlsq.functional import lsq_bmm_w8_q
    c = C.Case()
    c.shape, c.G, c.mid, c.causal, c.lengths = (1, 2, 2, 1, Tk, 64), 1, BF16, True, None
    c.q, c.k, c.v = C.inputs(1, 2, 1, 1, Tk, 64, 3)
    given = {None: None, "full": A.full_table()}[table]
    c.table, c.sides = C.F.fitted_sides(c.q, c.k, c.v, unsigned, BF16, given)
    s = lsq_bmm_w8_q(c.q, c.k, True, *c.sides[0], BF16).levels.to(torch.int64)          # [1, 2, 1, Tk]
    to = Tk - 1 if where == "last" else 0
    for h in range(2):
        top = int(s[0, h, 0].argmax())
        for x in (c.k, c.v):
            x.levels[0, h, [top, to]] = x.levels[0, h, [to, top]]
    s = lsq_bmm_w8_q(c.q, c.k, True, *c.sides[0], BF16).levels.to(torch.int64)
    chunk = Tk // 4
    mine = slice(Tk - chunk, Tk) if where == "last" else slice(0, chunk)
    rest = slice(0, Tk - chunk) if where == "last" else slice(chunk, Tk)
    assert bool((s[0, :, 0, mine].max(dim=-1).values >= s[0, :, 0, rest].max(dim=-1).values).all())
    assert bool((s[0, :, 0, to] == s[0, :, 0].max(dim=-1).values).all())
    return C.finish(c)


@pytest.mark.parametrize("where", ["last", "first"])
def test_the_maximum_in_another_chunk(where):
    _equals_cpu(_max_in_chunk(256, where, None, C.ALL_UNSIGNED), 4, where)
    # every table entry 2^24: S = 2^32 at 256 keys and 2^34 at 1024, summed over the whole prefix by every split
    for Tk in (256, 1024):
        c = _max_in_chunk(Tk, where, "full", SIGNED_PV)
        assert len(c.want.unique()) > 16
        _equals_cpu(c, 4, ("full table", Tk, where))


def test_the_result_does_not_depend_on_the_workspace():
    c = C.case(2, 2, 4, 1, 200, 32, 4, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (200, 70))
    for fill in (0x00, 0xFF):
        rc, y, ws, need = c_entry(c, 4, fill=fill)
        assert rc == 0 and torch.equal(y.cpu(), c.want), fill
        assert need == 2 * 2 * 4 * 208 + 8 * 2 * 2 * 4 * 4 * 32
    # a long call fills the workspace, shorter ones (n = 0 among them) run in the same bytes
    long = C.case(1, 1, 16, 1, 1024, 64, 4, C.ALL_U8, SIGNED_PV)
    rc, y, ws, need = c_entry(long, 16)
    assert rc == 0 and torch.equal(y.cpu(), long.want)
    for shape, splits, lengths in (((1, 1, 3, 1, 197, 64), 4, (100,)), ((1, 1, 16, 1, 130, 64), 3, (0,)), ((1, 1, 1, 1, 65, 64), 2, (64,)),
                                   ((1, 1, 16, 1, 1024, 64), 4, (3,))):
        d = C.case(*shape, 4, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, lengths)
        assert plan_of(d, splits)["workspace_bytes"] <= need
        rc, y, _, _ = c_entry(d, splits, ws=ws)
        assert rc == 0 and torch.equal(y.cpu(), d.want), shape
    assert bool((ws[need:] == GUARD).all())


def test_poisoned_slots_do_not_reach_the_result():
    """every slot at or beyond the batch's key count holds 0xFF: the same bytes.  k and v are dense buffers, so the last packet of
    the last row ends with the storage"""
    c = C.case(15, 1, 2, 1, 200, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, LENGTHS)
    k, v = C.poisoned(c, 0xFF)
    assert bool((k.levels[3, :, 15:] == 0xFF).all()) and torch.equal(k.levels[13], c.k.levels[13])
    assert torch.equal(C.definition(c, k=k, v=v), c.want)
    assert torch.equal(run(c, 4, k=k, v=v).cpu(), c.want)
    # the probabilities quantizer with quant_min = 5: its level of 0.0 is not its z_p, and still nothing beyond n is read
    d = C.Case()
    d.shape, d.G, d.mid, d.causal, d.lengths, d.table = c.shape, c.G, c.mid, c.causal, c.lengths, c.table
    d.q, d.k, d.v = c.q, c.k, c.v
    p = c.sides[1]
    d.sides = (c.sides[0], (p[0], p[1], 5) + tuple(p[3:]), c.sides[2])
    C.finish(d)
    assert not torch.equal(d.want, c.want)
    _equals_cpu(d, 4, "quant_min 5")
    assert torch.equal(run(d, 4, k=k, v=v).cpu(), d.want)


@pytest.mark.parametrize("mid", A.MIDS, ids=str)
def test_dtypes(mid):
    shape = (2, 2, 4, 1, 200, 32)
    for dtypes, unsigned in C.COMBOS + (((U8, U8, I8), (False, False, True)),):
        _equals_cpu(C.case(*shape, 5, dtypes, unsigned, mid, Z3, None, True, (200, 131)), 4, (dtypes, unsigned, mid))


def test_zero_points_far_from_the_middle():
    for dtypes in (C.ALL_U8, (I8, I8, I8), (U8, I8, U8)):
        _equals_cpu(C.case(2, 2, 4, 1, 200, 32, 6, dtypes, C.ALL_UNSIGNED, BF16, (3, 140, 250), None, True, (190, 66)), 4, dtypes)


@pytest.mark.parametrize("shape", [(1, 1, 2, 1, 8193, 32), (1, 1, 4, 1, 16384, 128), (1, 1, 1, 1, 65536, 16)], ids=str)
def test_beyond_the_single_launch_kernel(shape):
    """Tk > 8192: the decode plan says "composition", `split="auto"` takes the split family with the library's own chunk"""
    from torchlsq import extension as E
    B, Hkv, G, Tq, Tk, D = shape
    c = C.case(*shape, 7, C.ALL_U8, SIGNED_PV, BF16, Z3, None, True, (Tk - 3,))
    assert C.plan_of(c)["family"] == "composition"
    assert E.attn_decode_split_w8_plan(B, Hkv * G, Hkv, Tq, Tk, D, "auto", causal=True, causal_offset=Tk - Tq)["family"] == "split"
    pl = _equals_cpu(c, 0, shape)
    chunk = max(256, Tk // 64)                          # at most 64 splits
    assert pl["chunk"] == chunk and pl["splits"] == -(-Tk // chunk)


def test_stores_and_misaligned_operands():
    from torchlsq import extension as E
    c = C.case(2, 2, 3, 5, 197, 32, 8, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (197, 110))
    B, H, Hkv, T, Tk, D = c.shape
    # a y one byte off: still the split kernels, with the byte store -- through the C entry and through the host's `out`
    pl = plan_of(c, 4, y_aligned=False)
    assert pl["family"] == "split" and pl["store"] == "elements" and plan_of(c, 4)["store"] == "packets"
    rc, y, _, _ = c_entry(c, 4, y_shift=1)
    assert rc == 0 and y.data_ptr() % 16 == 1 and torch.equal(y.cpu(), c.want)
    raw = torch.full((B * T * H * D + 2,), GUARD, dtype=U8, device=DEV)
    yv = raw[1:-1].view(B, T, H, D).permute(0, 2, 1, 3)
    E.attn_decode_split_w8_q(*C.flat_args(c, DEV), splits=4, out=yv)
    assert torch.equal(raw[1:-1].view(B, T, H * D).cpu(), c.want) and int(raw[0]) == GUARD and int(raw[-1]) == GUARD
    # a q one byte off, a k one byte off: the composition, the same bytes
    _equals_cpu(c, 4, "q one byte off", "composition", (1, 0, 0))
    _equals_cpu(c, 4, "k one byte off", "composition", (0, 1, 0))
    # R 17: legal, not served
    _equals_cpu(C.case(1, 1, 17, 1, 130, 32, 8, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (127,)), 3, "R 17", "composition")


def test_launches_repeat_and_batches_depend_on_their_own_inputs_alone():
    from torchlsq.functional import lsq_attention_decode_w8_q
    c = C.case(3, 2, 4, 1, 197, 64, 11, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (197, 60, 133))
    first, second = run(c, 4), run(c, 4)
    assert torch.equal(first, second) and torch.equal(first.cpu(), c.want)
    assert torch.equal(run(c, 1), first) and torch.equal(run(c, 2), first) and torch.equal(run(c, None), first)
    sides, tab = C.F.sides_on(c.sides, DEV), c.table.to(DEV)
    for b in range(3):
        q, k, v = (C.with_levels(x, x.levels[b:b + 1]) for x in (C.moved(c.q, DEV), C.moved(c.k, DEV), C.moved(c.v, DEV)))
        one = lsq_attention_decode_w8_q(q, k, v, tab, *sides, c.mid, causal=True, key_lengths=c.lengths[b:b + 1].to(DEV), split=4).levels
        assert torch.equal(one[0], first[b]), b
    # one kv head alone: its G query heads' columns
    h, D, G = 1, 64, 4
    q, k, v = (C.with_levels(x, f(x.levels)) for x, f in ((C.moved(c.q, DEV), lambda t: t[:, h * G:(h + 1) * G]),
                                                         (C.moved(c.k, DEV), lambda t: t[:, h:h + 1]), (C.moved(c.v, DEV), lambda t: t[:, h:h + 1])))
    one = lsq_attention_decode_w8_q(q, k, v, tab, *sides, c.mid, causal=True, key_lengths=c.lengths.to(DEV), split=4).levels
    assert torch.equal(one, first[:, :, h * G * D:(h + 1) * G * D])


def test_gqa_decode_step_with_split_replays_in_a_graph():
    """KVCacheW8 (128 slots: two chunks of 64), RotaryW8Q and the core with decode=True, split=2 captured once -- the workspace's
    torch.empty inside the capture --; seven replays with only device buffers rewritten: every step is the CPU decode's and the
    prefill's row; then `lengths` is overwritten in place and the replay follows it"""
    from torchlsq import extension as E
    from torchlsq.quantized import KVCacheW8, RotaryW8Q
    case = C.gqa_decode_case()
    B, H, Hkv, T, D, Tmax = case["B"], case["H"], case["Hkv"], case["T"], case["D"], 128
    cpu_core = copy.deepcopy(case["core"])
    cpu_core.decode = True
    cpu_rot = RotaryW8Q(A.trained(-4.0, 4.0), D, Tmax, mid_dtype=BF16)         # the case's rotary with tables for 128 positions
    cpu_cache = KVCacheW8(B, Hkv, Tmax, D)
    cpu_steps = [C.gqa_decode_step(case, cpu_rot, cpu_core, cpu_cache, t) for t in range(T)]
    assert all(torch.equal(cpu_steps[t][:, 0], case["prefill"][:, t]) for t in range(T))
    rot, core = copy.deepcopy(cpu_rot).to(DEV), copy.deepcopy(cpu_core).to(DEV)
    core.split = 2
    cache = KVCacheW8(B, Hkv, Tmax, D, device=DEV)
    qt, kvt = case["q"][:, :1].to(DEV), case["kv"][:, :1].to(DEV)
    gcase = dict(case, consts=tuple(c.to(DEV) for c in case["consts"]))       # the constants are on the device before the capture
    pl = E.attn_decode_split_w8_plan(B, H, Hkv, 1, Tmax, D, 2, causal=True, causal_offset=Tmax - 1)
    assert pl["family"] == "split" and pl["splits"] == 2 and pl["chunk"] == 64
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        C.gqa_decode_step(gcase, rot, core, cache, 0, DEV, (qt, kvt))
    torch.cuda.current_stream().wait_stream(side)
    cache.lengths.zero_()
    cache.k.zero_()
    cache.v.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = C.gqa_decode_step(gcase, rot, core, cache, 0, DEV, (qt, kvt))
    cache.lengths.zero_()
    cache.k.zero_()
    cache.v.zero_()
    for t in range(T):
        qt.copy_(case["q"][:, t:t + 1])
        kvt.copy_(case["kv"][:, t:t + 1])
        graph.replay()
        assert cache.lengths.tolist() == [t + 1] * B
        assert torch.equal(out.cpu(), cpu_steps[t]) and torch.equal(out[:, 0].cpu(), case["prefill"][:, t]), t
    assert torch.equal(cache.k.cpu(), cpu_cache.k) and torch.equal(cache.v.cpu(), cpu_cache.v)
    # lengths overwritten in place: batch 0 starts over at slot 0, batch 1 goes on at 66 -- its keys now span both chunks (the slots
    # 7 .. 65 hold the level 0 in both caches) --; the replay appends there and attends to that many
    start = torch.tensor([0, 66], dtype=torch.int32)
    cpu_cache.lengths.copy_(start)
    want = C.gqa_decode_step(case, cpu_rot, cpu_core, cpu_cache, 5)
    cache.lengths.copy_(start.to(DEV))
    qt.copy_(case["q"][:, 5:6])
    kvt.copy_(case["kv"][:, 5:6])
    graph.replay()
    assert cache.lengths.tolist() == [1, 67] and torch.equal(out.cpu(), want) and not torch.equal(want, cpu_steps[5])
    assert torch.equal(cache.k.cpu(), cpu_cache.k) and torch.equal(cache.v.cpu(), cpu_cache.v)
