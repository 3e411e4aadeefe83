"""Decode attention on 8-bit levels against a grouped-query KV cache on the GPU (liblsq_hip_attn_decode_w8.so): bit for bit against the
op's CPU path (tests/attn_decode_w8_cases.py; tests/test_attn_decode_w8_cpu.py holds that to plain integers, to the existing module
and to poisoned slots), at the smallest shapes at which each mechanism of the kernel can fail.  The plan's family is asserted before
every comparison, and beside the op the library's C entry is called directly on the same operands -- no Python host, no fallback --:
status 0 and the same bytes are the decode kernel's own, EINVAL and untouched guard bytes mean "composition".  Every comparison is
torch.equal; the softmax tables are built once on the CPU and moved.
"""
import copy
import itertools

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


def _equals_cpu(c, note="", family="decode", shift=(0, 0, 0)):
    pl = C.plan_of(c, qkv_aligned=not any(shift))
    assert pl["family"] == family, (note, pl)
    C.check_not_degenerate(c)
    got = C.run(c, DEV, shift)
    assert got.shape == c.want.shape and got.dtype == c.want.dtype, note
    assert torch.equal(got.cpu(), c.want), note
    # the library's entry called directly: there is no fallback behind it, so status 0 and these bytes are the kernel's own
    rc, y = C.c_entry(c, DEV, shift)
    if family == "decode":
        assert rc == 0 and torch.equal(y.cpu(), c.want), (note, rc)
    else:
        assert rc == LSQ_EINVAL and bool((y.view(U8) == GUARD).all()), (note, rc)
    return pl


# (B, Hkv, G, Tq, Tk, D), key_lengths: one key; two batches and kv heads, a partial packet; a full row tile and both sides of a
# 64-key step; R 15 with causal rows of different n; ViT's 197 at D 128; a partial 64-step of D with five column sub-tiles and a
# third partial sub-tile group; 1024: eight waves
SHAPES = [((1, 1, 1, 1, 1, 16), None), ((2, 2, 4, 1, 40, 32), (40, 13)), ((1, 1, 16, 1, 65, 64), None), ((1, 2, 3, 5, 19, 32), (17,)),
          ((1, 1, 8, 2, 197, 128), (150,)), ((1, 1, 2, 1, 130, 80), None), ((1, 1, 4, 1, 1024, 64), (1000,))]


@pytest.mark.parametrize("combo", [0, 1])
@pytest.mark.parametrize("shape,lengths", SHAPES, ids=str)
def test_decode_equals_the_cpu_path(shape, lengths, combo):
    B, Hkv, G, Tq, Tk, D = shape
    dtypes, unsigned = C.COMBOS[combo]
    pl = _equals_cpu(C.case(*shape, 0, dtypes, SIGNED_PV if Tk >= 1024 else unsigned, BF16, Z3, None, True, lengths), (shape, combo))
    assert pl["grid"] == B * Hkv and pl["rows"] == G * Tq and pl["threads"] == (256 if Tk <= 256 else 512)
    assert pl["lds_bytes"] <= 163840 and not pl["lds_dynamic"]


def test_both_sides_of_the_64_kb_lds_line_and_the_largest_lds():
    from torchlsq import extension as E
    D = 128
    lo = max(T for T in range(2700, 2800) if not E.attn_decode_w8_plan(1, 2, 1, 1, T, D)["lds_dynamic"])
    assert E.attn_decode_w8_plan(1, 2, 1, 1, lo + 1, D)["lds_dynamic"]
    for Tk in (lo, lo + 1):
        pl = _equals_cpu(C.case(1, 1, 2, 1, Tk, D, 1, C.ALL_U8, SIGNED_PV), Tk)
        assert pl["lds_dynamic"] == (Tk > lo) and (pl["lds_bytes"] > 65536) == (Tk > lo)
    pl = _equals_cpu(C.case(1, 1, 16, 1, 8192, D, 1, C.ALL_U8, SIGNED_PV), 8192)
    assert pl["lds_bytes"] == 152832 and pl["lds_dynamic"] and pl["rows"] == 16


LENGTHS = (-3, 0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 199, 200, 205)


def test_key_counts_in_one_call():
    """B = 15, Tk = 200: a count on both sides of every packet, 64-key step and of Tk, and below 0"""
    c = C.case(15, 1, 2, 1, 200, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, LENGTHS)
    zero = c.want[1, 0, 0]
    assert bool((c.want[0] == zero).all()) and bool((c.want[1] == zero).all()) and len(c.want[2:].unique()) > 16
    _equals_cpu(c, "lengths")
    # two query rows per head: the causal offset moves the first row's count one below the second's
    _equals_cpu(C.case(15, 1, 2, 2, 200, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, LENGTHS), "lengths, Tq 2")
    _equals_cpu(C.case(15, 1, 2, 2, 200, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, 5, LENGTHS), "lengths, offset 5")
    _equals_cpu(C.case(15, 1, 2, 2, 200, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, False, LENGTHS), "lengths, not causal")


def test_poisoned_slots_do_not_reach_the_result():
    """every slot at or beyond the batch's key count holds 0xFF: the same bytes.  k and v are dense buffers, so the last packet of
    the last row ends with the storage"""
    c = C.case(15, 1, 2, 1, 200, 32, 2, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, LENGTHS)
    k, v = C.poisoned(c, 0xFF)
    assert bool((k.levels[3, :, 15:] == 0xFF).all()) and torch.equal(k.levels[13], c.k.levels[13])
    last = k.levels.storage_offset() + (k.levels.numel() - 1) * k.levels.element_size() + 1
    assert last == k.levels.untyped_storage().nbytes()
    assert torch.equal(C.definition(c, k=k, v=v), c.want)
    assert torch.equal(C.run(c, DEV, k=k, v=v).cpu(), c.want)
    # the probabilities quantizer with quant_min = 5: its level of 0.0 is not its z_p, and still nothing beyond n is read
    d = C.Case()
    d.shape, d.G, d.mid, d.causal, d.lengths, d.table = c.shape, c.G, c.mid, c.causal, c.lengths, c.table
    d.q, d.k, d.v = c.q, c.k, c.v
    p = c.sides[1]
    d.sides = (c.sides[0], (p[0], p[1], 5) + tuple(p[3:]), c.sides[2])
    C.finish(d)
    assert not torch.equal(d.want, c.want)
    _equals_cpu(d, "quant_min 5")
    assert torch.equal(C.run(d, DEV, k=k, v=v).cpu(), d.want)


@pytest.mark.parametrize("mid", A.MIDS, ids=str)
def test_every_dtype_combination(mid):
    for dtypes in itertools.product((U8, I8), repeat=3):
        for unsigned in itertools.product((True, False), repeat=3):
            _equals_cpu(C.case(1, 2, 2, 2, 65, 64, 3, dtypes, unsigned, mid, Z3, None, True, (50,)), (dtypes, unsigned, mid))


def test_zero_points_far_from_the_middle():
    for dtypes in (C.ALL_U8, (I8, I8, I8), (U8, I8, U8)):
        _equals_cpu(C.case(1, 2, 4, 1, 65, 64, 4, dtypes, C.ALL_UNSIGNED, BF16, (3, 140, 250), None, True, (60,)), dtypes)


def test_row_sums_beyond_32_bits_zero_entries_and_equal_scores():
    # every entry 2^24: S = 2^32 at 256 keys and 2^34 at 1024
    for Tk in (256, 1024):
        c = C.case(1, 1, 4, 2, Tk, 64, 5, C.ALL_U8, SIGNED_PV, BF16, Z3, "full", True, None)
        assert len(c.want.unique()) > 16
        _equals_cpu(c, ("full table", Tk))
    # a table whose tail is 0: entries that add nothing to S
    _equals_cpu(C.case(1, 2, 4, 1, 197, 64, 6, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, "zeros", True, (190,)), "zeros in the table")
    # rows of equal scores (q at its zero point: every product is 0) among ordinary ones
    c = C.Case()
    c.shape, c.G, c.mid, c.causal, c.lengths = (1, 8, 1, 2, 300, 64), 8, BF16, True, C.lens_tensor((290,))
    c.q, c.k, c.v = C.inputs(1, 1, 8, 2, 300, 64, 7)
    c.q.levels[:, 1::3] = A.QKV_Z
    c.table, c.sides = C.F.fitted_sides(c.q, C.expanded(c.k, 8), C.expanded(c.v, 8), C.ALL_UNSIGNED, BF16)
    C.finish(c)
    _equals_cpu(c, "equal scores")


def test_stale_lds_between_launches():
    """LDS is not zeroed between workgroups: a long call's bytes lie behind a shorter call's rows, rows beyond R and keys beyond nmax"""
    _equals_cpu(C.case(1, 1, 16, 1, 1024, 64, 8, C.ALL_U8, SIGNED_PV), "long")
    for shape, lengths in (((1, 1, 3, 1, 197, 64), (100,)), ((1, 1, 1, 1, 40, 64), (0,)), ((1, 1, 1, 1, 1, 64), None)):
        _equals_cpu(C.case(*shape, 8, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, lengths), shape)


def _host_call(c, out, shift=(0, 0, 0)):
    from torchlsq import extension as E
    return E.attn_decode_w8_q(*C.flat_args(c, DEV, shift), out=out)


def test_output_placement():
    c = C.case(2, 2, 3, 5, 19, 32, 9, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (19, 11))
    B, H, Hkv, T, Tk, D = c.shape
    # y through the [B, H, T, D] view of a [B, T, H D] region inside a larger buffer of guard bytes, rows 16 bytes longer than H D
    big = torch.full((B, T + 2, H * D + 16), GUARD, dtype=U8, device=DEV)
    yv = big[:, 1:T + 1, :H * D].view(B, T, H, D).permute(0, 2, 1, 3)
    assert C.plan_of(c, y_strides=C.F.strides(yv))["store"] == "packets"
    _host_call(c, yv)
    assert torch.equal(big[:, 1:T + 1, :H * D].cpu(), c.want)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, 1:T + 1, :H * D] = False
    assert bool((big[mask] == GUARD).all()), "bytes outside the logical y were written"
    # a y one byte off: still the decode kernel, with the byte store
    raw = torch.full((B * T * H * D + 2,), GUARD, dtype=U8, device=DEV)
    yv = raw[1:-1].view(B, T, H, D).permute(0, 2, 1, 3)
    pl = C.plan_of(c, y_aligned=False)
    assert pl["family"] == "decode" and pl["store"] == "elements" and yv.data_ptr() % 16 == 1
    _host_call(c, yv)
    assert torch.equal(raw[1:-1].view(B, T, H * D).cpu(), c.want) and int(raw[0]) == GUARD and int(raw[-1]) == GUARD
    # a q one byte off, a k one byte off: the composition, the same bytes
    _equals_cpu(c, "q one byte off", "composition", (1, 0, 0))
    _equals_cpu(c, "k one byte off", "composition", (0, 1, 0))


@pytest.mark.parametrize("shape", [(1, 1, 17, 1, 40, 32), (1, 2, 2, 1, 40, 24), (1, 1, 2, 1, 8193, 32)], ids=str)
def test_composition_on_the_gpu(shape):
    """R 17, D 24 and Tk 8193: legal, not served by the kernel -- the op runs the existing ops composed, the C entry refuses"""
    c = C.case(*shape, 10, C.ALL_U8, SIGNED_PV if shape[4] > 1024 else C.ALL_UNSIGNED, BF16, Z3, None, True, (shape[4] - 3,))
    _equals_cpu(c, shape, "composition")


def test_launches_repeat_and_batches_depend_on_their_own_inputs_alone():
    from torchlsq.functional import lsq_attention_decode_w8_q
    c = C.case(3, 2, 4, 1, 197, 64, 11, C.ALL_U8, C.ALL_UNSIGNED, BF16, Z3, None, True, (197, 60, 133))
    first, second = C.run(c, DEV), C.run(c, DEV)
    assert torch.equal(first, second) and torch.equal(first.cpu(), c.want)
    sides, tab = C.F.sides_on(c.sides, DEV), c.table.to(DEV)
    for b in range(3):
        q, k, v = (C.with_levels(x, x.levels[b:b + 1]) for x in (C.moved(c.q, DEV), C.moved(c.k, DEV), C.moved(c.v, DEV)))
        one = lsq_attention_decode_w8_q(q, k, v, tab, *sides, c.mid, causal=True, key_lengths=c.lengths[b:b + 1].to(DEV)).levels
        assert torch.equal(one[0], first[b]), b
    # one kv head alone: its G query heads' columns
    h, D, G = 1, 64, 4
    q, k, v = (C.with_levels(x, f(x.levels)) for x, f in ((C.moved(c.q, DEV), lambda t: t[:, h * G:(h + 1) * G]),
                                                         (C.moved(c.k, DEV), lambda t: t[:, h:h + 1]), (C.moved(c.v, DEV), lambda t: t[:, h:h + 1])))
    one = lsq_attention_decode_w8_q(q, k, v, tab, *sides, c.mid, causal=True, key_lengths=c.lengths.to(DEV)).levels
    assert torch.equal(one, first[:, :, h * G * D:(h + 1) * G * D])


def test_module_decode_equals_the_masked_core_on_expanded_k_and_v():
    from torchlsq.quantized import AttentionCoreW8Q
    D, G = 64, 4
    span = 6.0 * A.QKV_S * A.QKV_S * 74 * 74 * D ** 0.5
    core = AttentionCoreW8Q(A.trained(-span, span), A.trained(0.0, 1.0), A.trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16, causal=True)
    q, k, v = C.inputs(2, 2, G, 1, 197, D, 12)
    lens = C.lens_tensor((197, 77))
    want = core(q, C.expanded(k, G), C.expanded(v, G), key_lengths=lens).levels
    plain = copy.deepcopy(core).to(DEV)
    dec = copy.deepcopy(plain)
    dec.decode = True
    gq, gk, gv = (C.moved(x, DEV) for x in (q, k, v))
    a = plain(gq, C.expanded(gk, G), C.expanded(gv, G), key_lengths=lens.to(DEV))
    b = dec(gq, gk, gv, key_lengths=lens.to(DEV))
    assert len(want.unique()) > 16 and list(dec.state_dict()) == list(core.state_dict())
    assert torch.equal(a.levels, b.levels) and torch.equal(b.levels.cpu(), want)
    assert torch.equal(a.scale, b.scale) and torch.equal(a.zero_point, b.zero_point)


def test_gqa_decode_step_replays_in_a_graph():
    """KVCacheW8, RotaryW8Q and the core with decode=True captured once; seven replays with only device buffers rewritten: every
    step is the CPU decode's and the prefill's row; then `lengths` is overwritten in place and the replay follows it"""
    from torchlsq.quantized import KVCacheW8
    case = C.gqa_decode_case()
    B, H, Hkv, T, D = case["B"], case["H"], case["Hkv"], case["T"], case["D"]
    cpu_core = copy.deepcopy(case["core"])
    cpu_core.decode = True
    cpu_cache = KVCacheW8(B, Hkv, case["Tmax"], D)
    cpu_steps = [C.gqa_decode_step(case, case["rot"], cpu_core, cpu_cache, t) for t in range(T)]
    rot, core = copy.deepcopy(case["rot"]).to(DEV), copy.deepcopy(cpu_core).to(DEV)
    cache = KVCacheW8(B, Hkv, case["Tmax"], D, device=DEV)
    qt, kvt = case["q"][:, :1].to(DEV), case["kv"][:, :1].to(DEV)
    gcase = dict(case, consts=tuple(c.to(DEV) for c in case["consts"]))       # the constants are on the device before the capture
    from torchlsq import extension as E
    assert E.attn_decode_w8_plan(B, H, Hkv, 1, case["Tmax"], D, causal=True, causal_offset=case["Tmax"] - 1)["family"] == "decode"
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
    # lengths overwritten in place: batch 0 starts over at slot 0, batch 1 goes on at 3; the replay appends there and attends to that many
    start = torch.tensor([0, 3], dtype=torch.int32)
    cpu_cache.lengths.copy_(start)
    want = C.gqa_decode_step(case, case["rot"], cpu_core, cpu_cache, 5)
    cache.lengths.copy_(start.to(DEV))
    qt.copy_(case["q"][:, 5:6])
    kvt.copy_(case["kv"][:, 5:6])
    graph.replay()
    assert cache.lengths.tolist() == [1, 4] and torch.equal(out.cpu(), want) and not torch.equal(want, cpu_steps[5])
