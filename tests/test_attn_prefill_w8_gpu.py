"""Prefill attention on 8-bit levels on the GPU (liblsq_hip_attn_prefill_w8.so): bit for bit against the CPU path of
`lsq_attention_decode_w8_q` (tests/attn_decode_w8_cases.definition: code of the parent commit, which tests/test_attn_decode_w8_cpu.py
holds to plain integers, to the existing module and to poisoned slots), at the smallest shapes at which each mechanism of the kernel
can fail.  The plan's family is asserted before every comparison, and beside the op the library's C entry is called directly on the
same operands -- no Python host, no fallback --: status 0 and the same bytes are the prefill kernel's own, EINVAL and untouched guard
bytes mean "composition".  The C entry is also how shapes with G Tq <= 16 reach the prefill kernel: the op sends those to the decode
kernel.  Every comparison is torch.equal; the softmax tables are built once on the CPU and moved.
"""
import copy
import itertools

import pytest
import torch

import attn_decode_w8_cases as C
import attn_prefill_w8_cases as P
import attn_w8_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
GUARD, LSQ_EINVAL, Z3 = P.GUARD, P.LSQ_EINVAL, P.Z3


def _equals_cpu(c, note="", family="prefill", shift=(0, 0, 0), k=None, v=None):
    pl = P.plan_of(c, qkv_aligned=not any(shift))
    assert pl["family"] == family, (note, pl)
    if family == "prefill":
        assert pl == P.expected_plan(c), (note, pl)
    C.check_not_degenerate(c)
    got = P.run(c, DEV, shift, k, v)
    assert got.shape == c.want.shape and got.dtype == c.want.dtype, note
    assert torch.equal(got.cpu(), c.want), note
    # the library's entry called directly: there is no fallback behind it, so status 0 and these bytes are the kernel's own
    rc, y = P.c_entry(c, DEV, shift, k, v)
    if family == "prefill":
        assert rc == 0 and torch.equal(y.cpu(), c.want), (note, rc)
    else:
        assert rc == LSQ_EINVAL and bool((y.view(U8) == GUARD).all()), (note, rc)
    return pl


# (B, Hkv, G, Tq, Tk, D), causal, key_lengths: one key and one row (the op: the decode kernel; the C entry: this one); two live waves,
# a partial packet, every row its own n; a second row tile of one live row, keys on both sides of the 64-key step, a batch entry cut
# by its length; three row tiles, nmax_wave 16, 32, .. 130, a partial 64-step of D with five column sub-tiles; an offset with a length
# below it at D 128; rows above 1024 keys: the second packet per lane of the softmax
SHAPES = [((1, 1, 1, 1, 1, 16), 0, None), ((1, 2, 3, 17, 17, 32), 0, None), ((2, 2, 4, 65, 65, 32), 0, (65, 13)),
          ((1, 1, 2, 130, 130, 80), 0, None), ((1, 1, 8, 64, 197, 128), True, (150,)), ((1, 1, 2, 200, 1040, 64), True, None)]


@pytest.mark.parametrize("shape,causal,lengths", SHAPES, ids=str)
def test_prefill_equals_the_cpu_path(shape, causal, lengths):
    B, Hkv, G, Tq, Tk, D = shape
    c = P.case(*shape, 0, causal=causal, lengths=lengths)
    if G * Tq <= 16:        # the op's first choice is the decode kernel; the prefill kernel serves the shape too, through its C entry
        assert C.plan_of(c)["family"] == "decode" and P.plan_of(c) == P.expected_plan(c)
        assert torch.equal(P.run(c, DEV).cpu(), c.want)
        rc, y = P.c_entry(c, DEV)
        assert rc == 0 and torch.equal(y.cpu(), c.want)
        return
    pl = _equals_cpu(c, shape)
    assert pl["grid"] == B * Hkv * G * ((Tq + 63) // 64) and pl["rows"] == 64 and pl["threads"] == 256 and pl["lds_dynamic"] == (Tk > 848)


def test_both_sides_of_the_64_kb_lds_line_and_the_largest_lds():
    from torchlsq import extension as E
    D = 128
    lo = max(T for T in range(700, 900) if not E.attn_prefill_w8_plan(1, 1, 1, 16, T, D, causal=True, causal_offset=T - 16)["lds_dynamic"])
    assert E.attn_prefill_w8_plan(1, 1, 1, 16, lo + 1, D, causal=True, causal_offset=lo - 15)["lds_dynamic"]
    for Tk in (lo, lo + 1):
        c = P.case(1, 1, 1, 16, Tk, D, 1, unsigned=P.SIGNED_PV, causal=True)
        # G Tq = 16: the op would take the decode kernel; the C entry is the prefill kernel's
        pl = P.plan_of(c)
        assert pl == P.expected_plan(c) and pl["lds_dynamic"] == (Tk > lo) and (pl["lds_bytes"] > 65536) == (Tk > lo)
        rc, y = P.c_entry(c, DEV)
        assert rc == 0 and torch.equal(y.cpu(), c.want), Tk
    # Tk_eff = 2048: the largest LDS and the dynamic launch
    c = P.case(1, 1, 1, 16, 2048, D, 1, causal=True)
    pl = P.plan_of(c)
    assert pl == P.expected_plan(c) and pl["lds_bytes"] == 143360 and pl["lds_dynamic"] and pl["lds_row_stride"] == 2064
    C.check_not_degenerate(c)
    rc, y = P.c_entry(c, DEV)
    assert rc == 0 and torch.equal(y.cpu(), c.want)
    assert torch.equal(P.run(c, DEV).cpu(), c.want)


def test_tk_eff_2049_goes_to_composition():
    _equals_cpu(P.case(1, 1, 1, 17, 2049, 32, 2, causal=True), "Tk_eff 2049", "composition")
    # the same cache under an offset that keeps every row at or below 2048 keys is served in place
    _equals_cpu(P.case(1, 1, 1, 17, 2049, 32, 2, causal=2031), "Tk_eff 2048 of 2049")


def test_a_long_cache_is_served_in_place():
    """Tk = 8192 with causal offset 100 and 32 rows: Tk_eff = 132; every slot from 132 on poisoned with 0xFF gives the same bytes"""
    c = P.case(1, 1, 2, 32, 8192, 64, 3, unsigned=C.ALL_UNSIGNED, causal=100)
    assert P.tk_eff(c) == 132 and P.plan_of(c)["lds_row_stride"] == 144
    _equals_cpu(c, "long cache")
    k, v = P.poisoned_from(c, 132, 0xFF)
    assert bool((k.levels[:, :, 132:] == 0xFF).all()) and torch.equal(k.levels[:, :, :132], c.k.levels[:, :, :132])
    _equals_cpu(c, "long cache, poisoned", k=k, v=v)


LENGTHS = (-3, 0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 199, 200, 205)


@pytest.mark.parametrize("causal", [0, 5, True, False], ids=str)
def test_key_counts_in_one_call(causal):
    """B = 15, Tq = 70, Tk = 200: a count on both sides of every packet, 64-key step and of Tk, and below 0, in both row tiles"""
    c = P.case(15, 1, 1, 70, 200, 32, 4, causal=causal, lengths=LENGTHS)
    zero = c.want[1, 0, 0]
    assert bool((c.want[0] == zero).all()) and bool((c.want[1] == zero).all()) and len(c.want[2:].unique()) > 16
    _equals_cpu(c, ("lengths", causal))


def test_poisoned_slots_do_not_reach_the_result():
    """every slot at or beyond the batch entry's largest n holds 0xFF: the same bytes.  k and v are dense buffers, so the last packet
    of the last row ends with the storage"""
    c = P.case(15, 1, 1, 70, 200, 32, 4, causal=5, lengths=LENGTHS)
    k, v = C.poisoned(c, 0xFF)
    assert bool((k.levels[3, :, 15:] == 0xFF).all()) and bool((k.levels[14, :, 75:] == 0xFF).all()) and torch.equal(k.levels[14, :, :75], c.k.levels[14, :, :75])
    last = k.levels.storage_offset() + (k.levels.numel() - 1) * k.levels.element_size() + 1
    assert last == k.levels.untyped_storage().nbytes()
    assert torch.equal(C.definition(c, k=k, v=v), c.want)
    _equals_cpu(c, "poisoned", k=k, v=v)
    # the probabilities quantizer with quant_min = 5: its level of 0.0 is not its z_p, and still nothing beyond n is read
    d = C.Case()
    d.shape, d.G, d.mid, d.causal, d.lengths, d.table = c.shape, c.G, c.mid, c.causal, c.lengths, c.table
    d.q, d.k, d.v = c.q, c.k, c.v
    p = c.sides[1]
    d.sides = (c.sides[0], (p[0], p[1], 5) + tuple(p[3:]), c.sides[2])
    C.finish(d)
    assert not torch.equal(d.want, c.want)
    _equals_cpu(d, "quant_min 5")
    _equals_cpu(d, "quant_min 5, poisoned", k=k, v=v)


@pytest.mark.parametrize("mid", A.MIDS, ids=str)
def test_every_dtype_combination(mid):
    for dtypes in itertools.product((U8, I8), repeat=3):
        for unsigned in itertools.product((True, False), repeat=3):
            _equals_cpu(P.case(1, 2, 2, 33, 65, 64, 5, dtypes, unsigned, mid, causal=True, lengths=(50,)), (dtypes, unsigned, mid))


def test_zero_points_far_from_the_middle():
    for dtypes in (C.ALL_U8, (I8, I8, I8), (U8, I8, U8)):
        _equals_cpu(P.case(1, 2, 2, 33, 65, 64, 6, dtypes, C.ALL_UNSIGNED, BF16, (3, 140, 250), causal=True, lengths=(60,)), dtypes)


def test_row_sums_beyond_32_bits_zero_entries_and_equal_scores():
    # every entry 2^24: S = 2^32 at 256 keys and 2^34 at 1024
    for Tk in (256, 1024):
        c = P.case(1, 1, 2, 17, Tk, 64, 7, unsigned=P.SIGNED_PV, table="full", causal=True)
        assert len(c.want.unique()) > 16
        _equals_cpu(c, ("full table", Tk))
    # a table whose tail is 0: entries that add nothing to S
    _equals_cpu(P.case(1, 2, 2, 20, 197, 64, 8, table="zeros", causal=True, lengths=(190,)), "zeros in the table")
    # rows of equal scores (q at its zero point: every product is 0) among ordinary ones
    c = C.Case()
    c.shape, c.G, c.mid, c.causal, c.lengths = (1, 2, 1, 40, 300, 64), 2, BF16, True, C.lens_tensor((290,))
    c.q, c.k, c.v = C.inputs(1, 1, 2, 40, 300, 64, 9)
    c.q.levels[:, :, 1::3] = A.QKV_Z
    c.table, c.sides = C.F.fitted_sides(c.q, C.expanded(c.k, 2), C.expanded(c.v, 2), C.ALL_UNSIGNED, BF16)
    C.finish(c)
    _equals_cpu(c, "equal scores")


def test_stale_lds_between_launches():
    """LDS is not zeroed between workgroups: a long call's bytes lie behind a shorter call's rows, rows beyond Tq and keys beyond
    nmax_wave"""
    _equals_cpu(P.case(1, 1, 2, 200, 1040, 64, 0, causal=True), "long")
    _equals_cpu(P.case(1, 1, 3, 20, 197, 64, 10, causal=True, lengths=(100,)), "197")
    _equals_cpu(P.case(1, 1, 2, 17, 40, 64, 10, causal=True, lengths=(0,)), "no keys")
    c = P.case(1, 1, 1, 1, 1, 64, 10, causal=True)
    rc, y = P.c_entry(c, DEV)
    assert rc == 0 and torch.equal(y.cpu(), c.want)


def _host_call(c, out, shift=(0, 0, 0)):
    from torchlsq import extension as E
    return E.attn_prefill_w8_q(*C.flat_args(c, DEV, shift), out=out)


def test_output_placement():
    c = P.case(2, 2, 3, 19, 19, 32, 11, causal=0, lengths=(19, 11))
    B, H, Hkv, T, Tk, D = c.shape
    # y through the [B, H, T, D] view of a [B, T, H D] region inside a larger buffer of guard bytes, rows 16 bytes longer than H D
    big = torch.full((B, T + 2, H * D + 16), GUARD, dtype=U8, device=DEV)
    yv = big[:, 1:T + 1, :H * D].view(B, T, H, D).permute(0, 2, 1, 3)
    pl = P.plan_of(c, y_strides=C.F.strides(yv))
    assert pl["family"] == "prefill" and pl["store"] == "packets"
    _host_call(c, yv)
    assert torch.equal(big[:, 1:T + 1, :H * D].cpu(), c.want)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, 1:T + 1, :H * D] = False
    assert bool((big[mask] == GUARD).all()), "bytes outside the logical y were written"
    # a y one byte off: still the prefill kernel, with the byte store
    raw = torch.full((B * T * H * D + 2,), GUARD, dtype=U8, device=DEV)
    yv = raw[1:-1].view(B, T, H, D).permute(0, 2, 1, 3)
    pl = P.plan_of(c, y_aligned=False)
    assert pl == P.expected_plan(c, "elements") and yv.data_ptr() % 16 == 1
    _host_call(c, yv)
    assert torch.equal(raw[1:-1].view(B, T, H * D).cpu(), c.want) and int(raw[0]) == GUARD and int(raw[-1]) == GUARD
    # a q one byte off, a k one byte off: the composition, the same bytes
    _equals_cpu(c, "q one byte off", "composition", (1, 0, 0))
    _equals_cpu(c, "k one byte off", "composition", (0, 1, 0))
    # D = 24: the composition
    _equals_cpu(P.case(1, 2, 2, 19, 19, 24, 11, causal=0), "D 24", "composition")


def test_launches_repeat_and_batches_depend_on_their_own_inputs_alone():
    from torchlsq.functional import lsq_attention_prefill_w8_q
    c = P.case(3, 2, 2, 70, 130, 64, 12, causal=True, lengths=(130, 60, 97))
    assert P.plan_of(c)["family"] == "prefill"
    first, second = P.run(c, DEV), P.run(c, DEV)
    assert torch.equal(first, second) and torch.equal(first.cpu(), c.want)
    sides, tab = C.F.sides_on(c.sides, DEV), c.table.to(DEV)
    for b in range(3):
        q, k, v = (C.with_levels(x, x.levels[b:b + 1]) for x in (C.moved(c.q, DEV), C.moved(c.k, DEV), C.moved(c.v, DEV)))
        one = lsq_attention_prefill_w8_q(q, k, v, tab, *sides, c.mid, causal=True, key_lengths=c.lengths[b:b + 1].to(DEV)).levels
        assert torch.equal(one[0], first[b]), b
    # one kv head alone: its G query heads' columns
    h, D, G = 1, 64, 2
    q, k, v = (C.with_levels(x, f(x.levels)) for x, f in ((C.moved(c.q, DEV), lambda t: t[:, h * G:(h + 1) * G]),
                                                         (C.moved(c.k, DEV), lambda t: t[:, h:h + 1]), (C.moved(c.v, DEV), lambda t: t[:, h:h + 1])))
    one = lsq_attention_prefill_w8_q(q, k, v, tab, *sides, c.mid, causal=True, key_lengths=c.lengths.to(DEV)).levels
    assert torch.equal(one, first[:, :, h * G * D:(h + 1) * G * D])


def test_module_prefill_equals_decode_and_the_masked_core_on_expanded_k_and_v():
    from torchlsq import extension as E
    B, Hkv, G, T, D = 2, 2, 4, 40, 64
    core = P.core(D, causal=0)
    q, k, v = C.inputs(B, Hkv, G, T, T, D, 13)
    lens = C.lens_tensor((40, 23))
    want = core(q, C.expanded(k, G), C.expanded(v, G), key_lengths=lens).levels
    assert E.attn_prefill_w8_plan(B, Hkv * G, Hkv, T, T, D, q_strides=C.F.strides(q.levels), causal=True, causal_offset=0)["family"] == "prefill"
    plain = copy.deepcopy(core).to(DEV)
    dec, pre = copy.deepcopy(plain), copy.deepcopy(plain)
    dec.decode, pre.prefill = True, True
    gq, gk, gv = (C.moved(x, DEV) for x in (q, k, v))
    a = plain(gq, C.expanded(gk, G), C.expanded(gv, G), key_lengths=lens.to(DEV))
    b = dec(gq, gk, gv, key_lengths=lens.to(DEV))
    p = pre(gq, gk, gv, key_lengths=lens.to(DEV))
    assert len(want.unique()) > 16 and list(pre.state_dict()) == list(core.state_dict())
    assert torch.equal(p.levels, b.levels) and torch.equal(p.levels, a.levels) and torch.equal(p.levels.cpu(), want)
    assert torch.equal(a.scale, p.scale) and torch.equal(a.zero_point, p.zero_point)


def _prompt(case, rot, core, cache, dev, tokens=None, keep=None):
    """the prompt of `gqa_decode_case` on `dev`: q and k rotated, k and v appended to the empty cache, `core` with causal offset 0 and
    the returned lengths -> the context's levels [B, T, H D]"""
    from torchlsq.functional import LevelsTensor
    qb, kv = (case["q"].to(dev), case["kv"].to(dev)) if tokens is None else tokens
    consts = tuple(c.to(dev) for c in case["consts"])
    q, k, v = LevelsTensor(qb, *consts, 0, 255), LevelsTensor(kv[:, :, 0], *consts, 0, 255), LevelsTensor(kv[:, :, 1], *consts, 0, 255)
    rq = rot(q, positions=cache.lengths)
    kl, vl, lens = cache.append(k, v, rotary=rot)
    core.causal = 0
    operands = (LevelsTensor(rq.levels.permute(0, 2, 1, 3), rq.scale, rq.zero_point, rq.quant_min, rq.quant_max), kl, vl)
    if keep is not None:
        keep.extend(operands + (lens,))
    return core(*operands, key_lengths=lens).levels


def _prompt_case(T=19):
    """B 2, H 4, Hkv 2, D 32, Tmax 32: 19 prompt tokens and three more, the modules of `gqa_decode_case`"""
    base = C.gqa_decode_case()
    B, H, Hkv, D = base["B"], base["H"], base["Hkv"], base["D"]
    rot = type(base["rot"])(A.trained(-4.0, 4.0), D, 32, mid_dtype=BF16)
    return dict(base, T=T, Tmax=32, rot=rot, q=A.levels((B, T + 3, H, D), 95, U8), kv=A.levels((B, T + 3, 2, Hkv, D), 96, U8))


def test_prompt_then_steps_through_one_module_with_graph_capture():
    from torchlsq import extension as E
    from torchlsq.quantized import KVCacheW8
    full = _prompt_case()
    B, H, Hkv, T, D, Tmax = full["B"], full["H"], full["Hkv"], full["T"], full["D"], full["Tmax"]
    prompt = dict(full, q=full["q"][:, :T], kv=full["kv"][:, :T])
    assert E.attn_prefill_w8_plan(B, H, Hkv, T, Tmax, D, q_strides=(T * H * D, D, H * D), causal=True, causal_offset=0)["family"] == "prefill"
    assert E.attn_decode_w8_plan(B, H, Hkv, T, Tmax, D, q_strides=(T * H * D, D, H * D), causal=True, causal_offset=0)["family"] == "composition"
    # the CPU run: the definition; and the existing core on expanded k and v of the rotated prompt
    cpu_core = copy.deepcopy(full["core"])
    cpu_core.prefill = True
    cpu_cache = KVCacheW8(B, Hkv, Tmax, D)
    kept = []
    want = _prompt(prompt, full["rot"], cpu_core, cpu_cache, "cpu", keep=kept)
    assert cpu_cache.lengths.tolist() == [T] * B and len(want.unique()) > 32
    old = copy.deepcopy(full["core"])
    old.causal = 0
    rq, kl, vl, lens = kept
    assert torch.equal(old(rq, C.expanded(kl, H // Hkv), C.expanded(vl, H // Hkv), key_lengths=lens).levels, want)
    # the GPU: a warm-up on a side stream, the capture, a replay on the same buffers
    rot, core = copy.deepcopy(full["rot"]).to(DEV), copy.deepcopy(cpu_core).to(DEV)
    cache = KVCacheW8(B, Hkv, Tmax, D, device=DEV)
    qb, kvb = prompt["q"].to(DEV), prompt["kv"].to(DEV)
    gcase = dict(prompt, consts=tuple(c.to(DEV) for c in full["consts"]))

    def clear():
        cache.lengths.zero_()
        cache.k.zero_()
        cache.v.zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        warm = _prompt(gcase, rot, core, cache, DEV, (qb, kvb))
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(warm.cpu(), want)
    clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = _prompt(gcase, rot, core, cache, DEV, (qb, kvb))
    clear()
    graph.replay()
    assert cache.lengths.tolist() == [T] * B and torch.equal(out.cpu(), want)
    assert torch.equal(cache.k.cpu(), cpu_cache.k) and torch.equal(cache.v.cpu(), cpu_cache.v)
    # the token buffers and `lengths` overwritten in place: other tokens, batch 0 appends at slot 0 and batch 1 at slot 3 -- the
    # replay follows the new lengths (n = min(t + 1, lengths + T))
    other = dict(prompt, q=full["q"][:, 3:T + 3], kv=full["kv"][:, 3:T + 3])
    start = torch.tensor([0, 3], dtype=torch.int32)
    cpu2 = KVCacheW8(B, Hkv, Tmax, D)
    cpu2.k.copy_(cpu_cache.k)
    cpu2.v.copy_(cpu_cache.v)
    cpu2.lengths.copy_(start)
    want2 = _prompt(other, full["rot"], cpu_core, cpu2, "cpu")
    cache.lengths.copy_(start.to(DEV))
    qb.copy_(other["q"])
    kvb.copy_(other["kv"])
    graph.replay()
    assert cache.lengths.tolist() == [T, T + 3] and torch.equal(out.cpu(), want2) and not torch.equal(want2, want)
    # three decode steps through the SAME module, causal=True for the steps: the decode kernel, equal to the CPU steps
    clear()
    qb.copy_(prompt["q"])
    kvb.copy_(prompt["kv"])
    graph.replay()
    assert E.attn_decode_w8_plan(B, H, Hkv, 1, Tmax, D, causal=True, causal_offset=Tmax - 1)["family"] == "decode"
    core.causal = cpu_core.causal = True
    for t in range(T, T + 3):
        a = C.gqa_decode_step(full, full["rot"], cpu_core, cpu_cache, t)
        b = C.gqa_decode_step(gcase | dict(q=full["q"], kv=full["kv"]), rot, core, cache, t, DEV)
        assert cache.lengths.tolist() == [t + 1] * B and torch.equal(b.cpu(), a), t
