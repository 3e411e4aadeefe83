"""What tests/test_attn_chunk_w8_cpu.py and tests/test_attn_chunk_w8_gpu.py share: the cases of `attn_decode_w8_cases` (their `want` is
the definition, the parent commit's code) and their pools of `attn_paged_w8_cases` run through chunked prefill attention --
`lsq_attention_chunk_w8_q` on a device of choice, the library's two C entries called directly with a caller-made workspace and guard
bytes, the plans --, the expected bytes of the mask mode that `attn_decode_w8_cases.definition` does not know (`want_lengths`: built
per batch entry from that definition), and the whole decoder layer of `decoder_w8_cases` fed in chunks through
`AttentionCoreW8Q(chunk=True, causal="lengths")` by a `run` that never sets `causal` from a host-known start.  None of the three
imported modules is changed.
"""
import ctypes

import torch

import attn_decode_w8_cases as C
import attn_paged_w8_cases as P
import decoder_w8_cases as L

U8, I8, F32, BF16, F16 = C.U8, C.I8, C.F32, C.BF16, C.F16
GUARD = C.GUARD
LSQ_EINVAL = -1
LENGTHS = "lengths"


def mode_args(c, causal):
    """(mode, offset) of the ops for `causal` as the functional takes it (None / False, True, an int, "lengths")"""
    B, H, Hkv, Tq, Tk, D = c.shape
    if causal == LENGTHS:
        return 2, 0
    if causal is None or causal is False:
        return 0, 0
    return 1, (Tk - Tq if causal is True else int(causal))


def key_counts(c, causal, lengths):
    """n(b, t) by plain Python for all three modes: a list of B lists of Tq counts"""
    B, H, Hkv, Tq, Tk, D = c.shape
    if causal != LENGTHS:
        return C.key_counts(B, Tq, Tk, causal, lengths)
    return [[max(0, min(Tk, max(int(lengths[b]), 0)) - (Tq - 1 - t)) for t in range(Tq)] for b in range(B)]


def level_of_zero(c):
    """the context quantizer's level of 0.0 as a byte of the result's dtype"""
    o = c.sides[2]
    return torch.ops.torchlsq.lsq_levels_per_tensor(torch.zeros(1, dtype=c.mid), *o, 0).view(c.want.dtype)[0]


def want_lengths(c, lengths):
    """the expected levels [B, Tq, H D] of causal="lengths" with `lengths` (B ints), per batch entry from `C.definition`: with
    L = clamp(len_b, 0, Tk), L >= Tq is the definition at causal_offset = L - Tq with key_lengths [L]; L < Tq gives the last L rows by
    the definition at offset 0 with [L] and the context quantizer's level of 0.0 in the first Tq - L rows"""
    B, H, Hkv, Tq, Tk, D = c.shape
    out = torch.empty((B, Tq, H * D), dtype=c.want.dtype)
    for b in range(B):
        Lb = min(max(int(lengths[b]), 0), Tk)
        one = C.Case()
        one.table, one.sides, one.mid, one.lengths = c.table, c.sides, c.mid, torch.tensor([Lb], dtype=torch.int32)
        one.k, one.v = (C.with_levels(x, x.levels[b:b + 1]) for x in (c.k, c.v))
        if Lb >= Tq:
            one.causal, one.q = Lb - Tq, C.with_levels(c.q, c.q.levels[b:b + 1])
            out[b] = C.definition(one)[0]
        else:
            one.causal, one.q = 0, C.with_levels(c.q, c.q.levels[b:b + 1, :, Tq - Lb:])
            out[b, :Tq - Lb] = level_of_zero(c)
            if Lb:
                out[b, Tq - Lb:] = C.definition(one)[0]
    return out


def lens_of(c, lengths):
    return c.lengths if isinstance(lengths, str) else C.lens_tensor(lengths)


def run(c, dev, causal="case", splits=0, pg=None, lengths="case", shift=(0, 0, 0), operands=None, q=None):
    """`lsq_attention_chunk_w8_q` of the case on `dev` -> the levels [B, Tq, H D]; `causal`, `lengths`: instead of the case's; `pg`: the
    pools of `attn_paged_w8_cases.paged`; `operands`: (k, v) or (k_pool, v_pool, table) already on `dev` to use instead"""
    from torchlsq.functional import lsq_attention_chunk_w8_q
    causal = c.causal if isinstance(causal, str) and causal == "case" else causal
    lens = lens_of(c, lengths)
    bt = None
    if pg is None:
        k, v = (C.moved(c.k, dev, shift[1]), C.moved(c.v, dev, shift[2])) if operands is None else operands
    else:
        k, v, bt = P.on(dev, pg, shift[1:]) if operands is None else operands
    return lsq_attention_chunk_w8_q(C.moved(c.q if q is None else q, dev, shift[0]), k, v, c.table.to(dev), *C.F.sides_on(c.sides, dev), c.mid,
                                    causal=causal, key_lengths=None if lens is None else lens.to(dev), block_table=bt, splits=splits).levels


def plan_of(c, causal="case", splits=0, pg=None, lengths="case", qkv_aligned=True, y_aligned=True, overrides=()):
    from torchlsq import extension as E
    B, H, Hkv, Tq, Tk, D = c.shape
    causal = c.causal if isinstance(causal, str) and causal == "case" else causal
    mode, off = mode_args(c, causal)
    kw = dict(qkv_aligned=qkv_aligned, y_aligned=y_aligned, q_dtype=c.q.levels.dtype, k_dtype=c.k.levels.dtype, v_dtype=c.v.levels.dtype,
              causal=mode, causal_offset=off, has_lengths=lens_of(c, lengths) is not None, q_strides=C.F.strides(c.q.levels))
    if pg is None:
        kw.update(k_strides=C.F.strides(c.k.levels), v_strides=C.F.strides(c.v.levels))
        kw.update(dict(overrides))
        return E.attn_chunk_w8_plan(B, H, Hkv, Tq, Tk, D, splits, **kw)
    kw.update(k_strides=P.pool_strides(pg.k_pool.levels), v_strides=P.pool_strides(pg.v_pool.levels),
              bt_ld=int(pg.table.stride(0)) if B > 1 else pg.Mp)
    kw.update(dict(overrides))
    return E.attn_chunk_paged_w8_plan(B, H, Hkv, Tq, D, pg.Np, pg.ps, pg.Mp, splits, **kw)


def c_entry(c, dev, causal="case", splits=0, pg=None, lengths="case", shift=(0, 0, 0), ws=None, fill=0xA5, y_shift=0, operands=None):
    """`lsq_attn_chunk_w8` / `lsq_attn_chunk_paged_w8` called directly on the case's operands on the GPU with a caller-made workspace of
    the reported size (filled with `fill`, 64 guard bytes behind it): no Python host, so no fallback -> (status, the levels
    [B, Tq, H D] prefilled with 0x5A, the workspace, its reported size).  The guard bytes around y and behind the workspace are
    asserted untouched here."""
    from torchlsq import extension as E
    from torchlsq._attn_w8_host import _DTYPE_CODE, _LEVEL_CODE
    from torchlsq.functional import _act_constants
    B, H, Hkv, Tq, Tk, D = c.shape
    causal = c.causal if isinstance(causal, str) and causal == "case" else causal
    mode, off = mode_args(c, causal)
    lens = lens_of(c, lengths)
    lens = None if lens is None else lens.to(dev)
    q = C.moved(c.q, dev, shift[0])
    bt = None
    if pg is None:
        k, v = (C.moved(c.k, dev, shift[1]), C.moved(c.v, dev, shift[2])) if operands is None else operands
        ks, vs = C.F.strides(k.levels), C.F.strides(v.levels)
    else:
        k, v, bt = P.on(dev, pg, shift[1:]) if operands is None else operands
        ks, vs = P.pool_strides(k.levels), P.pool_strides(v.levels)
    sides, tab = C.F.sides_on(c.sides, dev), c.table.to(dev)
    raw = torch.full((B * Tq * H * D + 32,), GUARD, dtype=U8, device=dev)
    y = raw[y_shift:y_shift + B * Tq * H * D].view(B, Tq, H * D).view(c.want.dtype)
    need = plan_of(c, causal, splits, pg, lengths)["workspace_bytes"]
    made = ws is None
    if made:
        ws = torch.full((need + 64,), fill, dtype=U8, device=dev)
        ws[need:] = GUARD
    assert ws.data_ptr() % 16 == 0
    S = E.LsqAttnW8Strides
    geom = E.LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, *(_LEVEL_CODE[x.levels.dtype] for x in (q, k, v)), mode, off, 0 if lens is None else 1,
                                 S(*C.F.strides(q.levels)), S(*ks), S(*vs), S(*C.F.strides(y.view(B, Tq, H, D).permute(0, 2, 1, 3))))
    p_s, p_z = _act_constants(sides[1][0], sides[1][1], sides[1][4], sides[1][5])
    consts = E.LsqAttnDecodeW8Consts(q.scale.data_ptr(), q.zero_point.data_ptr(), k.scale.data_ptr(), k.zero_point.data_ptr(),
                                     v.scale.data_ptr(), v.zero_point.data_ptr(), p_s.data_ptr(), p_z.data_ptr())
    outs = [E.LsqAttnW8Out(s[0].data_ptr(), s[1].data_ptr(), *s[2:], _DTYPE_CODE[c.mid]) for s in sides]
    lib = E.attn_chunk_w8_library()
    head = (ctypes.byref(consts), *(ctypes.byref(o) for o in outs), tab.data_ptr(), None if lens is None else lens.data_ptr())
    tail = (q.levels.data_ptr(), k.levels.data_ptr(), v.levels.data_ptr(), y.data_ptr(), ws.data_ptr(), need, splits, None)
    torch.cuda.synchronize()                            # the call below goes to the default stream
    if pg is None:
        rc = lib.lsq_attn_chunk_w8(ctypes.byref(geom), *head, *tail)
    else:
        pages = E.LsqAttnPagedW8Pages(int(k.shape[0]), pg.ps, pg.Mp, int(bt.stride(0)) if B > 1 else pg.Mp)
        rc = lib.lsq_attn_chunk_paged_w8(ctypes.byref(geom), ctypes.byref(pages), *head, bt.data_ptr(), *tail)
    torch.cuda.synchronize()
    assert bool((raw[:y_shift] == GUARD).all()) and bool((raw[y_shift + B * Tq * H * D:] == GUARD).all()), "bytes outside y were written"
    assert not made or bool((ws[need:] == GUARD).all()), "bytes behind the reported workspace were written"
    return rc, y, ws, need


def check(c, dev, want, causal="case", splits=0, pg=None, lengths="case", family="chunk", forced=None, **kw):
    """the plan's family (and, with `forced`, its split count) asserted, then the op and the C entry on `dev` held to `want`: "chunk"
    gives status 0 and the same bytes, "composition" LSQ_EINVAL and untouched guard bytes"""
    pl = plan_of(c, causal, splits, pg, lengths, **{k: v for k, v in kw.items() if k in ("qkv_aligned", "y_aligned")})
    assert pl["family"] == family, pl
    if forced is not None:
        assert pl["splits"] == forced, pl
    run_kw = {k: v for k, v in kw.items() if k in ("shift", "operands")}
    got = run(c, dev, causal, splits, pg, lengths, **run_kw)
    assert torch.equal(got.cpu(), want), (c.shape, causal, splits, "the op")
    rc, y, ws, need = c_entry(c, dev, causal, splits, pg, lengths, **{k: v for k, v in kw.items() if k in ("shift", "operands", "y_shift", "fill")})
    if family == "chunk":
        assert rc == 0 and torch.equal(y.cpu(), want), (c.shape, causal, splits, "the C entry", rc)
    else:
        assert rc == LSQ_EINVAL and bool((y.view(U8) == GUARD).all()), rc
    return got


def poisoned(c, causal, lengths, fill, pg=None):
    """(k, v) of the case -- or with `pg` its pools, a `Paged` -- with every slot at or beyond the batch entry's nmax(b) filled with the
    byte `fill`"""
    B, H, Hkv, Tq, Tk, D = c.shape
    n = key_counts(c, causal, lengths)
    out = []
    for x in (c.k, c.v):
        lv = x.levels.clone()
        for b in range(B):
            lv.view(U8)[b, :, max(n[b]):] = fill
        out.append(C.with_levels(x, lv))
    if pg is None:
        return out
    d = C.Case()
    d.shape, d.k, d.v = c.shape, out[0], out[1]
    return P.paged(d, pg.ps, table=pg.table.to(torch.int64), extra=pg.Np - B * pg.Mp, fill=fill)


# ---------------------------------------------------------------------------------------------------
# the decoder layer of `decoder_w8_cases` fed in chunks: the core with chunk=True and causal="lengths", nothing set from the host
# ---------------------------------------------------------------------------------------------------
CHUNKINGS = {"whole": [67], "pieces": [20, 17, 24, 1, 5], "tokens": [1] * 67}


def chunk_layer(name, mid, device=None):
    """a copy of the case's converted layer whose core goes through the chunk route for every call"""
    import copy
    layer = copy.deepcopy(L.chain(name, mid))
    layer.core.chunk, layer.core.causal = True, LENGTHS
    return layer if device is None else layer.to(device)


def layer_run(layer, x, cache):
    """`decoder_w8_cases.run` without its two host-set attributes: the key counts come from the lengths the append returns"""
    H, Hkv, D = layer.H, layer.Hkv, layer.D
    n1 = layer.n1(x)
    qkv = layer.qkv(n1)
    q, k, v = L.heads(qkv, H, Hkv, D)
    B, T = int(q.shape[0]), int(q.shape[1])
    rbuf = torch.empty_like(qkv.levels)
    rq = layer.rot(q, positions=cache.lengths, out=rbuf[..., :H * D].view(B, T, H, D))
    kl, vl, lens = cache.append(k, v, rotary=layer.rot)
    ctx = layer.core(L.with_levels(rq, rq.levels.permute(0, 2, 1, 3)), kl, vl, key_lengths=lens,
                     block_table=cache.block_table if L.is_paged(cache) else None)
    add1 = layer.proj(ctx, x)
    n2 = layer.n2(add1)
    fc1 = layer.fc1(n2)
    gl = layer.act(fc1)
    out = layer.fc2(gl, add1)
    return out, dict(x=x, n1=n1, qkv=qkv, rq=rq, ctx=ctx, add1=add1, n2=n2, fc1=fc1, gelu=gl, out=out, k_cache=kl, v_cache=vl)


def layer_sequence(layer, xl, cache, chunks):
    """`decoder_w8_cases.sequence` on `layer_run` -> {stage: the levels of every call joined along T, on the CPU; "k", "v"}"""
    got, start = {s: [] for s in L.STAGES}, 0
    for T in chunks:
        x = L.with_levels(xl, xl.levels[:, start:start + T].contiguous())
        _, mids = layer_run(layer, x, cache)
        for s in L.STAGES:
            lv = mids[s].levels
            got[s].append(lv.reshape(lv.shape[0], T, -1).cpu())
        start += T
    out = {s: torch.cat(v, 1) for s, v in got.items()}
    assert cache.lengths.tolist() == [start] * int(xl.shape[0])
    out["k"], out["v"] = (t.cpu() for t in L.cached(cache, mids["k_cache"], mids["v_cache"], start))
    return out
