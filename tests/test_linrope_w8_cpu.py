"""The qkv linear of a decode step with the rotary embedding and the KV-cache append in its epilogue (include/lsq_hip_linrope_w8.h) on
CPU tensors, and what the GPU tests share.  `lsq_linear_w8_q8_dec_rope_q` defines nothing new, so the reference is PLAIN:
tests/test_lindec_w8_cpu.py's `reference` (an int64 matmul and the contract's float32 steps) gives the qkv bytes, torch.mul / sub /
add on `mid` tensors the rotation, numpy's level function its bytes, and plain indexing the placement.  Every comparison is on bytes."""
import functools

import pytest
import torch

import eltwise_w8_cases as E
import glu_w8_cases as G
import requant_w8_cases as R
import test_lindec_w8_cpu as L
from torchlsq import extension, functional as F

OPS = torch.ops.torchlsq
U8, I8 = torch.uint8, torch.int8
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FILL, TMAX, P = 0x5A, 32, 40            # the tables reach beyond the caches: a token at TMAX rotates q and skips k and v


@functools.lru_cache(maxsize=None)
def case(B, T, H, Hkv, D, Rd, K, x_dt=U8, w_dt=I8, qkv_u=True, rot_u=True, mid=BF16, bias="f32", paged=None, shift=0, layout=None):
    """CPU operands of one case, built once and left unchanged.  `paged`: None (dense caches [B, Hkv, TMAX, D]) or (page size,
    page_major).  positions[b] cycles through 0, TMAX - 1, TMAX, P and -2 from `shift`.  `layout`: None or one of LAYOUTS, what
    `call` hands the op besides.  `want`: rq, k, v as the op must leave destinations that held FILL; `at[b][t]`: (q written, k
    written, v written, batch entry or page, token or slot)"""
    lin = R.linear_case(B * T, (H + 2 * Hkv) * D, K, (x_dt, 117 if x_dt == U8 else -11, w_dt, None, None, bias), (qkv_u, False, mid), 0)
    return _placed(lin, (B, T, H, Hkv, D), Rd, rot_u, paged, shift, layout)


@functools.lru_cache(maxsize=None)
def extreme_case(paged=None):
    """K = 65536 on tests/test_lindec_w8_cpu.py's `extreme_lin`: sixteen sequences of one token, one q, one k and one v head of 32
    features, so the weight is [96, 65536] and every ROTATE and COPY item holds outputs with |I| = 65536 * 255 * 255 > 2^31"""
    return _placed(L.extreme_lin(96), (16, 1, 1, 1, 32), 32, True, paged, 0, None)


# what `call` hands the op besides the plain operands:
#   rq_in_qkv      rq is the first H heads of a [B, T, H + 2 Hkv, D] buffer, whose other heads are guard bytes
#   rq_padded      rq's heads lie D + 16 bytes apart, the 16 bytes behind each are guard bytes
#   token_major    dense caches stored [B, TMAX, Hkv, D], handed over as their [B, Hkv, TMAX, D] views
#   wide_table     the block table is the first Mp columns of a [B, Mp + 3] table whose other columns name pages of the NEXT sequence
#   no_positions   positions=None: every sequence starts at token 0
LAYOUTS = ("rq_in_qkv", "rq_padded", "token_major", "wide_table", "no_positions")


def _placed(lin, dims, Rd, rot_u, paged, shift, layout):
    """the case of a qkv projection's operands: the tables, the rotation's quantizer, the positions and what lands where"""
    assert layout is None or layout in LAYOUTS, layout
    B, T, H, Hkv, D = dims
    W, K, mid = H + 2 * Hkv, lin[0].shape[1], lin[11]
    qkv = L.reference(dict(lin=lin, res=None)).view(B, T, W, D)
    s_q, z_q = F._act_constants(lin[7], lin[8], *lin[9][2:])
    cos, sin = F.lsq_rope_tables(Rd, P, 10000.0, mid)
    pos = torch.tensor([0 if layout == "no_positions" else (0, TMAX - 1, TMAX, P, -2)[(b + shift) % 5] for b in range(B)], dtype=torch.int32)
    p = pos.to(torch.int64).reshape(B, 1) + torch.arange(T).reshape(1, T)
    d = ((qkv[:, :, :H + Hkv].to(F32) - z_q.to(F32)) * s_q).to(mid)
    c, s = (t[p.clamp(0, P - 1)].to(mid).unsqueeze(2) for t in (cos, sin))
    xi, xj = d[..., :Rd // 2], d[..., Rd // 2:Rd]
    u = torch.cat((torch.sub(torch.mul(xi, c), torch.mul(xj, s)), torch.add(torch.mul(xj, c), torch.mul(xi, s)), d[..., Rd:]), -1)
    rsc, rsh, rng = G.out_quantizer(u.float(), rot_u)
    lv = torch.from_numpy(E.numpy_levels(u.float().numpy(), rsc, rsh, rng))
    lv = lv.to(U8) if rot_u else lv.to(I8)
    R.assert_not_vacuous(lv, rng, (B, T, H, Hkv, D, Rd, K))
    table, wide = None, None
    shape = (B, Hkv, TMAX, D)
    if paged is not None:
        ps, Mp = paged[0], TMAX // paged[0]
        Np = B * Mp + 3
        table = torch.randperm(Np, generator=torch.Generator().manual_seed(7))[:B * Mp].reshape(B, Mp).to(torch.int32)
        if layout == "wide_table":      # a kernel that took the rows to lie Mp apart, or read beyond Mp, would write another sequence's page
            wide = torch.cat((table, table.roll(-1, 0)[:, torch.arange(3) % Mp]), 1)
            table = wide[:, :Mp]
        if B >= 7:
            table[5, 0], table[6, Mp - 1] = -1, Np + 1       # rows 5 and 6 sit at 0 and TMAX - 1 (shift 0): neither is written
        shape = (Np, Hkv, ps, D)
    rq = torch.full((B, T, H, D), FILL, dtype=lv.dtype)
    kc, vc = torch.full(shape, FILL, dtype=lv.dtype), torch.full(shape, FILL, dtype=qkv.dtype)
    at = [[None] * T for _ in range(B)]
    for b in range(B):
        for t in range(T):
            pp = int(p[b, t])
            outer, tok, there = b, pp, 0 <= pp < TMAX
            if there and paged is not None:
                outer, tok = int(table[b, pp // ps]), pp % ps
                there = 0 <= outer < shape[0]
            at[b][t] = (0 <= pp < P, there and pp < P, there, outer, tok)
            if at[b][t][0]:
                rq[b, t] = lv[b, t, :H]
            if at[b][t][1]:
                kc[outer, :, tok] = lv[b, t, H:]
            if there:
                vc[outer, :, tok] = qkv[b, t, H + Hkv:]
    return dict(lin=lin, cos=cos, sin=sin, pos=pos, rot=(rsc, rsh, rng), table=table, wide=wide, dims=(B, T, H, Hkv, D), paged=paged, at=at,
                layout=layout, want=(rq, kc, vc))


def call(c, device="cpu", fn=None, row=None, made=None):
    """`fn` (the host function by default) on the case's operands on `device`, into fresh destinations that lie inside larger buffers
    of FILL -> (rq, k, v, the guard bytes' tensors, `made`).  `row` = (b, t): on that row of x alone, as a call of its own.  `made`: the
    (arguments, destinations, whole buffers, guard bytes) of an earlier call, used again as they are."""
    fn = fn or extension.linrope_w8_q
    B, T, H, Hkv, D = c["dims"]
    lin, pos, table, rq_w, kc_w, layout = c["lin"], c["pos"], c["table"], c["want"][0], c["want"][1], c["layout"]
    x = lin[0].view(B, T, -1)
    if c["wide"] is not None:                                   # (a copy of the slice alone would be dense)
        table = c["wide"].to(device)[:, :table.shape[1]]
    if row is not None:
        b, t = row
        x, pos, table, B, T = x[b:b + 1, t:t + 1].contiguous(), pos[b:b + 1] + t, None if table is None else table[b:b + 1], 1, 1
    elif layout == "no_positions":
        pos = None
    if made is None:
        outer = kc_w.shape[0] if c["paged"] is not None else B
        q_shape = {"rq_in_qkv": (T, H + 2 * Hkv, D), "rq_padded": (T, H, D + 16)}.get(layout, (T, H, D))
        big = [torch.full((n + 2,) + s, FILL, dtype=dt, device=device) for n, s, dt in
               ((B, q_shape, rq_w.dtype), (outer, tuple(kc_w.shape[1:]), kc_w.dtype), (outer, tuple(kc_w.shape[1:]), c["want"][2].dtype))]
        if (c["paged"] is not None and not c["paged"][1]) or layout == "token_major":
            # storage [Np, ps, Hkv, D] or [B, TMAX, Hkv, D]: the pools or the caches are its permuted views
            big[1:] = [t.reshape(t.shape[0], t.shape[2], t.shape[1], D).permute(0, 2, 1, 3) for t in big[1:]]
        guards = [t[i] for t in big for i in (0, -1)]
        rq, kc, vc = (t[1:-1] for t in big)
        if layout in ("rq_in_qkv", "rq_padded"):
            guards.append(rq[:, :, H:] if layout == "rq_in_qkv" else rq[..., D:])
            rq = rq[:, :, :H, :D]
        dev = R.to(device, x, *lin[1:9], *F._act_constants(lin[7], lin[8], *lin[9][2:]), c["cos"], c["sin"], *c["rot"][:2], pos)
        made = ((*dev[:9], *lin[9], *dev[9:15], *c["rot"][2], lin[11], H, Hkv, kc, vc, dev[15], None if table is None else table.to(device)),
                (rq, kc, vc), big, guards)
    args, (rq, kc, vc), _, guards = made
    return fn(*args, out=rq), kc, vc, guards, made


def assert_row(c, device, b, t, fn=None):
    """the call on row (b, t) alone writes that row's bytes and nothing else"""
    got = call(c, device, fn=fn, row=(b, t))[:3]
    q_on, k_on, v_on, outer, tok = c["at"][b][t]
    want = [torch.full(g.shape, FILL, dtype=g.dtype) for g in got]
    o = outer if c["paged"] is not None else 0
    if q_on:
        want[0][0, 0] = c["want"][0][b, t]
    if k_on:
        want[1][o, :, tok] = c["want"][1][outer, :, tok]
    if v_on:
        want[2][o, :, tok] = c["want"][2][outer, :, tok]
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want)), (b, t)


# (B, T, H, Hkv, D, R, K, x, weight, qkv / rot levels unsigned, mid_dtype, bias, paged, shift, layout)
LAYOUT_CASES = [(2, 3, 2, 2, 64, 32, 272, U8, I8, True, True, F32, "f32", None, 1, "rq_in_qkv"),
                (16, 1, 4, 1, 128, 128, 272, I8, U8, False, False, BF16, "f32", None, 0, "rq_padded"),
                (2, 3, 2, 2, 64, 32, 4112, U8, I8, True, True, BF16, "f32", None, 3, "token_major"),
                (16, 1, 2, 1, 32, 32, 272, U8, I8, True, True, BF16, "f32", (16, True), 0, "wide_table"),
                (2, 3, 2, 2, 64, 32, 272, U8, I8, True, False, F16, None, (1, False), 0, "wide_table"),     # (b = 1 at TMAX - 1: row 1 is read)
                (2, 3, 2, 2, 64, 32, 272, U8, I8, True, True, F32, "f32", None, 0, "no_positions"),
                (16, 1, 2, 1, 32, 32, 272, I8, U8, False, True, BF16, None, (16, False), 0, "no_positions")]
CPU_CASES = [(2, 3, 2, 2, 64, 32, 272, U8, I8, True, True, F32, "f32", None, 1),
             (16, 1, 2, 1, 32, 32, 16, I8, U8, False, False, BF16, None, (16, True), 0),
             (3, 1, 2, 2, 64, 32, 4112, U8, I8, True, False, F16, "f32", (1, False), 0)] + LAYOUT_CASES


@pytest.mark.parametrize("spec", CPU_CASES, ids=lambda s: "-".join(str(v).replace("torch.", "") for v in s))
def test_cpu_path_equals_the_plain_reference(spec):
    c = case(*spec)
    rq, kc, vc, guards, _ = call(c)
    assert all(torch.equal(g, w) for g, w in zip((rq, kc, vc), c["want"])) and all(bool((g == FILL).all()) for g in guards)
    assert_row(c, "cpu", 1 // spec[1], 1 % spec[1])
    # the registered op: the same caches; rq comes from torch.empty, so only its written rows are defined
    rq2, kc2, vc2, _, _ = call(c, fn=lambda *a, out: OPS.lsq_linear_w8_q8_dec_rope_q(*a))
    written = torch.tensor([[row[0] for row in rows] for rows in c["at"]])
    assert torch.equal(rq2[written], c["want"][0][written]) and torch.equal(kc2, c["want"][1]) and torch.equal(vc2, c["want"][2])


def _module(route, rope_epilogue):
    """the qkv projection and the rotary module of tests/decoder_glu_w8_cases.py's layer as a QKVRotaryW8Q, an empty cache, n1's levels"""
    import copy
    import decoder_glu_w8_cases as D
    from torchlsq.quantized import QKVRotaryW8Q
    layer = D.chain("short", BF16)
    m = QKVRotaryW8Q(copy.deepcopy(layer.qkv), copy.deepcopy(layer.rot), layer.H, layer.Hkv, rope_epilogue=rope_epilogue)
    return m, D.make_cache("short", route), layer.n1(D.input_levels("short"))


@pytest.mark.parametrize("route", ["dense", "paged"])
def test_module_with_the_epilogue_equals_its_children_one_by_one(route):
    outs = []
    for flag in (True, False):
        m, cache, n1 = _module(route, flag)
        for a, b in ((0, 5), (5, 6), (6, 7)):       # a prompt of 5 (10 rows: the one op on the CPU), then two steps
            rq, kl, vl, lens = m(F.LevelsTensor(n1.levels[:, a:b].contiguous(), n1.scale, n1.zero_point, n1.quant_min, n1.quant_max), cache)
        outs.append((rq.levels, rq.scale, rq.zero_point, kl.levels, kl.scale, kl.zero_point, vl.levels, vl.scale, vl.zero_point, lens.clone()))
        outs[-1] += tuple(torch.tensor([t.quant_min, t.quant_max, t.type_min, t.type_max]) for t in (rq, kl, vl))
        assert lens.tolist() == [7, 7]
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and len(outs[0][3].unique()) > 16


def test_state_dict_keys_are_the_childrens():
    m, _, _ = _module("dense", None)
    keys = {"qkv." + k for k in m.qkv.state_dict()} | {"rotary." + k for k in m.rotary.state_dict()}
    assert set(m.state_dict()) == keys and m.rope_epilogue is None and F.W8A8_ROPE_EPILOGUE_DEFAULT in (True, False)
    m.rope_epilogue = True
    other, _, _ = _module("dense", None)
    other.load_state_dict(m.state_dict())
    assert other.rope_epilogue is True and set(m.state_dict()) == keys | {"_extra_state"}
    other.load_state_dict({k: v for k, v in m.state_dict().items() if k != "_extra_state"})
    assert other.rope_epilogue is None


@pytest.mark.parametrize("args, kw, want", [
    ((1, 1, 32, 8, 128, 4096), dict(P=64, Tmax=64), dict(served=True, block=1024, grid=192, chunks=1, x_resident=True, rotate_items=160,
                                                         pass_items=0, copy_items=32, lds_bytes=35840 + 1024 + 512 + 4112)),
    ((2, 3, 2, 2, 64, 4112), dict(R=32, P=64, pages=(9, 16, 4)), dict(served=True, grid=12, chunks=2, x_resident=False, rotate_items=4,
                                                                      pass_items=4, copy_items=4, lds_bytes=35840 + 1024 + 512 + 6 * 4112)),
    ((17, 1, 2, 2, 64, 64), dict(P=8, Tmax=8), dict(served=False, grid=0, block=0, rotate_items=0)),
    ((1, 1, 2, 2, 48, 64), dict(R=32, P=8, Tmax=8), dict(served=False)),
    ((1, 1, 2, 2, 64, 64), dict(R=16, P=8, Tmax=8), dict(served=False)),
    ((1, 1, 2, 2, 64, 64), dict(P=8, Tmax=8, interleaved=True), dict(served=False)),
    ((1, 1, 2, 2, 64, 24), dict(P=8, Tmax=8), dict(served=False)),
    ((1, 1, 2, 2, 64, 64), dict(P=8, Tmax=8, aligned=False), dict(served=False)),
    ((1, 1, 2, 2, 64, 64), dict(P=8, Tmax=8, q_strides=(256, 256, 72)), dict(served=False)),
])
def test_plan(args, kw, want):
    pl = extension.linrope_w8_plan(*args, **kw)
    assert {k: pl[k] for k in want} == want, pl


@pytest.mark.parametrize("kw, message", [
    (dict(R=31), "must be even"), (dict(R=96), "at most D"), (dict(P=0), "at least 1"), (dict(Tmax=0), "Tmax"),
    (dict(pages=(4, 0, 2)), "at least 1"), (dict(q_strides=(256, 256, 32)), "overlap"), (dict(k_strides=(-16, 64, 512)), "negative"),
])
def test_refusals(kw, message):
    with pytest.raises(RuntimeError, match=message):
        extension.linrope_w8_plan(1, 2, 2, 2, 64, 64, **dict(dict(P=8, Tmax=8), **kw))
    c = case(*CPU_CASES[0])
    with pytest.raises(Exception, match="k_cache must hold"):
        call(c, fn=lambda *a, out: extension.linrope_w8_q(*a[:26], a[26].view(I8), *a[27:], out=out))
