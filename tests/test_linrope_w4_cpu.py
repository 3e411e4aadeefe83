"""The qkv linear of a decode step on packed 4- / 2-bit weights with the rotary embedding and the KV-cache append in its epilogue
(include/lsq_hip_linrope_w4.h) on CPU tensors, and what the GPU tests share.  `lsq_linear_packed_q8_rope_q` defines nothing new, so
the reference is PLAIN: tests/test_lindec_w4_cpu.py's exact `case` / `reference` gives the qkv bytes, torch.mul / sub / add on `mid`
tensors the rotation, numpy's level function its bytes, and plain indexing the placement (the three steps of
tests/test_linrope_w8_cpu.py's `_placed`).  Every comparison is on bytes; destinations lie inside larger buffers of FILL."""
import functools

import pytest
import torch

import eltwise_w8_cases as E
import glu_w8_cases as G
import test_lindec_w4_cpu as W
from torchlsq import extension, functional as F

OPS = torch.ops.torchlsq
U8, F32, BF16 = torch.uint8, torch.float32, torch.bfloat16
FILL, TMAX, P = 0x5A, 32, 40            # the tables reach beyond the caches: a token at TMAX rotates q and skips k and v
# (B, T, H, Hkv, D, R, K, G, bits, page size or None, shift of the positions' cycle): the issue's table, row by row
CASES = [(1, 1, 1, 1, 32, 32, 128, 128, 4, None, 0), (2, 3, 2, 2, 64, 32, 4224, 32, 4, 16, 4), (16, 1, 4, 1, 128, 128, 2176, 128, 4, None, 0),
         (3, 1, 2, 1, 32, 32, 512, 256, 4, 1, 4), (2, 3, 2, 2, 64, 32, 768, 96, 4, None, 4), (16, 1, 2, 1, 32, 32, 1024, 64, 2, 16, 0),
         (2, 3, 2, 2, 64, 64, 256, 128, 2, None, 4), (1, 2, 253, 2, 32, 32, 128, 128, 4, None, 1)]
ident = lambda s: "-".join(str(v) for v in s)


@functools.lru_cache(maxsize=None)
def case(B, T, H, Hkv, D, Rd, K, Gs, bits, ps=None, shift=0, exact=True, seed=0):
    """CPU operands of one case, built once and left unchanged.  positions[b] cycles through 0, TMAX - 1, TMAX, P and -2 from
    `shift`.  `exact`: tests/test_lindec_w4_cpu.py's exact weights (far zero points: the 64-bit I) and `want`, rq, k, v as the op must
    leave destinations that held FILL, with `at[b][t]` = (q written, k written, v written, batch entry or page, token or slot).  Not
    vacuous: more than 16 distinct rq levels, and with at least two sequences a row written and a row skipped on every destination
    (one sequence of consecutive tokens cannot skip rq and write k: there a written row is asked for)."""
    lin = W.case(B * T, (H + 2 * Hkv) * D, K, Gs, bits, exact=exact, seed=seed)
    lx, s_x, zx, p, bias, (osc, osh, rng), _, mid, _ = lin["args"]
    s_q, z_q = F._act_constants(osc, osh, *rng[2:])
    cos, sin = F.lsq_rope_tables(Rd, P, 10000.0, mid)
    pos = torch.tensor([(0, TMAX - 1, TMAX, P, -2)[(b + shift) % 5] for b in range(B)], dtype=torch.int32)
    table, shape = None, (B, Hkv, TMAX, D)
    if ps is not None:
        Mp = TMAX // ps
        Np = B * Mp + 3
        table = torch.randperm(Np, generator=torch.Generator().manual_seed(7))[:B * Mp].reshape(B, Mp).to(torch.int32)
        if B >= 7:
            table[5, 0], table[6, Mp - 1] = -1, Np + 1       # rows 5 and 6 sit at 0 and TMAX - 1 (shift 0): neither is written
        shape = (Np, Hkv, ps, D)
    c = dict(x=lx.view(B, T, K), lin=(s_x, zx, *F._packed_operands(p, bias), osc, osh, *rng, s_q, z_q), cos=cos, sin=sin, pos=pos, table=table,
             dims=(B, T, H, Hkv, D), mid=mid, shape=shape, ps=ps, qkv_rng=rng, packed=p, bias=bias)
    if not exact:           # (random weights: the GPU test composes the existing GPU ops; the rotation's range is the qkv levels')
        c["rot"] = G.out_quantizer(1.2 * (torch.tensor([float(rng[0]), float(rng[1])]) - z_q.float()) * s_q, True)
        return c
    qkv = lin["want"].view(B, T, H + 2 * Hkv, D)
    pt = pos.to(torch.int64).reshape(B, 1) + torch.arange(T).reshape(1, T)
    d = ((qkv[:, :, :H + Hkv].to(F32) - z_q.to(F32)) * s_q).to(mid)
    cs, sn = (t[pt.clamp(0, P - 1)].to(mid).unsqueeze(2) for t in (cos, sin))
    xi, xj = d[..., :Rd // 2], d[..., Rd // 2:Rd]
    u = torch.cat((torch.sub(torch.mul(xi, cs), torch.mul(xj, sn)), torch.add(torch.mul(xj, cs), torch.mul(xi, sn)), d[..., Rd:]), -1)
    c["rot"] = rsc, rsh, rrng = G.out_quantizer(u.float(), True)
    lv = torch.from_numpy(E.numpy_levels(u.float().numpy(), rsc, rsh, rrng)).to(U8)
    rq, kc, vc = torch.full((B, T, H, D), FILL, dtype=U8), torch.full(shape, FILL, dtype=U8), torch.full(shape, FILL, dtype=qkv.dtype)
    at = [[None] * T for _ in range(B)]
    for b in range(B):
        for t in range(T):
            pp = int(pt[b, t])
            outer, tok, there = b, pp, 0 <= pp < TMAX
            if there and ps is not None:
                outer, tok = int(table[b, pp // ps]), pp % ps
                there = 0 <= outer < shape[0]
            at[b][t] = (0 <= pp < P, there and pp < P, there, outer, tok)
            if at[b][t][0]:
                rq[b, t] = lv[b, t, :H]
            if at[b][t][1]:
                kc[outer, :, tok] = lv[b, t, H:]
            if there:
                vc[outer, :, tok] = qkv[b, t, H + Hkv:]
    rows = [row for seq in at for row in seq]
    assert len(lv[:, :, :H].unique()) > 16, "a vacuous case"
    assert all(any(r[i] for r in rows) and (B == 1 or not all(r[i] for r in rows)) for i in range(3)), "a vacuous placement"
    return dict(c, at=at, want=(rq, kc, vc))


def call(c, device="cpu", fn=None, row=None, layout=None, made=None):
    """`fn` (the host function by default) on the case's operands on `device`, into fresh destinations inside larger buffers of FILL
    -> (rq, k, v, the guard bytes' tensors, `made`).  `row` = (b, t): on that row of x alone.  `layout`: "rq_in_qkv" (rq is the first
    H heads of a [B, T, H + 2 Hkv, D] buffer) or "token_major" (dense caches stored [B, TMAX, Hkv, D], handed over as permuted
    views).  `made`: the arguments and buffers of an earlier call, used again as they are."""
    fn = fn or extension.linrope_w4_q
    B, T, H, Hkv, D = c["dims"]
    x, pos, table = c["x"], c["pos"], c["table"]
    if row is not None:
        b, t = row
        x, pos, table, B, T = x[b:b + 1, t:t + 1].contiguous(), pos[b:b + 1] + t, None if table is None else table[b:b + 1], 1, 1
    if made is None:
        outer, tail = (c["shape"][0] if c["ps"] is not None else B), tuple(c["shape"][1:])
        big = [torch.full((n + 2,) + s, FILL, dtype=U8, device=device) for n, s in
               ((B, (T, H + 2 * Hkv if layout == "rq_in_qkv" else H, D)), (outer, tail), (outer, tail))]
        if layout == "token_major":
            big[1:] = [t.reshape(t.shape[0], t.shape[2], t.shape[1], D).permute(0, 2, 1, 3) for t in big[1:]]
        guards = [t[i] for t in big for i in (0, -1)]
        rq, kc, vc = (t[1:-1] for t in big)
        if layout == "rq_in_qkv":
            guards.append(rq[:, :, H:])
            rq = rq[:, :, :H]
        to = lambda t: t.to(device) if isinstance(t, torch.Tensor) else t
        made = ((to(x), *map(to, c["lin"]), to(c["cos"]), to(c["sin"]), *map(to, c["rot"][:2]), *c["rot"][2], c["mid"], H, Hkv, kc, vc, to(pos),
                 to(table)), (rq, kc, vc), guards)
    args, (rq, kc, vc), guards = made
    return fn(*args, out=rq), kc, vc, guards, made


def assert_row(c, device, b, t, fn=None):
    """the call on row (b, t) alone writes that row's bytes and nothing else"""
    got = call(c, device, fn=fn, row=(b, t))[:3]
    q_on, k_on, v_on, outer, tok = c["at"][b][t]
    want = [torch.full(g.shape, FILL, dtype=g.dtype) for g in got]
    o = outer if c["ps"] is not None else 0
    for on, i in ((k_on, 1), (v_on, 2)):
        if on:
            want[i][o, :, tok] = c["want"][i][outer, :, tok]
    if q_on:
        want[0][0, 0] = c["want"][0][b, t]
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want)), (b, t)


@pytest.mark.parametrize("spec", CASES, ids=ident)
def test_cpu_path_equals_the_plain_reference(spec):
    c = case(*spec)
    rq, kc, vc, guards, _ = call(c)
    assert all(torch.equal(g, w) for g, w in zip((rq, kc, vc), c["want"])) and all(bool((g == FILL).all()) for g in guards)
    # the registered op: the same caches; rq comes from torch.empty, so only its written rows are defined
    rq2, kc2, vc2, _, _ = call(c, fn=lambda *a, out: OPS.lsq_linear_packed_q8_rope_q(*a))
    written = torch.tensor([[row[0] for row in rows] for rows in c["at"]])
    assert torch.equal(rq2[written], c["want"][0][written]) and torch.equal(kc2, c["want"][1]) and torch.equal(vc2, c["want"][2])


def module(c, route, rope_epilogue, device="cpu"):
    """a case's projection and rotation as a QKVRotaryPackedA8Q and an empty cache of `route`"""
    from torchlsq.quantized import KVCacheW8, PackedLinearA8Q, PagedKVCacheW8, QKVRotaryPackedA8Q, RotaryW8Q
    B, T, H, Hkv, D = c["dims"]
    p, (osc, osh), rng = c["packed"], c["lin"][8:10], c["qkv_rng"]
    qkv = PackedLinearA8Q(p.shape[1], p.shape[0], p.bits, p.group_size, p.quant_min, output_range=rng, mid_dtype=c["mid"])
    qkv.codes, qkv.scale, qkv.zero_point = p.codes.reshape(p.shape[0], -1), p.scale.reshape(p.shape[0], -1), p.zero_point.reshape(p.shape[0], -1)
    qkv.bias = torch.nn.Parameter(c["bias"].clone(), requires_grad=False)
    qkv.output_scale, qkv.output_shift = osc.clone(), osh.clone()
    rot = RotaryW8Q(None, D, P, rotary_dim=2 * c["cos"].shape[1], mid_dtype=c["mid"])
    rot.output_scale, rot.output_shift, rot.output_range = c["rot"][0].clone(), c["rot"][1].clone(), c["rot"][2]
    cache = KVCacheW8(B, Hkv, TMAX, D) if route == "dense" else PagedKVCacheW8(B * 2 + 1, Hkv, 16, D, B, 2)
    return QKVRotaryPackedA8Q(qkv, rot, H, Hkv, rope_epilogue=rope_epilogue).eval().to(device), cache.to(device)


def module_steps(c, route, rope_epilogue, device="cpu", wrap=None):
    """a prompt of T - 2 tokens, then two steps -> every tensor the last call returns, and the final lengths"""
    m, cache = module(c, route, rope_epilogue, device)
    s_x, zx = (t.to(device) for t in c["lin"][:2])
    T = c["dims"][1]
    for a, b in ((0, T - 2), (T - 2, T - 1), (T - 1, T)):
        x = F.LevelsTensor(c["x"][:, a:b].contiguous().to(device), s_x, zx, 0, 255)
        rq, kl, vl, lens = (wrap or (lambda f, *args: f(*args)))(m, x, cache)
    return (rq.levels, rq.scale, rq.zero_point, kl.levels, kl.scale, kl.zero_point, vl.levels, vl.scale, vl.zero_point, lens.clone())


@pytest.mark.parametrize("route", ["dense", "paged"])
def test_module_with_the_epilogue_equals_its_children_one_by_one(route):
    c = case(*CASES[4])                             # [2, 3, K]: a prompt of one token (2 rows), then two steps
    outs = [module_steps(c, route, flag) for flag in (True, False)]
    assert outs[0][-1].tolist() == [3, 3] and all(torch.equal(a, b) for a, b in zip(*outs)) and len(outs[0][0].unique()) > 16


def test_state_dict_keys_are_the_childrens():
    m, _ = module(case(*CASES[0]), "dense", None)
    keys = {"qkv." + k for k in m.qkv.state_dict()} | {"rotary." + k for k in m.rotary.state_dict()}
    assert set(m.state_dict()) == keys and m.rope_epilogue is None and F.W4A8_ROPE_EPILOGUE_DEFAULT in (True, False)
    m.rope_epilogue = True
    other, _ = module(case(*CASES[0]), "dense", None)
    other.load_state_dict(m.state_dict())
    assert other.rope_epilogue is True and set(m.state_dict()) == keys | {"_extra_state"}


FIXED = 2 * 16384 + 4 * 256 + 512       # two regions of partial sums, four byte tiles, the placement


@pytest.mark.parametrize("args, kw, want", [
    ((1, 1, 32, 8, 128, 4096, 128, 4), dict(P=64, Tmax=64), dict(served=True, block=1024, grid=192, chunks=1, x_resident=True, rotate_items=160,
                                                                 pass_items=0, copy_items=32, lds_bytes=FIXED + 4112 + 32 * 4)),
    ((2, 3, 2, 2, 64, 4224, 32, 4), dict(R=32, P=64, pages=(9, 16, 4)), dict(served=True, grid=12, chunks=2, x_resident=False, rotate_items=4,
                                                                             pass_items=4, copy_items=4, lds_bytes=FIXED + 6 * 4112 + 6 * 128 * 4)),
    ((17, 1, 2, 2, 64, 128, 128, 4), dict(P=8, Tmax=8), dict(served=False, grid=0, block=0, lds_bytes=0, rotate_items=0)),
    ((1, 1, 2, 2, 48, 128, 128, 4), dict(R=32, P=8, Tmax=8), dict(served=False)),
    ((1, 1, 2, 2, 64, 128, 128, 4), dict(R=16, P=8, Tmax=8), dict(served=False)),
    ((1, 1, 2, 2, 64, 128, 128, 4), dict(P=8, Tmax=8, interleaved=True), dict(served=False)),
    ((1, 1, 2, 2, 64, 96, 48, 4), dict(P=8, Tmax=8), dict(served=False)),
    ((1, 1, 2, 2, 64, 128, 128, 4), dict(P=8, Tmax=8, aligned=False), dict(served=False)),
    ((1, 1, 2, 2, 64, 128, 128, 4), dict(P=8, Tmax=8, q_strides=(256, 256, 72)), dict(served=False)),
])
def test_plan(args, kw, want):
    pl = extension.linrope_w4_plan(*args, **kw)
    assert {k: pl[k] for k in want} == want, pl


@pytest.mark.parametrize("kw, message", [
    (dict(R=31), "must be even"), (dict(R=96), "at most D"), (dict(P=0), "at least 1"), (dict(pages=(4, 0, 2)), "at least 1"),
    (dict(q_strides=(256, 256, 32)), "overlap"), (dict(bits=3), "bits must be 4 or 2"), (dict(group_size=96), "not a multiple of group_size"),
])
def test_refusals(kw, message):
    kw = dict(dict(P=8, Tmax=8, group_size=128, bits=4), **kw)
    with pytest.raises(RuntimeError, match=message):
        extension.linrope_w4_plan(1, 2, 2, 2, 64, 128, kw.pop("group_size"), kw.pop("bits"), **kw)
    with pytest.raises(Exception, match="k_cache must hold"):
        call(case(*CASES[0]), fn=lambda *a, out: extension.linrope_w4_q(*a[:28], a[28].view(torch.int8), *a[29:], out=out))
