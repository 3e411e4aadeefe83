"""What tests/test_attn_paged_w8_cpu.py and tests/test_attn_paged_w8_gpu.py share: a dense decode case of `attn_decode_w8_cases` (its
`want` is the definition, the parent commit's code) scattered into the pages of two pools under a block table, so that the gather of
the pools IS the case's k and v; the paged op run on a device of choice, the library's C entry called directly with a caller-made
workspace and guard bytes, and the plan.  Pages the table does not name, and whatever else a test wants, hold the byte `fill`.
Everything is seeded.
"""
import ctypes

import torch

import attn_decode_w8_cases as C
import attn_w8_cases as A

U8, I8, F32, BF16, F16 = A.U8, A.I8, A.F32, A.BF16, A.F16
GUARD = C.GUARD
LSQ_EINVAL = -1
Z3 = (A.QKV_Z,) * 3
SIGNED_PV = (True, False, False)       # fitted int8 probabilities and context: many keys leave a quint8 probability few levels


class Paged:
    """k_pool, v_pool: LevelsTensors [Np, Hkv, ps, D] on the CPU (views of storage in `order`); table: int32 [B, Mp] (a view of a
    [B, Mp + bt_pad] buffer); ps, Mp, Np"""


def tables(B, Mp, Np, kind, seed=0):
    """an int64 [B, Mp] table of distinct pages below Np: "perm" a seeded random permutation, "rev" the last pages first, "ident" the
    first pages in order"""
    assert Np >= B * Mp
    if kind == "perm":
        pages = torch.randperm(Np, generator=A.gen(300 + seed))[:B * Mp]
    elif kind == "rev":
        pages = torch.arange(Np - 1, Np - 1 - B * Mp, -1)
    else:
        pages = torch.arange(B * Mp)
    return pages.reshape(B, Mp).to(torch.int64)


def pool_of(dense, table, ps, Np, order="hsd", fill=0x3C):
    """dense [B, Hkv, Mp ps, D] levels scattered into a pool [Np, Hkv, ps, D] under `table` (int64 [B, Mp], entries in range); `order`
    "hsd": storage [Np, Hkv, ps, D]; "shd": storage [Np, ps, Hkv, D], the pool its permuted view"""
    B, Hkv, Tk, D = (int(n) for n in dense.shape)
    Mp = Tk // ps
    shape = (Np, Hkv, ps, D) if order == "hsd" else (Np, ps, Hkv, D)
    store = torch.full(shape, fill, dtype=U8).view(dense.dtype)
    pool = store if order == "hsd" else store.permute(0, 2, 1, 3)
    pool[table.reshape(-1)] = dense.reshape(B, Hkv, Mp, ps, D).permute(0, 2, 1, 3, 4).reshape(B * Mp, Hkv, ps, D)
    return pool


def paged(c, ps, kind="perm", order="hsd", extra=3, bt_pad=0, seed=0, table=None, fill=0x3C):
    """the case's k and v in pools of B Mp + `extra` pages; `table`: an int64 [B, Mp] table to use instead (entries may repeat only
    where the dense rows agree)"""
    B, H, Hkv, Tq, Tk, D = c.shape
    assert Tk % ps == 0
    Mp = Tk // ps
    pg = Paged()
    pg.ps, pg.Mp, pg.Np = ps, Mp, B * Mp + extra
    t = tables(B, Mp, pg.Np, kind, seed) if table is None else table
    buf = torch.full((B, Mp + bt_pad), -7, dtype=torch.int32)
    buf[:, :Mp] = t.to(torch.int32)
    pg.table = buf[:, :Mp]
    pg.k_pool = C.with_levels(c.k, pool_of(c.k.levels, t, ps, pg.Np, order, fill))
    pg.v_pool = C.with_levels(c.v, pool_of(c.v.levels, t, ps, pg.Np, order, fill))
    return pg


def gathered(pg, table=None):
    from torchlsq.functional import lsq_kv_gather_paged_w8
    t = pg.table if table is None else table
    return lsq_kv_gather_paged_w8(pg.k_pool, t), lsq_kv_gather_paged_w8(pg.v_pool, t)


def pool_strides(pool):
    from torchlsq._attn_paged_w8_host import _pool_strides
    return _pool_strides(pool)


def on(dev, pg, shift=(0, 0)):
    """(k_pool, v_pool, table) of `pg` on `dev`, the pools' storage copied whole (`shift` bytes off the allocation's base)"""
    if str(dev) == "cpu":
        return pg.k_pool, pg.v_pool, pg.table
    base = torch.empty(0, dtype=torch.int32).set_(pg.table.untyped_storage()).to(dev)
    table = base.as_strided(tuple(pg.table.shape), tuple(pg.table.stride()), pg.table.storage_offset())
    return C.moved(pg.k_pool, dev, shift[0]), C.moved(pg.v_pool, dev, shift[1]), table


def run(c, pg, dev, splits=0, shift=(0, 0), q_shift=0, table=None, lengths="case", operands=None):
    """`lsq_attention_decode_paged_w8_q` of the case on `dev` -> the levels [B, Tq, H D]; `operands`: (k_pool, v_pool, table) already on
    `dev` to use instead"""
    from torchlsq.functional import lsq_attention_decode_paged_w8_q
    kp, vp, bt = on(dev, pg, shift) if operands is None else operands
    if table is not None:
        bt = table.to(dev)
    lens = c.lengths if isinstance(lengths, str) else lengths
    return lsq_attention_decode_paged_w8_q(C.moved(c.q, dev, q_shift), kp, vp, bt, c.table.to(dev), *C.F.sides_on(c.sides, dev), c.mid,
                                           causal=c.causal, key_lengths=None if lens is None else lens.to(dev), splits=splits).levels


def plan_of(c, pg, splits=0, qkv_aligned=True, y_aligned=True):
    from torchlsq import extension as E
    B, H, Hkv, Tq, Tk, D = c.shape
    on_, off = C.causal_args(c)
    return E.attn_paged_w8_plan(B, H, Hkv, Tq, D, pg.Np, pg.ps, pg.Mp, splits, bt_ld=int(pg.table.stride(0)) if B > 1 else pg.Mp,
                                q_strides=C.F.strides(c.q.levels), k_strides=pool_strides(pg.k_pool.levels),
                                v_strides=pool_strides(pg.v_pool.levels), qkv_aligned=qkv_aligned, y_aligned=y_aligned,
                                q_dtype=c.q.levels.dtype, k_dtype=c.k.levels.dtype, v_dtype=c.v.levels.dtype, causal=on_, causal_offset=off,
                                has_lengths=c.lengths is not None)


def workspace(c, pg, splits, fill, dev):
    """(the workspace tensor: the reported bytes filled with `fill` and 64 guard bytes behind them, the reported size)"""
    need = plan_of(c, pg, splits)["workspace_bytes"]
    ws = torch.full((need + 64,), fill, dtype=U8, device=dev)
    ws[need:] = GUARD
    assert ws.data_ptr() % 16 == 0
    return ws, need


def c_entry(c, pg, dev, splits=0, shift=(0, 0), ws=None, fill=0xA5, y_shift=0, operands=None):
    """`lsq_attn_paged_w8_decode` called directly on the case's operands on the GPU with a caller-made workspace: no Python host, so no
    fallback -> (status, the levels [B, Tq, H D] prefilled with 0x5A, the workspace, its reported size).  `operands`: (k_pool, v_pool,
    table) already on `dev` to use instead"""
    from torchlsq import extension as E
    from torchlsq._attn_w8_host import _DTYPE_CODE, _LEVEL_CODE
    from torchlsq.functional import _act_constants
    B, H, Hkv, Tq, Tk, D = c.shape
    q = C.moved(c.q, dev)
    kp, vp, bt = on(dev, pg, shift) if operands is None else operands
    sides, tab = C.F.sides_on(c.sides, dev), c.table.to(dev)
    lens = None if c.lengths is None else c.lengths.to(dev)
    raw = torch.full((B * Tq * H * D + 32,), GUARD, dtype=U8, device=dev)
    y = raw[y_shift:y_shift + B * Tq * H * D].view(B, Tq, H * D).view(c.want.dtype)
    guard_from = None                                   # a workspace the caller made: the caller checks its guard bytes
    if ws is None:
        ws, need = workspace(c, pg, splits, fill, dev)
        guard_from = need
    else:
        need = plan_of(c, pg, splits)["workspace_bytes"]
    S = E.LsqAttnW8Strides
    on_, off = C.causal_args(c)
    geom = E.LsqAttnDecodeW8Geom(B, H, Hkv, Tq, Tk, D, *(_LEVEL_CODE[x.levels.dtype] for x in (q, kp, vp)), 1 if on_ else 0, off,
                                 0 if lens is None else 1, S(*C.F.strides(q.levels)), S(*pool_strides(kp.levels)), S(*pool_strides(vp.levels)),
                                 S(*C.F.strides(y.view(B, Tq, H, D).permute(0, 2, 1, 3))))
    pages = E.LsqAttnPagedW8Pages(int(kp.shape[0]), pg.ps, pg.Mp, int(bt.stride(0)) if B > 1 else pg.Mp)
    p_s, p_z = _act_constants(sides[1][0], sides[1][1], sides[1][4], sides[1][5])
    consts = E.LsqAttnDecodeW8Consts(q.scale.data_ptr(), q.zero_point.data_ptr(), kp.scale.data_ptr(), kp.zero_point.data_ptr(),
                                     vp.scale.data_ptr(), vp.zero_point.data_ptr(), p_s.data_ptr(), p_z.data_ptr())
    outs = [E.LsqAttnW8Out(s[0].data_ptr(), s[1].data_ptr(), *s[2:], _DTYPE_CODE[c.mid]) for s in sides]
    torch.cuda.synchronize()                            # the call below goes to the default stream
    rc = E.attn_paged_w8_library().lsq_attn_paged_w8_decode(
        ctypes.byref(geom), ctypes.byref(pages), ctypes.byref(consts), *(ctypes.byref(o) for o in outs), tab.data_ptr(),
        None if lens is None else lens.data_ptr(), bt.data_ptr(), q.levels.data_ptr(), kp.levels.data_ptr(), vp.levels.data_ptr(), y.data_ptr(),
        ws.data_ptr(), need, splits, None)
    torch.cuda.synchronize()
    assert bool((raw[:y_shift] == GUARD).all()) and bool((raw[y_shift + B * Tq * H * D:] == GUARD).all()), "bytes outside y were written"
    assert guard_from is None or bool((ws[guard_from:] == GUARD).all()), "bytes behind the reported workspace were written"
    return rc, y, ws, need


def append_reference(k, v, k_pool, v_pool, table, positions):
    """the append by plain Python loops on CPU tensors (in place): WRITES SKIP"""
    B, T = int(k.shape[0]), int(k.shape[1])
    Np, ps, Mp = int(k_pool.shape[0]), int(k_pool.shape[2]), int(table.shape[1])
    for b in range(B):
        for t in range(T):
            p = (0 if positions is None else int(positions[b])) + t
            if p < 0 or p >= Mp * ps:
                continue
            e = int(table[b, p // ps])
            if e < 0 or e >= Np:
                continue
            k_pool[e, :, p % ps] = k[b, t]
            v_pool[e, :, p % ps] = v[b, t]
