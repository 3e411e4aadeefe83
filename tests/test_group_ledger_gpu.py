"""GPU: the group-wise ledger -- every shape-dependent branch of the two kernel bodies of liblsq_hip_group.so
(csrc/group/lsq_grp_fwd_body.inc, lsq_grp_bwd_body.inc) is driven by a constructed case and held to the CPU oracle there.

tests/group_ledger_cases.py holds the table: the restated launch plan (held to extension.group_plan here, with the device's
CU count), the classifier that names the branches a shape takes, the cases and the input recipe.  A case asserts the tags it
is in the table for before it runs, and counts for its tags only after its calls agreed with the oracle:
  * y, dx and the int8 levels bit for bit against oracle.lsq_oracle on [1, n / G, G] (16-bit storage: the oracle's fp32 result
    rounded to the storage type, NaNs where the oracle's are);
  * d_scale / d_shift within 1e-6 of sum|terms| on the finite groups, and with the oracle's NaN / +-inf pattern on the poisoned
    ones: a non-finite term stayed inside its group;
  * eval mode: zero sums; init mode: y and dx carry x's and grad's own bits.
The small cases run in all four storage types and all 16 modes (sym, eval, init, use_grad_scaling), on two gradients (with
and without the poisoned border groups of the waves' ranges, see make_inputs), through the fused call and through
lsq_per_group's eval path; the chip-sized ones in fp32 and bf16, affine training and eval, with the oracle on windows of
whole groups where the tensor is large.  The last test asserts that the tags of the held cases are the whole list, and prints
the ledger."""
import ctypes
import itertools
import time

import numpy as np
import pytest
import torch
import torchlsq  # noqa: F401  (registers torch.ops.torchlsq.*)

import group_ledger_cases as C
from helpers import assert_bits_equal, check_sums, same_stored
from oracle import lsq_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
Q = C.Q
MODES = list(itertools.product([False, True], [False, True], [False, True], [False, True]))   # sym, eval, init, use_gs
TRAIN = (*Q, True, 1.0, False, False, False)
EVAL = (*Q, True, 1.0, False, True, False)

LEDGER = {}       # tag -> every held run that drove it: (case, dtype)
TIMES = {}


def _name(dtype):
    return str(dtype).split(".")[-1]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _np(t):
    return (t.float() if t.dtype in (torch.bfloat16, torch.float16) else t).cpu().numpy()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy()


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), what + ": the bits differ"


def _assert_plan(dtype, n, G, cus):
    from torchlsq import extension as E
    p, got = C.plan(C.vec_of(dtype), n, G, cus), E.group_plan(dtype, n, G)
    for k, key in (("form", "form"), ("reduction", "reduction"), ("lanes_per_group", "items_per_group"), ("fwd_grid", "fwd_grid"),
                   ("bwd_grid", "bwd_grid")):
        assert got[k] == min(p[key], 2 ** 31 - 1) if k == "lanes_per_group" else got[k] == p[key], (dtype, n, G, k, got, p)
    return p


def _held(case, dtype, tags):
    for t in tags:
        LEDGER.setdefault(t, []).append((case, _name(dtype)))


def _levels(x, s, b, G, with_y):
    from torchlsq import extension as E
    if with_y:
        return E.group_forward(x, s, b, G, *TRAIN, levels_bias=0)
    return None, E.group_forward(x, s, b, G, *TRAIN, levels_bias=0, levels_only=True)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
def test_restated_plan_equals_the_library_plan(dtype):
    cus, V = _cus(), C.vec_of(dtype)
    for case in C.CASES:
        G, groups, n = C.case_shape(case, V, cus)
        _assert_plan(dtype, n, G, cus)
    for n, G in C.sweep(V):
        _assert_plan(dtype, n, G, cus)


@pytest.mark.parametrize("case,dtype", [pytest.param(c, d, id="%s-%s" % (c, _name(d))) for c in C.SMALL for d in C.DTYPES])
def test_small_case_equals_the_oracle(case, dtype):
    from torchlsq import extension as E
    from torchlsq.functional import lsq_per_group
    t0 = time.perf_counter()
    cus, V = _cus(), C.vec_of(dtype)
    G, groups, n = C.case_shape(case, V, cus)
    tags = C.case_tags(case, V, cus)
    _assert_plan(dtype, n, G, cus)
    x, g, gb, s, b, _ = C.make_inputs(V, G, groups, dtype, cus)
    xd, sd, bd = x.to(DEV), s.to(DEV), b.to(DEV)
    grads = {True: (g, g.to(DEV), _np(g)), False: (gb, gb.to(DEV), _np(gb))}       # by use_grad_scaling
    xn, sn, bn = _np(x), s.numpy(), b.numpy()
    oy = {init: O.fwd_pc(xn, sn, bn, 1, groups, G, *Q, init_mode=init) for init in (False, True)}
    olv = O.levels_pc(xn, sn, bn, 1, groups, G, *Q)
    for k, (sym, ev, init, ugs) in enumerate(MODES):
        gsc = 0.5 if k % 3 else 1.0
        args = (*Q, ugs, gsc, sym, ev, init)
        what = "%s %s sym=%d eval=%d init=%d ugs=%d" % (case, _name(dtype), sym, ev, init, ugs)
        gc, gd, gn = grads[ugs]
        y = E.group_forward(xd, sd, bd, G, *args)
        dx, ds, db = E.group_backward(gd, xd, sd, bd, G, *args)
        torch.cuda.synchronize()
        r = O.bwd_pc(gn, xn, sn, bn, 1, groups, G, *Q, ugs, gsc, sym, ev, init)
        same_stored(y, oy[init], dtype, what + " y")
        same_stored(dx, r.dx, dtype, what + " dx")
        if init:
            assert_bits_equal(_bits(y), _bits(x), what + " y carries x's bits")
            assert_bits_equal(_bits(dx), _bits(gc), what + " dx carries grad's bits")
        if ev:
            assert not ds.cpu().numpy().any() and not db.cpu().numpy().any(), what + " eval mode: zero sums"
        check_sums(ds, r.ds_wide, r.abs_ds, what + " d_scale")
        check_sums(db, r.db_wide, r.abs_db, what + " d_shift")
        if k in (0, 1):       # (affine training on the border gradient and on the plain one): the fused call, one item
            (fy,) = E.group_forward_multi([xd], [sd], [bd], [G], *args)
            ((fdx, fds, fdb),) = E.group_backward_multi([gd], [xd], [sd], [bd], [G], *args)
            for a, c, nm in ((fy, y, "y"), (fdx, dx, "dx"), (fds, ds, "d_scale"), (fdb, db, "d_shift")):
                _same_bits(a, c, what + " fused single-item list " + nm)
    # the int8 levels, with and without y
    for with_y in (True, False):
        y, lv = _levels(xd, sd, bd, G, with_y)
        assert np.array_equal(lv.cpu().numpy().astype(np.int32).reshape(-1), olv.reshape(-1)), "%s levels (y: %d)" % (case, with_y)
        if with_y:
            same_stored(y, oy[False], dtype, case + " y next to levels")
    # eval through lsq_per_group: the forward saves the inside mask, the backward is hip_backward_from_mask -- the eval
    # kernel's dx bits, the NaN and the two border elements of x included
    assert E.saves_mask(True, False, True, True)
    xs = xd.clone().requires_grad_(True)
    y = lsq_per_group(xs, sd, bd, G, *Q, eval_mode=True)
    y.backward(grads[True][1])
    kdx = E.group_backward(grads[True][1], xd, sd, bd, G, *EVAL)[0]
    torch.cuda.synchronize()
    same_stored(y.detach(), oy[False], dtype, case + " lsq_per_group eval y")
    _same_bits(xs.grad, kdx, case + " lsq_per_group eval dx against the eval kernel's")
    _held(case, dtype, tags)
    TIMES[(case, dtype)] = time.perf_counter() - t0


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
def test_small_cases_in_one_fused_list_equal_their_single_calls(dtype):
    """every small case as an item of one mixed list: the *_multi_kernel instantiations of all three reductions, bit for bit"""
    from torchlsq import extension as E
    cus, V = _cus(), C.vec_of(dtype)
    xs, gs, ss, bs, Gs = [], [], [], [], []
    for case in C.SMALL:
        G, groups, n = C.case_shape(case, V, cus)
        x, g, gb, s, b, _ = C.make_inputs(V, G, groups, dtype, cus)
        xs.append(x.to(DEV)), gs.append(gb.to(DEV)), ss.append(s.to(DEV)), bs.append(b.to(DEV)), Gs.append(G)
    per, launches = E.group_multi_plan(dtype, [x.numel() for x in xs], Gs)
    assert launches == 3 and max(sum(1 for p in per if p[0] == k) for k in range(3)) <= E.GROUP_MULTI_ITEMS
    for args in (TRAIN, (*Q, True, 1.0, True, False, False), EVAL, (*Q, False, 1.0, False, False, True)):
        ys = E.group_forward_multi(xs, ss, bs, Gs, *args)
        outs = E.group_backward_multi(gs, xs, ss, bs, Gs, *args)
        torch.cuda.synchronize()
        for case, x, g, s, b, G, y, (dx, ds, db) in zip(C.SMALL, xs, gs, ss, bs, Gs, ys, outs):
            what = "%s %s in the mixed list %r" % (case, _name(dtype), args[4:])
            _same_bits(y, E.group_forward(x, s, b, G, *args), what + " y")
            for a, c, nm in zip((dx, ds, db), E.group_backward(g, x, s, b, G, *args), ("dx", "d_scale", "d_shift")):
                _same_bits(a, c, what + " " + nm)


def _windows(p, groups):
    """three stretches of whole groups: the start, the tiles (blocks) on both sides of the forward's second trip -- item
    fwd_grid * tile; the middle of the tensor where there is no second trip -- and the tail"""
    G = p["G"]
    per_trip = (C.TILE * p["V"] if p["form"] == "packet" else C.BLOCK) * p["fwd_grid"]
    span = C.TILE * p["V"] if p["form"] == "packet" else 4 * C.BLOCK
    w = max(2, -(-2 * span // G))
    mid = per_trip if per_trip + span < p["n"] else p["n"] // 2
    lo = max(0, (mid - span) // G)
    out = [(0, min(w, groups)), (lo, min(groups, lo + w + 1)), (max(0, groups - w), groups)]
    return out


@pytest.mark.parametrize("case,dtype", [pytest.param(c, d, id="%s-%s" % (c, _name(d))) for c in C.CHIP
                                        for d in (torch.float32, torch.bfloat16)])
def test_chip_sized_case_equals_the_oracle(case, dtype):
    from torchlsq import extension as E
    t0 = time.perf_counter()
    cus, V = _cus(), C.vec_of(dtype)
    G, groups, n = C.case_shape(case, V, cus)
    tags = C.case_tags(case, V, cus)
    p = _assert_plan(dtype, n, G, cus)
    x, _, g, s, b, _ = C.make_inputs(V, G, groups, dtype, cus, waves="few")
    xd, gd, sd, bd = x.to(DEV), g.to(DEV), s.to(DEV), b.to(DEV)
    x2, g2 = xd.view(groups, G), gd.view(groups, G)
    what = "%s %s" % (case, _name(dtype))
    # forward and levels: the oracle on the windows, the per-channel op on the [n / G, G] view everywhere
    y, lv = E.group_forward(xd, sd, bd, G, *TRAIN, levels_bias=0)
    edx, eds, edb = E.group_backward(gd, xd, sd, bd, G, *EVAL)
    cy, clv = E.hip_forward_per_channel(x2, sd, bd, 0, *TRAIN, levels_bias=0)
    cedx = E.hip_backward_per_channel(g2, x2, sd, bd, 0, *EVAL)[0]
    _same_bits(y, cy.view(-1), what + " y against the per-channel op")
    _same_bits(lv, clv.view(-1), what + " levels against the per-channel op")
    _same_bits(edx, cedx.view(-1), what + " eval dx against the per-channel op")
    assert not bool(eds.any()) and not bool(edb.any()), what + " eval mode: zero sums"
    sn, bn = s.numpy(), b.numpy()
    for lo, hi in _windows(p, groups):
        sl, k = slice(lo * G, hi * G), hi - lo
        xw, gw = _np(x[sl]), _np(g[sl])
        win = what + " groups [%d, %d)" % (lo, hi)
        same_stored(y[sl], O.fwd_pc(xw, sn[lo:hi], bn[lo:hi], 1, k, G, *Q), dtype, win + " y")
        assert np.array_equal(lv[sl].cpu().numpy().astype(np.int32), O.levels_pc(xw, sn[lo:hi], bn[lo:hi], 1, k, G, *Q).reshape(-1)), win + " levels"
        same_stored(edx[sl], O.bwd_pc(gw, xw, sn[lo:hi], bn[lo:hi], 1, k, G, *EVAL).dx, dtype, win + " eval dx")
    del cy, clv, cedx, edx, y, lv
    # training: dx everywhere and the sums of every group against the oracle
    dx, ds, db = E.group_backward(gd, xd, sd, bd, G, *TRAIN)
    torch.cuda.synchronize()
    r = O.bwd_pc(_np(g), _np(x), sn, bn, 1, groups, G, *TRAIN)
    same_stored(dx, r.dx, dtype, what + " dx")
    check_sums(ds, r.ds_wide, r.abs_ds, what + " d_scale")
    check_sums(db, r.db_wide, r.abs_db, what + " d_shift")
    assert int(np.isfinite(r.ds_wide).sum()) > groups - 64      # (the recipe poisons a handful of groups)
    _held(case, dtype, tags)
    TIMES[(case, dtype)] = time.perf_counter() - t0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_name)
def test_c_entry_with_an_offset_levels_pointer(dtype):
    """lsq_group_forward with a levels pointer one byte past a packet's alignment: forward_per_group sends the packet plan to
    the element form (torch-made buffers are aligned, so only a C caller gets there).  Status 0, the aligned call's bytes --
    which are the oracle's -- and untouched guard bytes on both sides; with y and with y = NULL; int8 levels and, with a
    level_bias, uint8 ones."""
    from torchlsq import extension as E
    lib = E.group_library()
    cus, V = _cus(), C.vec_of(dtype)
    G, groups = 8 * V, 37
    n = G * groups
    assert "fwd/packet/pg_shift" in C.tags(V, n, G, cus)
    code = {torch.float32: E.LSQ_F32, torch.bfloat16: E.LSQ_BF16}[dtype]
    x, _, _, s, b, _ = C.make_inputs(V, G, groups, dtype, cus)
    xd, bd = x.to(DEV), b.to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    FILL, OFF, PAD = 0x5A, 17, 64
    # (int8 levels; then a level_bias that makes them uint8: [-128, 127] + 128, on scales small enough to use the range)
    for q, bias, scale in ((Q, 0, s), ((-128, 127, -128, 127), -128, s.abs().clamp(min=0.05) * 0.02)):
        sd = scale.to(DEV)
        params = E.LsqParams(*q, 1, 0, 0, 0, 1.0, 0)
        want = O.levels_pc(_np(x), scale.numpy(), b.numpy(), 1, groups, G, *q).reshape(-1) - bias
        want_y = O.fwd_pc(_np(x), scale.numpy(), b.numpy(), 1, groups, G, *q)
        if bias:
            assert want.max() > 127 and want.min() >= 0

        def call(levels_ptr, y):
            ex = E.LsqFwdExtras(levels_ptr, bias, 0)
            rc = lib.lsq_group_forward(code, xd.data_ptr(), None if y is None else y.data_ptr(), n, G, sd.data_ptr(), bd.data_ptr(),
                                       ctypes.byref(params), ctypes.byref(ex), stream)
            torch.cuda.synchronize()
            assert rc == 0, lib.lsq_group_last_error()

        aligned = torch.full((n,), FILL, dtype=torch.uint8, device=DEV)
        assert aligned.data_ptr() % V == 0
        call(aligned.data_ptr(), None)
        got = aligned.cpu().numpy()
        assert np.array_equal((got if bias else got.view(np.int8)).astype(np.int32), want), "aligned levels %r" % (q,)
        for with_y in (True, False):
            buf = torch.full((n + PAD,), FILL, dtype=torch.uint8, device=DEV)
            assert buf.data_ptr() % 16 == 0 and (buf.data_ptr() + OFF) % V == 1
            y = torch.empty_like(xd) if with_y else None
            call(buf.data_ptr() + OFF, y)
            h = buf.cpu().numpy()
            what = "%s %r bias %d y: %d" % (_name(dtype), q, bias, with_y)
            assert (h[:OFF] == FILL).all() and (h[OFF + n:] == FILL).all(), what + ": guard bytes were written"
            assert np.array_equal(h[OFF:OFF + n], got), what + ": level bytes differ from the aligned call's"
            if with_y:
                same_stored(y, want_y, dtype, what + " y")
    _held("c_entry_offset_levels", dtype, {"fwd/elem/misaligned-levels"})


def test_ledger_every_branch_tag_is_covered():
    """the tags of the held cases are the whole list of group_ledger_cases.ALL_TAGS (NO_CASE names what no shape reaches),
    and the three branches no test ran before this file are held in every storage type"""
    print("\ngroup ledger: %d tags, %d covered, %d held runs in %.1f s on %d CUs" %
          (len(C.ALL_TAGS), len(set(LEDGER) & set(C.ALL_TAGS)), len(TIMES), sum(TIMES.values()), _cus()))
    for t in C.ALL_TAGS:
        runs = LEDGER.get(t, [])
        print("  %-42s <- %s  (%d runs)" % (t, "%s %s" % runs[0] if runs else "NOTHING", len(runs)))
    for what, why in C.NO_CASE.items():
        print("  no case: %s -- %s" % (what, why))
    slow = sorted(((v, k) for k, v in TIMES.items()), reverse=True)[:5]
    print("  slowest: " + ", ".join("%s %s %.2f s" % (k[0], _name(k[1]), v) for v, k in slow))
    missing = sorted(set(C.ALL_TAGS) - set(LEDGER))
    assert not missing, "branches that no oracle-checked case drove: %s" % missing
    assert set(LEDGER) == set(C.ALL_TAGS), sorted(set(LEDGER) - set(C.ALL_TAGS))
    for t in C.NEW_BRANCHES:
        have = {d for _, d in LEDGER[t]}
        assert have == {_name(d) for d in C.DTYPES}, "%s is held in %s only" % (t, sorted(have))
