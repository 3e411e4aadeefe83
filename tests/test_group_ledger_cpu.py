"""CPU: what the group-wise ledger (tests/test_group_ledger_gpu.py) rests on and needs no device for -- the restated launch
plan against lsq_group_plan, the classifier's tags of every case at 256 CUs, the input recipe, and the CPU op on the recipe's
inputs against the oracle."""
import numpy as np
import pytest
import torch

import group_ledger_cases as C
from helpers import assert_bits_equal, check_sums
from oracle import lsq_oracle as O


def _name(dtype):
    return str(dtype).split(".")[-1]


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
def test_restated_plan_equals_the_library_plan_where_the_chip_does_not_matter(dtype):
    """form, reduction and items per group never depend on the CU count; the grids are compared for the shapes that get the
    same ones from 64 to 1024 CUs (without a device the library plans for a part it cannot ask)"""
    from torchlsq import extension as E
    V = C.vec_of(dtype)
    shapes = [(C.case_shape(c, V, 256)[2], C.case_shape(c, V, 256)[0], c) for c in C.CASES] + [(n, G, "sweep") for n, G in C.sweep(V)]
    grids = 0
    for n, G, what in shapes:
        got = E.group_plan(dtype, n, G)
        lo, hi = C.plan(V, n, G, 64), C.plan(V, n, G, 1024)
        assert (got["form"], got["reduction"], got["lanes_per_group"], got["vec"]) == (lo["form"], lo["reduction"], lo["items_per_group"], V), (what, n, G, got)
        if (lo["fwd_grid"], lo["bwd_grid"]) == (hi["fwd_grid"], hi["bwd_grid"]):
            assert (got["fwd_grid"], got["bwd_grid"]) == (lo["fwd_grid"], lo["bwd_grid"]), (what, n, G, got, lo)
            grids += 1
    assert grids >= 100


def test_every_case_has_its_tags_at_256_cus_and_the_cases_cover_the_list():
    covered = {"fwd/elem/misaligned-levels"}          # (the C-entry test of the GPU file: no shape gives it)
    for V in (2, 4, 8):
        per_v = set()
        for case in C.CASES:
            per_v |= C.case_tags(case, V, 256)
        for t in C.NEW_BRANCHES:
            assert t in per_v, (V, t)
        covered |= per_v
    assert covered == set(C.ALL_TAGS), (sorted(set(C.ALL_TAGS) - covered), sorted(covered - set(C.ALL_TAGS)))
    # the wave ranges of the restated plan tile the groups: every group in exactly one wave's range
    for case in C.SMALL:
        G, groups, n = C.case_shape(case, 4, 256)
        p = C.plan(4, n, G, 256)
        seen = [q for w in range(p["bwd_grid"] * C.WAVES) for r in C.wave_range(p, w) for q in r]
        assert sorted(seen) == list(range(groups)), case
        assert all(C.wave_range(p, w) for w in range(C.busy_waves(p))) and not C.wave_range(p, p["bwd_grid"] * C.WAVES), case


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
def test_recipe_puts_the_edge_values_where_it_says(dtype):
    V = C.vec_of(dtype)
    for case in C.SMALL:
        G, groups, n = C.case_shape(case, V, 256)
        x, g, gb, s, b, edge = C.make_inputs(V, G, groups, dtype, 256)
        assert x.shape == g.shape == gb.shape == (n,) and s.shape == b.shape == (groups,)
        xe = torch.cat([x[q * G:(q + 1) * G] for q in edge]).double()
        assert int(torch.isnan(xe).sum()) == 1 and int(torch.isinf(xe).sum()) == 2, case
        for v in (-1.5, 2.25, 1.125, C.TINY[dtype]):
            assert bool((xe == float(torch.tensor(v, dtype=dtype))).any()), (case, v)
        assert bool(((xe == 0) & torch.signbit(xe)).any()), case
        assert x[0] != x[0] and (G < 2 or bool(torch.isinf(x[G - 1]))), case          # first and last element of group 0
        assert float(s[2]) < 0 and float(s[3]) == 0 and 0 < float(s[5]) < 1e-29
        assert bool(torch.isinf(g[2 * G - 1])) and float(x[2 * G - 1]) == 100.0 and bool(torch.isnan(g[4 * G:5 * G].float()).any())
        assert bool(torch.isnan(x[(groups - 1) * G:].float()).any())
        # the border gradient: the plain one plus non-finite values, in the first and last group of every wave's range
        diff = torch.nonzero(g.view(torch.uint8).view(n, -1).ne(gb.view(torch.uint8).view(n, -1)).any(1)).reshape(-1)
        assert len(diff) and not bool(torch.isfinite(gb[diff].float()).any()), case
        p = C.plan(V, n, G, 256)
        ends = {q for w in range(C.busy_waves(p)) for q in (C.wave_range(p, w)[0][0], C.wave_range(p, w)[-1][-1])}
        assert {int(i) // G for i in diff} <= ends, case


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=_name)
def test_cpu_op_equals_the_oracle_on_the_recipe(dtype):
    from torchlsq import extension  # noqa: F401
    V = C.vec_of(dtype)
    for case in C.SMALL:
        G, groups, n = C.case_shape(case, V, 256)
        x, g, gb, s, b, _ = C.make_inputs(V, G, groups, dtype, 256)
        xn, sn, bn = x.numpy(), s.numpy(), b.numpy()
        for grad, (sym, ev, init) in ((g, (False, False, False)), (gb, (True, False, False)), (gb, (False, True, False)), (g, (False, False, True))):
            args = (*C.Q, True, 1.0, sym, ev, init)
            y = torch.ops.torchlsq.lsq_forward_per_group(x, s, b, G, *args)
            dx, ds, db = torch.ops.torchlsq.lsq_backward_per_group(grad, x, s, b, G, *args)
            r = O.bwd_pc(grad.numpy(), xn, sn, bn, 1, groups, G, *args)
            what = "%s %s sym=%d eval=%d init=%d" % (case, _name(dtype), sym, ev, init)
            assert_bits_equal(y.numpy(), O.fwd_pc(xn, sn, bn, 1, groups, G, *C.Q, init_mode=init), what + " y")
            assert_bits_equal(dx.numpy(), r.dx, what + " dx")
            check_sums(ds, r.ds_wide, r.abs_ds, what + " d_scale")
            check_sums(db, r.db_wide, r.abs_db, what + " d_shift")
        lv = torch.ops.torchlsq.lsq_levels_per_group(x, s, b, G, *C.Q, 0)
        assert np.array_equal(lv.numpy().astype(np.int32).reshape(-1), O.levels_pc(xn, sn, bn, 1, groups, G, *C.Q).reshape(-1)), case
