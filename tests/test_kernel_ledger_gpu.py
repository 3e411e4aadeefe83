"""GPU: the kernel ledger -- every per-channel kernel instantiation that liblsq_hip.so ships is launched by a constructed case
and held to the CPU oracle there, or is listed in tests/golden/kernel_ledger_exempt.json with the lsq_pc_plan.hpp /
lsq_pc_geom.hpp condition that keeps every input away from it.  The tools build records the kernels it launches
(tools/lsq_tools.py: launched_reset / launched); a case counts for a kernel only after the call that launched it agreed with
the oracle: y / dx / int8 levels bit for bit (16-bit storage: the fp32 result rounded to the storage type), d_scale / d_shift
within 1e-6 of sum|terms| on the finite channels and with the oracle's NaN / inf pattern on the poisoned ones, zero sums in
eval mode, x's / grad's own bits with init.

Every case has the same inputs: seeded normal data with NaN, +-inf, -0.0, both borders, a .5 tie and a subnormal written into
x (distinct places of one channel: first and last packet of the first and the last row, then the middles -- _inputs asserts
that every value is still there, also where the quantized axis is the last one or there is one row), a negative, a zero and a tiny scale, and an inf and a NaN
upstream gradient in channels of their own.

CASES below is the table: family, [outer.., C, inner..] as a function of the packet width V (16 bytes / element size), the
quantized axis, and the tools knobs of each run.  Shapes are the smallest the production policy (no knob) sends to the family;
a run with a knob is there for what the policy takes only from millions of elements on (the ring needs four row tiles per
workgroup on a grid of 4-8 workgroups per CU; the 768-lane workgroups start at 3 * 2^18 elements) or never by itself (4- and
8-byte storage: the ring with one channel per lane, the 1024-lane workgroups; the forward's ring) -- those are marked
"knob"."""
import ctypes
import itertools
import os
import time

import numpy as np
import pytest
import torch

from helpers import assert_bits_equal, pc_coordinates, per_channel_kernels
from helpers import check_sums as _check_sums, same_stored as _same_stored
from oracle import lsq_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROD_LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip.so")
EXEMPT = os.path.join(ROOT, "tests", "golden", "kernel_ledger_exempt.json")

DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
Q = (-8, 7, -128, 127)

NONE, RING, REGS = {}, {"force_ring": 2}, {"force_ring": 1}
# name: (shape(V), axis, runs = ((knobs, "policy" | "knob"), ...), misaligned view, storage types (None = all four))
CASES = {
    # 256-lane windows, one channel per lane (inner a multiple of V)
    "win_cpl1": (lambda V: (9, 6, 3 * V), 1, ((NONE, "policy"), (RING, "knob"), (REGS, "knob")), False, None),
    # ... two channels per lane (inner = V + 1: every packet but the first of a row straddles a channel border)
    "win_cpl2": (lambda V: (9, 8, V + 1), 1, ((NONE, "policy"), (RING, "knob"), (REGS, "knob")), False, None),
    # ... V channels per lane (inner = 3 < V; fp64: V = 2, two channels)
    "win_cplv": (lambda V: (9, 8, 3), 1, ((NONE, "policy"), (RING, "knob"), (REGS, "knob")), False, None),
    # ... V == 1: an odd row length, and a view that starts one element past a 16-byte boundary
    "win_v1_odd": (lambda V: (9, 7, 3), 1, ((NONE, "policy"),), False, None),
    "win_misaligned": (lambda V: (9, 6, 3 * V), 1, ((NONE, "policy"),), True, None),
    # many rows: four row tiles per workgroup, the ring by policy where the storage type takes it by default
    "win_rows_cpl2": (lambda V: (4099, 8, V + 1), 1, ((NONE, "policy"),), False, None),
    # row-group windows (the quantized axis is the last one): the usual block, ring and register loops, the forward with the
    # LDS table (knob 2) and direct
    "ww": (lambda V: (41, 12 * V), 1, ((NONE, "policy"), (RING, "knob"), (REGS, "knob"), ({"set_fwd_direct": 2}, "knob")), False, None),
    # ... 768 / 1024 lanes: by policy for 16-bit storage (rows of 48 lanes, 3 * 2^18 elements), by knob elsewhere
    "ww_big_policy": (lambda V: (2048, 48 * V), 1, ((NONE, "policy"),), False, (torch.bfloat16, torch.float16)),
    "ww_big": (lambda V: (41, 12 * V), 1, (({"set_ww_big": 1}, "knob"),), False, None),
    # ... rows of 128 lanes cut into 64-lane windows (4- and 8-byte storage by policy)
    "ww_split64": (lambda V: (41, 128 * V), 1, ((NONE, "policy"), ({"set_ww_split64": 1}, "knob")), False, None),
    # owner windows: 256 owners of one channel (two packets a row) / of V channels (runs of V + 1 positions)
    "own_cpl1": (lambda V: (32, 256, 2 * V), 1, ((NONE, "policy"),), False, None),
    "own_cpl2": (lambda V: (16, 256 * V, V + 1), 1, ((NONE, "policy"),), False, None),
    # the segment walk: one row of one workgroup's span (short walk, no finalize); seven rows of three spans (the backward's
    # loop form + finalize; the forward's loop form starts at nine iterations, which the policy gives only to 2048 channels and
    # more of such rows: knob)
    "seg_short": (lambda V: (1, 6, 256 * V), 1, ((NONE, "policy"),), False, None),
    "seg_loop": (lambda V: (7, 6, 2 * 256 * V + V), 1, ((NONE, "policy"), ({"set_seg_no_up_front": 1}, "knob")), False, None),
}
FWD_MODES = [(init, levels) for init in (False, True) for levels in (False, True)]
BWD_MODES = [(sym, init, False) for sym in (False, True) for init in (False, True)] + [(False, init, True) for init in (False, True)]

LEDGER = {}       # kernel symbol -> every oracle-checked run that launched it
TIMES = {}


@pytest.fixture(scope="module")
def T():
    import torchlsq  # noqa: F401
    import lsq_tools
    from torchlsq import extension
    extension._assert_has_ops()
    lsq_tools.activate()
    yield lsq_tools
    lsq_tools.deactivate()


@pytest.fixture(scope="module")
def shipped():
    return per_channel_kernels(PROD_LIB)


def _inputs(shape, axis, dtype):
    """(x, grad, scale, shift) on the CPU: the same recipe for every case"""
    from torchlsq import synth
    n = int(np.prod(shape))
    outer, C, inner = O.axis_to_ocl(shape, axis)
    assert C >= 6
    pdt = torch.float64 if dtype == torch.float64 else torch.float32
    x = synth.normal_like(n, 61, 0.5, 1.0, dtype=dtype).view(outer, C, inner).clone()
    g = synth.normal_like(n, 62, 0.0, 1e-3, dtype=dtype).view(outer, C, inner).clone()
    s = synth.uniform_like(C, 63, 0.05, 0.35, dtype=pdt).clone()
    b = synth.normal_like(C, 64, 0.0, 0.1, dtype=pdt).clone()
    s[0], b[0] = 0.25, 0.5            # exact in every storage type: borders at -1.5 and 2.25, a tie at 1.125
    s[2], s[3], s[5] = -0.125, 0.0, 1e-30
    tiny = {torch.float32: 1e-40, torch.float64: 1e-310, torch.bfloat16: 1e-40, torch.float16: 1e-6}[dtype]
    nan, inf = float("nan"), float("inf")
    # The edge values of a channel go to distinct places of its [outer, inner] plane: the corners first (first and last packet of
    # the first and the last row, the last one ragged where inner is no multiple of V), then the middles; where rows or columns
    # coincide (inner == 1: the quantized axis is the last one; outer == 1) a taken place moves on to the next free one.
    P, last, mid, half = outer * inner, inner - 1, inner // 2, (outer // 2) * inner
    assert P >= 16
    prefer = [0, last, P - inner, P - 1, mid, P - inner + mid, half + last, half, half + mid]
    taken = {c: set() for c in range(C)}
    written = []

    def put(t, c, v):
        k = next(q for q in itertools.chain(prefer, range(P)) if q not in taken[c])
        taken[c].add(k)
        t[k // inner, c, k % inner] = v
        written.append((t, (k // inner, c, k % inner), v))
    # channel 0 (scale 0.25, shift 0.5): everything; the negative, zero and tiny scales and the last channel: a few each
    for v in (nan, inf, -inf, -0.0, -1.5, 2.25, 1.125, tiny):
        put(x, 0, v)
    for c, vals in ((2, (nan, -0.0, inf)), (3, (inf, tiny, -0.0)), (5, (tiny, -inf, nan)), (C - 1, (nan, -0.0))):
        for v in vals:
            put(x, c, v)
    # (test_non_finite_gradients_stay_in_their_channel: the last element of channel 1's first row, saturated; channel 4)
    g[0, 1, last] = inf
    x[0, 1, last] = 100.0
    written += [(g, (0, 1, last), inf), (x, (0, 1, last), 100.0)]
    for v in (nan, -inf):
        put(g, 4, v)
    for t, pos, v in written:        # every listed value is there: no place was written twice
        have, want = t[pos].reshape(1), torch.tensor([v], dtype=dtype)
        assert have.view(torch.uint8).tolist() == want.view(torch.uint8).tolist() or (v != v and bool(torch.isnan(have))), (shape, pos, v)
    assert bool(torch.tensor(tiny, dtype=dtype) != 0)
    return x.view(shape), g.view(shape), s, b


def _np(t):
    return (t.float() if t.dtype in (torch.bfloat16, torch.float16) else t).cpu().numpy()


def _bits(t):
    return t.cpu().contiguous().view(torch.uint8).numpy()


def _reference(shape, axis, dtype, x, g, s, b):
    outer, C, inner = O.axis_to_ocl(shape, axis)
    xs, gs, sn, bn = _np(x), _np(g), s.numpy(), b.numpy()
    ref = {"y": {init: O.fwd_pc(xs, sn, bn, outer, C, inner, *Q, init) for init in (False, True)},
           "levels": O.levels_pc(xs, sn, bn, outer, C, inner, *Q)}
    for m in BWD_MODES:
        sym, init, ev = m
        ref[m] = O.bwd_pc(gs, xs, sn, bn, outer, C, inner, *Q, True, 1.0, sym, ev, init)
    return ref


def _held(T, shipped, run, names, check):
    """`check()` holds the call that launched `names` to the oracle; only then do they count as covered by `run`"""
    assert names, run + ": the tools library recorded no per-channel launch"
    unknown = sorted(names - set(shipped))
    assert not unknown, "%s launched kernels that liblsq_hip.so does not ship: %s" % (run, unknown)
    coords = "; ".join(sorted(pc_coordinates(shipped[k]) for k in names))
    try:
        check()
    except AssertionError as e:
        raise AssertionError("%s [%s]: %s" % (run, coords, e)) from None
    for k in names:
        LEDGER.setdefault(k, []).append(run)


@pytest.mark.parametrize("case,dtype", [pytest.param(c, d, id="%s-%s" % (c, str(d).split(".")[-1])) for c in sorted(CASES)
                                        for d in DTYPES if CASES[c][4] is None or d in CASES[c][4]])
def test_case_equals_the_oracle(T, shipped, case, dtype):
    from torchlsq import extension as E
    shape_of, axis, runs, misaligned, only = CASES[case]
    t0 = time.perf_counter()
    V = 16 // torch.empty(0, dtype=dtype).element_size()
    shape = shape_of(V)
    dev = torch.device("cuda:0")
    x, g, s, b = _inputs(shape, axis, dtype)
    ref = _reference(shape, axis, dtype, x, g, s, b)
    n = x.numel()

    def place(t):
        if not misaligned:
            return t.to(dev)
        buf = torch.empty(n + 1, dtype=t.dtype, device=dev)
        buf[1:].copy_(t.reshape(-1))
        return buf[1:].view(shape)
    xd, gd, sd, bd = place(x), place(g), s.to(dev), b.to(dev)
    assert (xd.data_ptr() % 16 != 0) == misaligned
    for knobs, how in runs:
        tag = "%s %s %s%s" % (case, str(dtype).split(".")[-1], how, "".join(" %s=%d" % kv for kv in sorted(knobs.items())))
        try:
            for k, v in knobs.items():
                T.set_knob(k, v)
            for init, levels in FWD_MODES:
                T.launched_reset()
                out = E.hip_forward_per_channel(xd, sd, bd, axis, *Q, True, 1.0, False, False, init, levels_bias=0 if levels else None)
                torch.cuda.synchronize()
                y, lv = out if levels else (out, None)

                def check_fwd():
                    _same_stored(y, ref["y"][init], dtype, "y")
                    if init:
                        assert_bits_equal(_bits(y), _bits(x), "y carries x's bits")
                    if levels:
                        assert np.array_equal(lv.cpu().numpy().astype(np.int32).reshape(-1), ref["levels"].reshape(-1)), "int8 levels"
                _held(T, shipped, tag + " forward init=%d levels=%d" % (init, levels), T.launched(), check_fwd)
            for sym, init, ev in BWD_MODES:
                T.launched_reset()
                dx, ds, db = E.hip_backward_per_channel(gd, xd, sd, bd, axis, *Q, True, 1.0, sym, ev, init)
                torch.cuda.synchronize()
                r = ref[(sym, init, ev)]

                def check_bwd():
                    _same_stored(dx, r.dx, dtype, "dx")
                    if init:
                        assert_bits_equal(_bits(dx), _bits(g), "dx carries grad's bits")
                    if ev:
                        assert not ds.cpu().numpy().any() and not db.cpu().numpy().any(), "eval mode: zero sums"
                    _check_sums(ds, r.ds_wide, r.abs_ds, "d_scale")
                    _check_sums(db, r.db_wide, r.abs_db, "d_shift")
                _held(T, shipped, tag + " backward sym=%d init=%d eval=%d" % (sym, init, ev), T.launched(), check_bwd)
        finally:
            T.reset_knobs()
    TIMES[(case, dtype)] = time.perf_counter() - t0


def test_launch_record_names_shipped_kernels(T, shipped):
    """the record itself: a forward and a two-step backward leave the mangled symbols of the code object (the forward kernel;
    the backward kernel and its finalize), a reset empties it, and a buffer that is too small gets the size and no byte"""
    from torchlsq import extension as E
    dev = torch.device("cuda:0")
    x, g, s, b = (t.to(dev) for t in _inputs((41, 48), 1, torch.float32))
    lib = T.activate()
    T.launched_reset()
    assert T.launched() == set() and lib.lsq_hip_debug_launched_names(None, 0) == 1       # (the terminator)
    E.hip_forward_per_channel(x, s, b, 1, *Q, True, 1.0, False, False, False)
    fwd = T.launched()
    assert len(fwd) == 1 and fwd <= set(shipped) and shipped[next(iter(fwd))]["family"] == "fwd_pc", fwd
    T.launched_reset()
    E.hip_backward_per_channel(g, x, s, b, 1, *Q, True, 1.0, False, False, False)
    bwd = T.launched()
    assert bwd <= set(shipped) and sorted(shipped[k]["family"] for k in bwd) == ["bwd_pc", "finalize_ww"], bwd
    need = lib.lsq_hip_debug_launched_names(None, 0)
    assert need == sum(len(k) + 1 for k in bwd)                                             # names + newlines, the last one's place: NUL
    small = ctypes.create_string_buffer(b"\x7f" * (need - 1), need - 1)
    assert lib.lsq_hip_debug_launched_names(small, need - 1) == need and small.raw == b"\x7f" * (need - 1)
    exact = ctypes.create_string_buffer(need)
    assert lib.lsq_hip_debug_launched_names(exact, need) == need and set(exact.value.decode().split("\n")) == bwd
    T.launched_reset()
    assert T.launched() == set()
    torch.cuda.synchronize()


def test_ledger_every_shipped_kernel_is_covered_or_exempt(shipped):
    """covered == shipped - exempt: a kernel that is neither fails with its coordinates, and so does an exempt one that ran"""
    import json
    with open(EXEMPT) as f:
        exempt = {e["symbol"] for e in json.load(f)["exempt"]}
    covered = set(LEDGER)
    # a kernel that a run with every knob 0 reached is the policy's, whatever knob run reached it too
    by_policy = {k: [r for r in runs if " policy " in r] for k, runs in LEDGER.items()}
    print("\nkernel ledger: %d shipped, %d covered (%d by a run with every knob 0, %d through a tools knob only), %d exempt; cases took %.1f s" %
          (len(shipped), len(covered), sum(1 for k in covered if by_policy[k]), sum(1 for k in covered if not by_policy[k]),
           len(exempt), sum(TIMES.values())))
    for k in sorted(covered, key=lambda k: pc_coordinates(shipped[k])):
        print("  %-100s <- %s  (%d runs)" % (pc_coordinates(shipped[k]), (by_policy[k] or LEDGER[k])[0], len(LEDGER[k])))
    stale = sorted(pc_coordinates(shipped[k]) for k in covered & exempt)
    missing = sorted(pc_coordinates(shipped[k]) for k in set(shipped) - covered - exempt)
    assert not stale, "exempt, but a case launched them (stale entries):\n  " + "\n  ".join(stale)
    assert not missing, "%d shipped per-channel kernels that no oracle-checked case launched and no exemption lists:\n  %s" % (
        len(missing), "\n  ".join(missing))
    assert covered == set(shipped) - exempt
