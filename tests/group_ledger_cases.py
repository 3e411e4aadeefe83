"""The group-wise ledger's table (tests/test_group_ledger_gpu.py, tests/test_group_ledger_cpu.py): a restatement of the launch
plan of liblsq_hip_group.so, a classifier that names the branches of the two kernel bodies a shape drives, the cases, and
the one input recipe every case runs on.

  * `plan(V, n, G, cus)` restates plan_group (csrc/group/lsq_grp_body.hpp) in Python; the tests hold it to
    extension.group_plan.  V = 16 bytes / element size, cus = compute units of the device.
  * `tags(V, n, G, cus)` reads lsq_grp_fwd_body.inc / lsq_grp_bwd_body.inc against that plan: which arm of every branch that
    depends on the shape is taken.  ALL_TAGS is the whole list; NO_CASE names the combinations that have no case, all but
    one of them because no shape reaches them.
  * CASES: every entry is a function of V, so all four storage types meet the same packet geometry; the chip-sized ones also
    take cus, so a part with another CU count fails its tag assertion instead of silently testing less.
  * `make_inputs` writes NaN, +-inf, -0.0, both borders, a tie and a subnormal into x, a negative, a zero and a tiny scale,
    and non-finite gradients into groups of their own and into the border groups of the waves' ranges, and asserts that
    every written value is still in place.
"""
import itertools

import torch

BLOCK, UNROLL, WAVES = 256, 4, 4          # kBlock, kGrpUnroll, waves per workgroup
STEP = 64 * UNROLL                        # items a wave loads per step of the backward
TILE = BLOCK * UNROLL                     # packets per tile of the packet-form forward
FWD_PER_CU, BWD_PER_CU = 16, 4            # kGrpFwdBlocksPerCU, kGrpBwdBlocksPerCU
Q = (-8, 7, -128, 127)                    # with scale 0.25 and shift 0.5: borders at -1.5 and 2.25, a tie at 1.125

DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]


def vec_of(dtype):
    return 16 // torch.empty(0, dtype=dtype).element_size()


def _cdiv(a, b):
    return (a + b - 1) // b


def _log2_exact(v):
    return v.bit_length() - 1 if v > 0 and v & (v - 1) == 0 else -1


def plan(V, n, G, cus):
    """plan_group restated: form, reduction, items per group, both grids, groups per wave, units per wave"""
    packet = G % V == 0
    ipg = G // V if packet else G
    pg_shift = _log2_exact(ipg)
    mode = "p2" if packet and pg_shift >= 0 else ("scan-packet" if packet else "scan-element")
    fwd_round, bwd_round = cus * FWD_PER_CU, cus * BWD_PER_CU
    n_items = n // V if packet else n
    if packet:
        fwd_grid = min(max(1, _cdiv(n_items, TILE)), fwd_round)
    else:
        fwd_grid = min(max(1, _cdiv(n, BLOCK)), fwd_round)
    p = dict(V=V, n=n, G=G, cus=cus, form="packet" if packet else "element", mode=mode, items_per_group=ipg, pg_shift=pg_shift,
             n_items=n_items, n_groups=n // G, fwd_grid=fwd_grid, groups_per_wave=0, units=0, unit=0, units_per_wave=0)
    if mode == "p2":
        unit = max(STEP, ipg)
        units = max(1, _cdiv(n_items, unit))
        p["bwd_grid"] = min(_cdiv(units, WAVES), bwd_round)
        p["unit"], p["units"] = unit, units
        p["units_per_wave"] = _cdiv(units, p["bwd_grid"] * WAVES)
    else:
        n_groups = max(1, n // G)
        want = min(n_groups, max(1, min(bwd_round * WAVES, _cdiv(n_items, STEP))))
        gpw = _cdiv(n_groups, want)
        p["groups_per_wave"] = gpw
        p["bwd_grid"] = _cdiv(_cdiv(n_groups, gpw), WAVES)
    p["reduction"] = "butterfly" if mode == "p2" else "scan"
    return p


def wave_range(p, w):
    """the groups wave `w` of the backward sums, in the order it walks them (a list of ranges; empty: the wave has none)"""
    ng = p["n_groups"]
    if p["mode"] == "p2":
        per_unit = p["unit"] // p["items_per_group"]
        n_waves = p["bwd_grid"] * WAVES
        return [range(u * per_unit, min((u + 1) * per_unit, ng)) for u in range(w, p["units"], n_waves)]
    gpw = p["groups_per_wave"]
    lo = w * gpw
    return [range(lo, min(lo + gpw, ng))] if lo < ng else []


def busy_waves(p):
    if p["mode"] == "p2":
        return min(p["units"], p["bwd_grid"] * WAVES)
    return _cdiv(p["n_groups"], p["groups_per_wave"])


def _straddles(gi, count, width):
    """does one of `count` consecutive groups of gi items, the first at offset 0, lie across a multiple of `width`?"""
    if gi > width:
        return True
    return any((j * gi) % width + gi > width for j in range(min(count, width)))


def tags(V, n, G, cus):
    """the arms of the shape-dependent branches of lsq_grp_fwd_body.inc / lsq_grp_bwd_body.inc that (V, n, G) takes"""
    p = plan(V, n, G, cus)
    t = set()
    ipg, items = p["items_per_group"], p["n_items"]
    # ---- backward
    if p["mode"] == "p2":
        pg = ("1" if ipg == 1 else "2..32" if ipg <= 32 else "64" if ipg == 64 else "65..255" if ipg < 256 else
              "256" if ipg == 256 else "512..")
        partial = items % p["unit"] != 0
        several = p["units"] > p["bwd_grid"] * WAVES
        t.add("bwd/p2/pg=" + pg)
        t.add("bwd/p2/" + ("partial-last-unit" if partial else "whole-units"))
        t.add("bwd/p2/" + ("several-units-a-wave" if several else "one-unit-a-wave"))
        if 64 < ipg < 256:
            t.add("bwd/p2/pg=65..255+" + ("partial-last-unit" if partial else "whole-units"))
        if several:
            t.add("bwd/p2/several-units-a-wave+" + ("lane-sums" if ipg > 64 else "butterfly"))
    else:
        k = "bwd/sp/" if p["mode"] == "scan-packet" else "bwd/se/"
        gpw, ng = p["groups_per_wave"], p["n_groups"]
        t.add(k + ("gi>=64" if ipg >= 64 else "gi<64"))
        t.add(k + ("several-groups-a-wave" if gpw > 1 else "one-group-a-wave"))
        t.add(k + ("pass-straddled" if _straddles(ipg, gpw, 64) else "pass-aligned"))
        t.add(k + ("step-straddled" if _straddles(ipg, gpw, STEP) else "step-aligned"))
        t.add(k + ("last-wave-ragged" if ng % gpw else "last-wave-full"))
        if ipg >= 64 and gpw > 1:
            t.add(k + "gi>=64+several-groups-a-wave")
        if ipg > STEP:
            t.add(k + "gi>256+" + ("several-groups-a-wave" if gpw > 1 else "one-group-a-wave"))
    # ---- forward
    grid = p["fwd_grid"]
    if p["form"] == "packet":
        n_full, rest = items // TILE, items % TILE
        t.add("fwd/packet/" + ("partial-tile-only" if n_full == 0 else "full+partial-tile" if rest else "full-tiles-only"))
        t.add("fwd/packet/" + ("several-trips" if n_full > grid else "one-trip"))
        t.add("fwd/packet/" + ("pg_shift" if p["pg_shift"] >= 0 else "divu64"))
        if rest and n_full % grid:
            t.add("fwd/packet/partial-owner>0")
    else:
        t.add("fwd/elem/" + ("several-blocks" if n > BLOCK else "one-block"))
        t.add("fwd/elem/" + ("several-trips" if n > grid * BLOCK else "one-trip"))
    return t


_SCAN = ["gi<64", "gi>=64", "one-group-a-wave", "several-groups-a-wave", "pass-aligned", "pass-straddled", "step-aligned",
         "step-straddled", "last-wave-full", "last-wave-ragged", "gi>=64+several-groups-a-wave", "gi>256+one-group-a-wave",
         "gi>256+several-groups-a-wave"]
ALL_TAGS = sorted(
    ["bwd/p2/pg=" + c for c in ("1", "2..32", "64", "65..255", "256", "512..")] +
    ["bwd/p2/whole-units", "bwd/p2/partial-last-unit", "bwd/p2/one-unit-a-wave", "bwd/p2/several-units-a-wave",
     "bwd/p2/pg=65..255+whole-units", "bwd/p2/pg=65..255+partial-last-unit",
     "bwd/p2/several-units-a-wave+butterfly", "bwd/p2/several-units-a-wave+lane-sums"] +
    ["bwd/sp/" + s for s in _SCAN] + ["bwd/se/" + s for s in _SCAN] +
    ["fwd/packet/partial-tile-only", "fwd/packet/full+partial-tile", "fwd/packet/full-tiles-only", "fwd/packet/one-trip",
     "fwd/packet/several-trips", "fwd/packet/pg_shift", "fwd/packet/divu64", "fwd/packet/partial-owner>0",
     "fwd/elem/one-block", "fwd/elem/several-blocks", "fwd/elem/one-trip", "fwd/elem/several-trips",
     # lsq_group_forward only (the C-entry test): a packet plan whose levels pointer is not V-aligned runs the element form
     "fwd/elem/misaligned-levels"])
# the three branches no test ran before this file: an oracle-checked case in every storage type
NEW_BRANCHES = ("bwd/se/gi>=64", "bwd/p2/pg=65..255+partial-last-unit", "bwd/p2/pg=256")
NO_CASE = {
    "bwd/p2/pg>=256 + partial-last-unit": "the unit is max(256, PG) packets = one group, and n is a multiple of G",
    "bwd/s*/gi<64 + one-group-a-wave": "a wave gets ceil(groups / ceil(items / 256)) groups: one only for gi >= 193, or for a "
                                       "tensor of a single group, which has no neighbour to leak into",
    "fwd/packet/partial-owner=0 + full tiles": "not impossible: a multiple of 16 * cus full tiles (67 MB and more); workgroup 0 then "
                                               "runs what it runs in every partial-tile-only case -- listed, not required",
    "fwd/elem/partial-owner": "the element form has no tiles: every workgroup strides over elements",
    "fwd/packet/several-trips + partial-tile-only": "a second trip needs more full tiles than workgroups",
}

# name: (G(V), groups(V, cus), chip-sized, the tags the case is there for)
CASES = {
    "p2_pg1": (lambda V: V, lambda V, cus: 13, False,                   # (13 groups, not 9: so that fp64's
               {"bwd/p2/pg=1", "bwd/p2/partial-last-unit"}),            # two-element groups hold the eight edge values)
    "p2_pg64": (lambda V: 64 * V, lambda V, cus: 7, False, {"bwd/p2/pg=64", "bwd/p2/partial-last-unit"}),
    "p2_mid_whole": (lambda V: 128 * V, lambda V, cus: 8, False, {"bwd/p2/pg=65..255+whole-units", "fwd/packet/full-tiles-only"}),
    "p2_mid_partial": (lambda V: 128 * V, lambda V, cus: 7, False, {"bwd/p2/pg=65..255+partial-last-unit"}),
    "p2_pg256": (lambda V: 256 * V, lambda V, cus: 7, False, {"bwd/p2/pg=256", "bwd/p2/whole-units"}),
    "p2_big": (lambda V: 1024 * V, lambda V, cus: 7, False, {"bwd/p2/pg=512..", "bwd/p2/one-unit-a-wave"}),
    "p2_loop_small": (lambda V: 8 * V, lambda V, cus: (16 * cus + 3) * 32 + 8, True,
                      {"bwd/p2/pg=2..32", "bwd/p2/several-units-a-wave+butterfly", "bwd/p2/partial-last-unit",
                       "fwd/packet/full+partial-tile", "fwd/packet/partial-owner>0"}),
    "p2_loop_mid": (lambda V: 128 * V, lambda V, cus: 2 * (16 * cus + 3) + 1, True,
                    {"bwd/p2/several-units-a-wave+lane-sums", "bwd/p2/pg=65..255+partial-last-unit"}),
    "sp_3": (lambda V: 3 * V, lambda V, cus: 171, False, {"bwd/sp/gi<64", "bwd/sp/several-groups-a-wave", "bwd/sp/last-wave-full"}),
    "sp_3_few": (lambda V: 3 * V, lambda V, cus: 8, False, {"bwd/sp/pass-aligned", "bwd/sp/step-aligned"}),   # (one wave, 24 items)
    "sp_63": (lambda V: 63 * V, lambda V, cus: 9, False, {"bwd/sp/gi<64", "bwd/sp/pass-straddled"}),
    "sp_65": (lambda V: 65 * V, lambda V, cus: 7, False, {"bwd/sp/gi>=64+several-groups-a-wave", "bwd/sp/last-wave-ragged"}),
    # (sp_96 and sp_384: 7 groups, the recipe's minimum; 5 would reach the same branches with groups 4, 5 and the last one merged)
    "sp_96": (lambda V: 96 * V, lambda V, cus: 7, False, {"bwd/sp/gi>=64+several-groups-a-wave", "bwd/sp/step-straddled"}),
    "sp_384": (lambda V: 384 * V, lambda V, cus: 7, False, {"bwd/sp/gi>256+one-group-a-wave", "fwd/packet/divu64"}),
    "sp_384_many": (lambda V: 384 * V, lambda V, cus: 16 * cus + 1, True, {"bwd/sp/gi>256+several-groups-a-wave"}),
    "se_1": (lambda V: 1, lambda V, cus: 170, False, {"bwd/se/gi<64", "bwd/se/pass-aligned", "fwd/elem/one-block"}),
    "se_7": (lambda V: 7, lambda V, cus: 41, False, {"bwd/se/gi<64", "bwd/se/pass-straddled", "bwd/se/last-wave-ragged"}),
    "se_63": (lambda V: 63, lambda V, cus: 9, False, {"bwd/se/gi<64", "bwd/se/last-wave-full"}),
    "se_65": (lambda V: 65, lambda V, cus: 7, False, {"bwd/se/gi>=64+several-groups-a-wave", "bwd/se/last-wave-ragged",
                                                      "bwd/se/step-straddled"}),
    "se_127": (lambda V: 127, lambda V, cus: 9, False, {"bwd/se/gi>=64+several-groups-a-wave", "bwd/se/pass-straddled"}),
    "se_259": (lambda V: 259, lambda V, cus: 7, False, {"bwd/se/gi>256+one-group-a-wave"}),
    "se_259_many": (lambda V: 259, lambda V, cus: 16 * cus + 1, True, {"bwd/se/gi>256+several-groups-a-wave"}),   # (its element twin)
    "fwd_loop_packet": (lambda V: 128 * V, lambda V, cus: (16 * cus + 1) * 8 + 3, True,
                        {"fwd/packet/several-trips", "fwd/packet/partial-owner>0", "fwd/packet/full+partial-tile"}),
    "fwd_loop_elem": (lambda V: 7, lambda V, cus: _cdiv(16 * cus * 256 + 300, 7), True, {"fwd/elem/several-trips"}),
}
SMALL = [c for c in CASES if not CASES[c][2]]
CHIP = [c for c in CASES if CASES[c][2]]


def case_shape(case, V, cus):
    """(G, groups, n): every group size of the table keeps its form in every storage type -- the packet-form sizes are
    multiples of V by construction, the element-form ones (1, 7, 63, 65, 127, 259) are odd and V is 2, 4 or 8"""
    G_of, groups_of, _, _ = CASES[case]
    G, groups = G_of(V), groups_of(V, cus)
    assert groups >= 7
    return G, groups, G * groups


def case_tags(case, V, cus):
    """the case's tags on this part, after asserting the ones it is in the table for"""
    G, groups, n = case_shape(case, V, cus)
    got = tags(V, n, G, cus)
    want = CASES[case][3]
    assert want <= got, "%s (V=%d, %d CUs): planned for %s, the shape gives %s" % (case, V, cus, sorted(want - got), sorted(got))
    assert got <= set(ALL_TAGS), sorted(got - set(ALL_TAGS))
    return got


TINY = {torch.float32: 1e-40, torch.float64: 1e-310, torch.bfloat16: 1e-40, torch.float16: 1e-6}
EDGE_GROUP = (0.25, 0.5)      # scale and shift of group 0 (and of the groups that take what a short group 0 cannot hold)


def make_inputs(V, G, groups, dtype, cus, waves="all", seed=61):
    """(x, grad, grad_border, scale, shift, edge groups) on the CPU, flat: the same recipe for every case.

    x ~ N(0.5, 1), grad ~ N(0, 1e-3), scale in [0.05, 0.35), shift ~ N(0, 0.1); then
      * group 0 (scale 0.25, shift 0.5): NaN, +inf, -inf, -0.0, both borders, the tie and a subnormal in x, at the first and
        last element of the group, the last element of a packet and the first of the next and, where the group spans them,
        on both sides of the 64-item and the 256-item border of its wave's walk.  A group of fewer than eight elements passes
        the rest on to groups 6, 7, ... (the returned edge groups), which get group 0's scale and shift;
      * groups 2, 3, 5: a negative, a zero and a 1e-30 scale;
      * group 1: grad +inf on a saturated x; group 4: grad NaN and -inf; the last group: a NaN in x;
    `grad_border` is `grad` plus one non-finite gradient in the first group (a NaN, at its last element) and in the last group
    (+inf, at its first element) of every wave's range, the ranges taken from the restated plan -- of `waves`: "all", or "few"
    = the first three and the last busy wave for the chip-sized cases.  The sums of a wave live in its registers, so its range
    is where a term could leak.  Where a wave owns two or three groups that poisons every group of the tensor, so the tests
    run both: `grad` keeps finite sums to compare in every case, `grad_border` shows what stays inside a group.
    Every value written is asserted to be in place at the end: no place was written twice."""
    n = G * groups
    p = plan(V, n, G, cus)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    pdt = torch.float64 if dtype == torch.float64 else torch.float32
    x = (torch.randn(n, generator=gen, dtype=torch.float32) + 0.5).to(dtype)
    g = (torch.randn(n, generator=gen, dtype=torch.float32) * 1e-3).to(dtype)
    s = (torch.rand(groups, generator=gen, dtype=torch.float64) * 0.3 + 0.05).to(pdt)
    b = (torch.randn(groups, generator=gen, dtype=torch.float64) * 0.1).to(pdt)
    nan, inf, tiny = float("nan"), float("inf"), TINY[dtype]
    e = V if p["form"] == "packet" else 1                      # elements per item
    prefer = []
    for k in (0, G - 1, V - 1, V, 64 * e - 1, 64 * e, STEP * e - 1, STEP * e, G // 2):
        if 0 <= k < G and k not in prefer:
            prefer.append(k)
    taken, written = {}, []

    def put(t, grp, v, order=None, must=True):
        used = taken.setdefault((id(t), grp), set())
        k = next((q for q in itertools.chain(order or prefer, range(G)) if q not in used), None)
        if k is None:
            assert not must, "group %d of %d elements is full" % (grp, G)
            return False
        used.add(k)
        t[grp * G + k] = v
        written.append((t, grp * G + k, v))
        return True

    edge_vals = (nan, inf, -inf, -0.0, -1.5, 2.25, 1.125, tiny)
    edge_groups = [0] + list(range(6, 6 + _cdiv(len(edge_vals), G) - 1))
    assert edge_groups[-1] < groups - 1, "%d groups of %d elements cannot hold the edge values" % (groups, G)
    for grp in edge_groups:
        s[grp], b[grp] = EDGE_GROUP
    for k, v in enumerate(edge_vals):
        put(x, edge_groups[k // G], v)
    s[2], s[3], s[5] = -0.125, 0.0, 1e-30
    last = G - 1
    g[1 * G + last], x[1 * G + last] = inf, 100.0
    taken.setdefault((id(g), 1), set()).add(last)
    taken.setdefault((id(x), 1), set()).add(last)
    written += [(g, G + last, inf), (x, G + last, 100.0)]
    for v in (nan, -inf)[:G]:
        put(g, 4, v)
    put(x, groups - 1, nan)
    gb = g.clone()
    for key in [k for k in taken if k[0] == id(g)]:
        taken[(id(gb), key[1])] = set(taken[key])
    written += [(gb, pos, v) for t, pos, v in written if t is g]
    busy = busy_waves(p)
    which = range(busy) if waves == "all" else sorted(set(w for w in (0, 1, 2, busy - 1) if 0 <= w < busy))
    for w in which:
        stretches = wave_range(p, w)
        first, final = stretches[0][0], stretches[-1][-1]
        put(gb, first, nan, order=[G - 1, 0], must=False)
        if final != first:
            put(gb, final, inf, order=[0, G - 1], must=False)
    for t, pos, v in written:
        have, want = t[pos].reshape(1), torch.tensor([v], dtype=dtype)
        assert have.view(torch.uint8).tolist() == want.view(torch.uint8).tolist() or (v != v and bool(torch.isnan(have))), (G, groups, pos, v)
    assert bool(torch.tensor(tiny, dtype=dtype) != 0)
    return x, g, gb, s, b, edge_groups


def sweep(V, count=200, seed=5):
    """`count` seeded (n, G) pairs: group sizes of both forms and every reduction, one to a few thousand groups, and every
    eighth pair with enough groups to pass the persistent grids of a 256-CU part"""
    gen = torch.Generator(device="cpu").manual_seed(seed + V)
    r = torch.randint(0, 2 ** 31 - 1, (count, 3), generator=gen).tolist()
    out = []
    for k, (a, c, d) in enumerate(r):
        kind = a % 4
        if kind == 0:
            G = V << (c % 12)                      # P2
        elif kind == 1:
            G = V * (3 + c % 700)                  # packets, any count
        elif kind == 2:
            G = 1 + c % 600                        # anything
        else:
            G = (1, 2, 3, 5, 7, 63, 64, 65, 127, 128, 255, 256, 257, 259)[c % 14]
        groups = 1 + d % 3000 if k % 8 else 20000 + d % 200000
        out.append((G * groups, G))
    return out
