#!/usr/bin/env python3
"""A/B: the gated product act(gate) * up on 8-bit levels (liblsq_hip_glu_w8.so: lsq_glu_w8_q8_q) against the only route of the parent
commit on the same inputs: uint8 levels in and out, mid_dtype bfloat16, SiLU, C in {11008, 14336} x M in {1, 16, 512, 2048}.  gate and
up are the halves of ONE fused [M, 2 C] buffer, as a fused gate_up linear leaves them.

    new      one launch that reads the halves in place: 2 bytes read and 1 written per hidden element
    parent   `.contiguous()` of each half, `lsq_lut_w8` (the activation's byte table), `lsq_mul_gate_w8_q8_q` (its same-shape form):
             four launches, 4 bytes read and 3 written per hidden element
    dense    the parent's route where gate and up are two dense tensors already: the table op and the gate multiply, two launches,
             3 bytes read and 2 written per hidden element
    copy     a plain device-to-device copy of 1.5 M C bytes: the op's own 3 M C bytes of traffic, the yardstick of a bandwidth kernel

The parent's route has a quantizer between the activation and the product (it cannot be expressed on levels without one), so the new
op's float table is built with that quantizer (`lsq_glu_table(..., act_out=...)`): the two routes then compute the same bytes, and
they are compared for equality, with two launches of the new route and the non-vacuity of the output quantizer, before any timing.
Then each route is captured as ONE graph of back-to-back calls, one per input set, over as many sets as exceed the 256 MB Infinity
Cache by a quarter -- at most MAX_SETS of them: the sets of the M = 1 and M = 16 cases stay cache-resident, and their lines say so in
the `MB` column, the bytes of all input sets -- and ROUNDS rounds alternate the graphs in one process, timed with HIP events.
Reported: the median microseconds per call of each route, the spread of a route's rounds ((max - min) / median), new / parent,
new / dense, new / copy, and the op's 3 M C bytes over the time as a share of 8 TB/s.

Expectation from byte counts (3 against >= 5 bytes per element and at least one launch fewer), marked per line: `HIT` where
new / parent < 1 - the larger of the two routes' spreads, `MISS` otherwise; the same for the dense column.

    python tools/exp_glu_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CASES = [(C, M) for C in (11008, 14336) for M in (1, 16, 512, 2048)]
CACHE_BYTES = 256 << 20
MAX_SETS = 512
PEAK = 8e12
RNG = (0, 255, 0, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, three cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r34_glu_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, _act_constants, lsq_act_table, lsq_glu_table
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [CASES[0], CASES[2], CASES[7]] if args.quick else CASES
    gen = torch.Generator(device=dev).manual_seed(0)
    s_g = torch.tensor([0.05], device=dev)                  # the gate spans -6.4 .. 6.35: both bends of the SiLU
    z_g = torch.tensor([128], dtype=torch.int32, device=dev)
    s_u = torch.tensor([0.0371], device=dev)
    z_u = torch.tensor([128], dtype=torch.int32, device=dev)
    # the quantizer between the activation and the product: the SiLU's range on the 256 gate levels on 0..255
    v = F.silu(LevelsTensor(torch.arange(256, dtype=torch.uint8, device=dev), s_g, z_g, *RNG).dequantize(torch.float32))
    a_sc, a_sh = ((v.max() - v.min()) / 255).reshape(1), v.min().reshape(1).clone()
    s_a, z_a = _act_constants(a_sc, a_sh, 0, 255)
    byte_table = lsq_act_table("silu", s_g, z_g, torch.uint8, a_sc, a_sh, *RNG, mid_dtype=torch.bfloat16)
    table = lsq_glu_table("silu", s_g, z_g, torch.uint8, (a_sc, a_sh, *RNG), torch.bfloat16)
    lines = ["# exp_glu_w8_ab: the gated product SiLU(gate) * up on 8-bit levels (liblsq_hip_glu_w8.so), reading the halves of a fused "
             "[M, 2 C] buffer in place, vs the parent's only route (.contiguous() of each half, lsq_lut_w8, lsq_mul_gate_w8_q8_q), vs that "
             "route on operands that are dense already, and vs a device-to-device copy of 1.5 M C bytes; %s, %d CUs" % (
                 torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` input sets of `MB` "
             "megabytes in all (1.25 x the 256 MB cache, at most %d sets: fewer megabytes than 320 are cache-resident); spread = (max - "
             "min) / median of a route's rounds; uint8 levels in and out, mid_dtype bfloat16; the new route's bytes checked against the "
             "parent's on the same inputs before any timing; %%: 3 M C bytes / time over 8 TB/s; per: packets per lane; HIT: "
             "new / other < 1 - the larger spread of the two" % (rounds, MAX_SETS),
             "%-12s %5s %4s %5s %3s | %8s %6s %5s | %9s %6s %6s %-4s | %8s %6s %6s %-4s | %8s %6s" % (
                 "C x M", "calls", "sets", "MB", "per", "new us", "spread", "%", "parent us", "spread", "new/p", "", "dense us", "spread",
                 "new/d", "", "copy us", "new/c")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    misses = []
    for C, M in cases:
        fused_bytes = M * 2 * C
        nsets = min(MAX_SETS, -(-CACHE_BYTES * 5 // 4 // fused_bytes))
        iters = max(args.iters, nsets)
        gu = [torch.randint(0, 256, (M, 2 * C), device=dev, generator=gen, dtype=torch.uint8) for _ in range(nsets)]
        gd = [g[:, :C].contiguous() for g in gu]
        ud = [g[:, C:].contiguous() for g in gu]
        src = [torch.randint(0, 256, (M * C * 3 // 2,), device=dev, generator=gen, dtype=torch.uint8) for _ in range(nsets)]
        dst = torch.empty_like(src[0])
        plan = E.glu_w8_plan(M, C, 2 * C, 2 * C)
        assert plan["family"] == "packets"
        t = ops.lsq_glu_w8_q8(gu[0][:, :C], gu[0][:, C:], s_u, z_u, table, torch.float32)
        sample = t.flatten()[:1 << 22].double()         # the output quantizer: the products' 2nd to 98th percentile on 0..255
        lo, hi = sample.quantile(0.02), sample.quantile(0.98)
        osc = ((hi - lo) / 255).float().reshape(1)
        osh = (-torch.round(-lo / osc.double()) * osc.double()).float().reshape(1)
        del t

        def new(i):
            return ops.lsq_glu_w8_q8_q(gu[i][:, :C], gu[i][:, C:], s_u, z_u, table, osc, osh, *RNG, torch.bfloat16)

        def parent(i):
            g, u = gu[i][:, :C].contiguous(), gu[i][:, C:].contiguous()
            return ops.lsq_mul_gate_w8_q8_q(ops.lsq_lut_w8(g, byte_table, torch.uint8), s_a, z_a, u, s_u, z_u, osc, osh, *RNG, torch.bfloat16)

        def dense(i):
            return ops.lsq_mul_gate_w8_q8_q(ops.lsq_lut_w8(gd[i], byte_table, torch.uint8), s_a, z_a, ud[i], s_u, z_u, osc, osh, *RNG,
                                            torch.bfloat16)

        def copy(i):
            return dst.copy_(src[i])

        routes = [new, parent, dense, copy]
        with torch.no_grad():
            y = new(0)
            assert y.shape == (M, C) and y.is_contiguous() and torch.equal(y, new(0)), "two launches differ"
            assert torch.equal(y, parent(0)) and torch.equal(y, dense(0)), "not the bytes of the parent's route"
            inside = ((y > 0) & (y < 255)).float().mean().item()
            assert len(y.unique()) > 32 and 0.25 <= inside and bool((y == 0).any()) and bool((y == 255).any()), \
                "a vacuous output quantizer (%.2f inside)" % inside
            del y
            graphs = []
            for fn_ in routes:
                def run(fn_=fn_):
                    for i in range(iters):
                        fn_(i % nsets)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    run()
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    run()
                graphs.append(g)
        times = [[] for _ in graphs]
        for _ in range(rounds + 1):                     # the first round warms up
            for j, g in enumerate(graphs):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                g.replay()
                t1.record()
                t1.synchronize()
                times[j].append(t0.elapsed_time(t1) * 1e3 / iters)
        med = [statistics.median(t[1:]) for t in times]
        spread = [(max(t[1:]) - min(t[1:])) / m for t, m in zip(times, med)]
        tn, tp, td, tc = med
        marks = ["HIT" if tn / other < 1 - max(spread[0], spread[j]) else "MISS" for j, other in ((1, tp), (2, td))]
        for mark, what in zip(marks, ("parent", "dense")):
            if mark == "MISS":
                misses.append("%d x %d (%s)" % (C, M, what))
        line = "%-12s %5d %4d %5.0f %3d | %8.2f %6.3f %5.1f | %9.2f %6.3f %6.2f %-4s | %8.2f %6.3f %6.2f %-4s | %8.2f %6.2f" % (
            "%d x %d" % (C, M), iters, nsets, nsets * fused_bytes / 1e6, plan["packets_per_lane"], tn, spread[0],
            100 * 3 * M * C / (tn * 1e-6) / PEAK, tp, spread[1], tn / tp, marks[0], td, spread[2], tn / td, marks[1], tc, tn / tc)
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                  # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del graphs, gu, gd, ud, src, dst
        torch.cuda.empty_cache()
    lines.append("# expectation (new / parent and new / dense < 1 beyond the spread in every case): %s"
                 % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    lines.append("# whether LDS or VALU bounds the kernel in the large cases: NOT MEASURED (no counter run was made)")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
