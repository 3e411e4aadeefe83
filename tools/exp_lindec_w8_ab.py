#!/usr/bin/env python3
"""A/B: the decode shape of the W8A8 linears with an 8-bit output (liblsq_hip_lindec_w8.so: lsq_linear_w8_q8_dec_q /
lsq_linear_w8_q8_dec_add_q) against the parent commit's route on the same inputs: uint8 levels in and out, int8 weight levels,
mid_dtype bfloat16, M in {1, 4, 16}, the four linears of a 4096-wide decoder layer: [4096, 4096], [6144, 4096], [22016, 4096] and
[4096, 11008] + a levels residual.

    new      the 16-wave weight-streaming kernel with the levels epilogue: one launch
    parent   lsq_linear_w8_q8_q / lsq_linear_w8_q8_add_q, which send M <= 16 to the 32-row tile of liblsq_hip_requant_w8.so /
             liblsq_hip_resadd_w8.so (four-wave workgroups): one launch, the same bytes moved
    float    the float-output decode op lsq_linear_w8_q8 (bfloat16 y) followed by lsq_levels_per_tensor: two launches (for the
             residual case WITHOUT the residual add, so this column is a lower bound of that route there)

The two level routes are compared for equality, with two launches of the new route and the non-vacuity of the output quantizer, before
any timing.  Then each route is captured as ONE graph of back-to-back calls, one per WEIGHT set, over as many weight sets as exceed the
256 MB Infinity Cache by a quarter, and ROUNDS rounds alternate the graphs in one process, timed with HIP events.  Reported: the median
microseconds per call of each route, the spread of a route's rounds ((max - min) / median), new / parent, new / float, and the weight's
N K bytes over the new route's time as a share of 8 TB/s.

No ratio can be derived beforehand: both level routes move the same bytes.  The supposition is that 16 waves per compute unit stream
the weights better than four-wave workgroups; the expectation new / parent < 1 is marked per line, `HIT` where new / parent < 1 - the
larger of the two routes' spreads, `MISS` otherwise.  `torchlsq.functional.W8A8_DECODE_DEFAULT` becomes True only if all 12 are HITs.

    python tools/exp_lindec_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (N, K, residual)
LAYERS = [(4096, 4096, False), (6144, 4096, False), (22016, 4096, False), (4096, 11008, True)]
ROWS = (1, 4, 16)
CACHE_BYTES = 256 << 20
PEAK = 8e12
RNG = (0, 255, 0, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, three cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r35_lindec_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [(layer, M) for layer in LAYERS for M in ROWS]
    if args.quick:
        cases = [cases[0], cases[5], cases[11]]
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x, zx = torch.tensor([0.0371], device=dev), torch.tensor([117], dtype=torch.int32, device=dev)
    s_r, z_r = torch.tensor([0.05], device=dev), torch.tensor([128], dtype=torch.int32, device=dev)
    lines = ["# exp_lindec_w8_ab: the decode shape of the W8A8 linears with an 8-bit output (liblsq_hip_lindec_w8.so, 16 waves per workgroup) vs "
             "the parent's route (the 32-row tile of liblsq_hip_requant_w8.so / liblsq_hip_resadd_w8.so) vs the float-output decode op + "
             "lsq_levels_per_tensor; %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` weight sets of `MB` "
             "megabytes in all (1.25 x the 256 MB cache); spread = (max - min) / median of a route's rounds; uint8 levels in and out, int8 "
             "weight levels, mid_dtype bfloat16; the new route's bytes checked against the parent's on the same inputs before any timing; "
             "%%: N K bytes / time over 8 TB/s; HIT: new / parent < 1 - the larger spread of the two" % rounds,
             "%-22s %5s %4s %5s %5s | %8s %6s %5s | %9s %6s %6s %-4s | %8s %6s %6s" % (
                 "N x K x M", "calls", "sets", "MB", "grid", "new us", "spread", "%", "parent us", "spread", "new/p", "", "float us", "spread",
                 "new/f")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    misses = []
    for (N, K, residual), M in cases:
        nsets = -(-CACHE_BYTES * 5 // 4 // (N * K))
        iters = max(args.iters, nsets)
        ws = [torch.randint(-128, 128, (N, K), device=dev, generator=gen, dtype=torch.int8) for _ in range(nsets)]
        w_s = torch.rand(N, device=dev, generator=gen) * 0.002 + 0.0005
        w_z = torch.zeros(N, dtype=torch.int32, device=dev)
        bias = torch.randn(N, device=dev, generator=gen)
        x = torch.randint(0, 256, (M, K), device=dev, generator=gen, dtype=torch.uint8)
        res = torch.randint(0, 256, (M, N), device=dev, generator=gen, dtype=torch.uint8)
        plan = E.lindec_w8_plan(M, N, K)
        assert plan["served"] and plan["store"] == "packets"
        t = ops.lsq_linear_w8_q8(x, s_x, zx, ws[0], w_s, w_z, bias, torch.float32).flatten().double()
        lo, hi = t.quantile(0.02), t.quantile(0.98)         # the output quantizer: the results' 2nd to 98th percentile on 0..255
        osc = ((hi - lo) / 255).float().reshape(1)
        osh = (-torch.round(-lo / osc.double()) * osc.double()).float().reshape(1)
        tail = (s_r * 0 + osc * 0.4, z_r, None, None, 0, 255, 0, 255)
        del t

        def new(i):
            if residual:
                return ops.lsq_linear_w8_q8_dec_add_q(x, s_x, zx, ws[i], w_s, w_z, bias, osc, osh, *RNG, False, torch.bfloat16, res, *tail)
            return ops.lsq_linear_w8_q8_dec_q(x, s_x, zx, ws[i], w_s, w_z, bias, osc, osh, *RNG, False, torch.bfloat16)

        def parent(i):
            if residual:
                return ops.lsq_linear_w8_q8_add_q(x, s_x, zx, ws[i], w_s, w_z, bias, osc, osh, *RNG, False, torch.bfloat16, res, *tail)
            return ops.lsq_linear_w8_q8_q(x, s_x, zx, ws[i], w_s, w_z, bias, osc, osh, *RNG, False, torch.bfloat16)

        def floats(i):
            y = ops.lsq_linear_w8_q8(x, s_x, zx, ws[i], w_s, w_z, bias, torch.bfloat16)
            return ops.lsq_levels_per_tensor(y, osc, osh, *RNG, 0)

        routes = [new, parent, floats]
        with torch.no_grad():
            y = new(0)
            assert y.shape == (M, N) and y.dtype == torch.uint8 and torch.equal(y, new(0)), "two launches differ"
            assert torch.equal(y, parent(0)), "not the bytes of the parent's route"
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
        tn, tp, tf = med
        mark = "HIT" if tn / tp < 1 - max(spread[0], spread[1]) else "MISS"
        name = "%d x %d%s x %d" % (N, K, "+r" if residual else "", M)
        if mark == "MISS":
            misses.append(name)
        line = "%-22s %5d %4d %5.0f %5d | %8.2f %6.3f %5.1f | %9.2f %6.3f %6.2f %-4s | %8.2f %6.3f %6.2f" % (
            name, iters, nsets, nsets * N * K / 1e6, plan["grid"], tn, spread[0], 100 * N * K / (tn * 1e-6) / PEAK, tp, spread[1], tn / tp,
            mark, tf, spread[2], tn / tf)
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                  # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del graphs, ws
        torch.cuda.empty_cache()
    lines.append("# expectation (new / parent < 1 beyond the spread in every case): %s"
                 % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    lines.append("# what bounds the new kernel (the weight stream, the LDS reduction or the launch): NOT MEASURED (no counter run was made)")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
