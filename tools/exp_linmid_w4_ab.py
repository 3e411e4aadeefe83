#!/usr/bin/env python3
"""A/B: the W4A8 / W2A8 linears with an 8-bit output at 17 to 256 rows (liblsq_hip_linmid_w4.so: lsq_linear_packed_q8_q /
lsq_linear_packed_q8_add_q with decode=True; one launch up to 64 rows, one per block of 64 rows beyond) against two alternatives on the
same buffers: uint8 levels in and out, packed group-wise codes (4 bits at G = 128 and G = 32, 2 bits at G = 128), mid_dtype bfloat16,
M in {17, 32, 48, 64, 128, 256}, the four linears of a 4096-wide decoder layer: [4096, 4096] without and with a levels residual,
[6144, 4096], [22016, 4096] and [4096, 11008] + a levels residual.

    new      decode=True: liblsq_hip_linmid_w4.so, the weight streamed once per 64 rows
    auto     what `decode=None` runs when `W4A8_MID_DEFAULT` is on: per block of rows `new` where `_lindec_w4_host._linmid_wins`, else
             `blocks` (the route `kern`: how many of its launches are the new kernel's)
    parent   (a) the composition the parent commit runs (decode=False): lsq_linear_packed_q8 16 rows at a time into a bfloat16 y, the
             residual's dequantize and add in torch, lsq_levels_per_tensor
    blocks   (b) liblsq_hip_lindec_w4.so called ceil(M / 16) times into row slices of one output: host code only

The three routes are compared for equality, with two launches of the new route and the non-vacuity of the output quantizer, before any
timing.  Then each route is captured as ONE graph of back-to-back calls, one per WEIGHT set, over as many weight sets as exceed the
256 MB Infinity Cache by a quarter, and ROUNDS rounds alternate the graphs in one process, timed with HIP events.  Reported: the median
microseconds per call of each route, the spread of a route's rounds ((max - min) / median), new / parent, new / blocks, and the packed
weight's bytes (codes, qscale, qzero) over the new route's time as a share of 8 TB/s.

No ratio is fixed beforehand.  `HIT` where auto / parent < 1 - the larger of the two routes' spreads, `MISS` otherwise;
`torchlsq.functional.W4A8_MID_DEFAULT` is True only if every case is a HIT.  new / parent and new / blocks say where the kernel earns
its place: `p` / `b` mark the cases where it does not beat that route beyond the spread.

    python tools/exp_linmid_w4_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (N, K, residual)
LAYERS = [(4096, 4096, False), (4096, 4096, True), (6144, 4096, False), (22016, 4096, False), (4096, 11008, True)]
ROWS = (17, 32, 48, 64, 128, 256)
FORMATS = [(4, 128), (4, 32), (2, 128)]     # (bits, G)
CACHE_BYTES = 256 << 20
PEAK = 8e12
RNG = (0, 255, 0, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, three cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r41_linmid_w4_ab.txt"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import _lindec_w4_host as H, extension as E
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [(fmt, layer, M) for fmt in FORMATS for layer in LAYERS for M in ROWS]
    if args.quick:
        cases = [cases[3], cases[40], cases[89]]
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x, zx = torch.tensor([0.0371], device=dev), torch.tensor([117], dtype=torch.int32, device=dev)
    z_r = torch.tensor([128], dtype=torch.int32, device=dev)
    lines = ["# exp_linmid_w4_ab: the W4A8 / W2A8 linears with an 8-bit output at 17 to 256 rows (liblsq_hip_linmid_w4.so, one launch per 64 "
             "rows) vs (a) the parent's composition (lsq_linear_packed_q8 -> torch add -> lsq_levels_per_tensor) vs (b) liblsq_hip_lindec_w4.so "
             "called ceil(M / 16) times into row slices; %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` weight sets of `MB` "
             "megabytes in all (1.25 x the 256 MB cache); spread = (max - min) / median of a route's rounds; uint8 levels in and out, "
             "mid_dtype bfloat16; the new route's bytes checked against the parent's on the same inputs before any timing; %%: the packed "
             "weight's bytes / time over 8 TB/s; HIT: auto / parent < 1 - the larger spread of the two; p / b: new does not beat the "
             "parent / the blocks of 16 rows beyond the spread; kern: launches of the new kernel among auto's" % rounds,
             "%-5s %-22s %5s %4s %5s | %8s %6s %5s | %9s %6s %6s | %9s %6s %6s | %8s %6s %6s %4s %-4s" % (
                 "b/G", "N x K x M", "calls", "sets", "MB", "new us", "spread", "%", "parent us", "spread", "new/p", "blocks us",
                 "spread", "new/b", "auto us", "spread", "auto/p", "kern", "")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    misses = []
    for (bits, G), (N, K, residual), M in cases:
        wbytes = N * K * bits // 8 + N * (K // G) * 8
        nsets = -(-CACHE_BYTES * 5 // 4 // wbytes)
        iters = max(args.iters, nsets)
        codes = [torch.randint(0, 256, (N, K * bits // 8), device=dev, generator=gen, dtype=torch.uint8) for _ in range(nsets)]
        qs = torch.rand(N * (K // G), device=dev, generator=gen) * 0.02 + 0.005
        qz = torch.randint(0, 1 << bits, (N * (K // G),), device=dev, generator=gen, dtype=torch.int32)
        bias = torch.randn(N, device=dev, generator=gen)
        x = torch.randint(0, 256, (M, K), device=dev, generator=gen, dtype=torch.uint8)
        res = torch.randint(0, 256, (M, N), device=dev, generator=gen, dtype=torch.uint8)
        plan = E.linmid_w4_plan(min(M, 64), N, K, G, bits)
        assert plan["served"] and plan["store"] == "packets"
        y_b = torch.empty(M, N, dtype=torch.uint8, device=dev)
        t = ops.lsq_linear_packed_q8(x, s_x, zx, codes[0], qs, qz, bias, G, bits, torch.float32).flatten().double()
        lo, hi = t.quantile(0.02), t.quantile(0.98)         # the output quantizer: the results' 2nd to 98th percentile on 0..255
        osc = ((hi - lo) / 255).float().reshape(1)
        osh = (-torch.round(-lo / osc.double()) * osc.double()).float().reshape(1)
        tail = (osc * 0.4, z_r, None, None, 0, 255, 0, 255)
        del t

        def packed(i, decode):
            w = (codes[i % nsets], qs, qz, bias, G, bits)
            if residual:
                return ops.lsq_linear_packed_q8_add_q(x, s_x, zx, *w, osc, osh, *RNG, False, torch.bfloat16, res, *tail, decode)
            return ops.lsq_linear_packed_q8_q(x, s_x, zx, *w, osc, osh, *RNG, False, torch.bfloat16, decode)

        def blocks(i):
            w = (codes[i % nsets], qs, qz, bias, G, bits)
            for m0 in range(0, M, 16):
                if residual:
                    E.lindec_w4_linear_levels_add(x[m0:m0 + 16], s_x, zx, *w, osc, osh, *RNG, False, torch.bfloat16, res[m0:m0 + 16], *tail,
                                                  decode=True, out=y_b[m0:m0 + 16])
                else:
                    E.lindec_w4_linear_levels(x[m0:m0 + 16], s_x, zx, *w, osc, osh, *RNG, False, torch.bfloat16, decode=True, out=y_b[m0:m0 + 16])
            return y_b

        def auto(i):
            with H.measured_routes():
                return packed(i, True)

        routes = [lambda i: packed(i, True), lambda i: packed(i, False), blocks, auto]
        kern = sum(m1 - m0 > 16 for m0, m1 in H._row_blocks(M, N, K, G, bits, x, codes[0], True))
        with torch.no_grad():
            y = packed(0, True)
            assert y.shape == (M, N) and y.dtype == torch.uint8 and torch.equal(y, packed(0, True)), "two launches differ"
            assert torch.equal(y, packed(0, False)), "not the bytes of the composition"
            assert torch.equal(y, blocks(0)), "not the bytes of the blocks of 16 rows"
            assert torch.equal(y, auto(0)), "not the bytes of the measured route"
            inside = ((y > 0) & (y < 255)).float().mean().item()
            assert len(y.unique()) > 32 and 0.25 <= inside and bool((y == 0).any()) and bool((y == 255).any()), \
                "a vacuous output quantizer (%.2f inside)" % inside
            del y
            graphs = []
            for fn_ in routes:
                def run(fn_=fn_):
                    for i in range(iters):
                        fn_(i)
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
        tn, tp, tb, ta = med
        beats = lambda j, k: med[j] / med[k] < 1 - max(spread[j], spread[k])
        mark = "HIT" if beats(3, 1) else "MISS"
        name = "%d x %d%s x %d" % (N, K, "+r" if residual else "", M)
        if mark == "MISS":
            misses.append("%d/%d %s" % (bits, G, name))
        line = "%-5s %-22s %5d %4d %5.0f | %8.2f %6.3f %5.1f | %9.2f %6.3f %5.2f%s | %9.2f %6.3f %5.2f%s | %8.2f %6.3f %6.2f %4d %-4s" % (
            "%d/%d" % (bits, G), name, iters, nsets, nsets * wbytes / 1e6, tn, spread[0], 100 * wbytes / (tn * 1e-6) / PEAK,
            tp, spread[1], tn / tp, " " if beats(0, 1) else "p", tb, spread[2], tn / tb, " " if beats(0, 2) else "b", ta, spread[3], ta / tp,
            kern, mark)
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                  # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del graphs, codes
        torch.cuda.empty_cache()
    lines.append("# auto / parent < 1 beyond the spread: %s" % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    lines.append("# `p` / `b` behind new/p / new/b: the new kernel alone does not beat the parent / the blocks of 16 rows beyond the spread")
    lines.append("# what bounds the new kernel (the weight stream, the staging of x, the LDS reduction or the launch): NOT MEASURED (no counter run was made)")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))


if __name__ == "__main__":
    main()
