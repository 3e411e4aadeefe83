#!/usr/bin/env python3
"""A/B: the decode shape of the W4A8 / W2A8 linears with an 8-bit output (liblsq_hip_lindec_w4.so: lsq_linear_packed_q8_q /
lsq_linear_packed_q8_add_q with decode=True) against what the parent commit offers on the same inputs: uint8 levels in and out, packed
group-wise codes (4 bits at G = 128 and G = 32, 2 bits at G = 128), mid_dtype bfloat16, M in {1, 4, 16}, the four linears of a
4096-wide decoder layer: [4096, 4096], [6144, 4096], [22016, 4096] and [4096, 11008] + a levels residual.

    new      one launch of the 16-wave kernel that streams the codes and writes the levels
    parent   the composition: lsq_linear_packed_q8 (bfloat16 y), the residual's dequantize and add in torch, lsq_levels_per_tensor
             (the same ops with decode=False)
    w8       lsq_linear_w8_q8_dec_q / _dec_add_q (liblsq_hip_lindec_w8.so) on int8 weight levels of the same [N, K], for information:
             by bytes the new route moves about bits / 8 + 8 / G of what it moves

The two packed routes are compared for equality, with two launches of the new route and the non-vacuity of the output quantizer, before
any timing.  Then each route is captured as ONE graph of back-to-back calls, one per WEIGHT set, over as many weight sets as exceed the
256 MB Infinity Cache by a quarter, and ROUNDS rounds alternate the graphs in one process, timed with HIP events.  Reported: the median
microseconds per call of each route, the spread of a route's rounds ((max - min) / median), new / parent, new / w8, and the packed
weight's bytes (codes, qscale, qzero) over the new route's time as a share of 8 TB/s.

No ratio is fixed beforehand.  `HIT` where new / parent < 1 - the larger of the two routes' spreads, `MISS` otherwise;
`torchlsq.functional.W4A8_DECODE_DEFAULT` is True only if every case is a HIT.

    python tools/exp_lindec_w4_ab.py [--quick] [--out FILE]
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
FORMATS = [(4, 128), (4, 32), (2, 128)]     # (bits, G)
CACHE_BYTES = 256 << 20
PEAK = 8e12
RNG = (0, 255, 0, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, three cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r38_lindec_w4_ab.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [(fmt, layer, M) for fmt in FORMATS for layer in LAYERS for M in ROWS]
    if args.quick:
        cases = [cases[0], cases[17], cases[35]]
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x, zx = torch.tensor([0.0371], device=dev), torch.tensor([117], dtype=torch.int32, device=dev)
    z_r = torch.tensor([128], dtype=torch.int32, device=dev)
    lines = ["# exp_lindec_w4_ab: the decode shape of the W4A8 / W2A8 linears with an 8-bit output (liblsq_hip_lindec_w4.so, one launch) vs the "
             "parent's composition (lsq_linear_packed_q8 -> torch add -> lsq_levels_per_tensor) vs liblsq_hip_lindec_w8.so on int8 weights of "
             "the same shape; %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` weight sets of `MB` "
             "megabytes in all (1.25 x the 256 MB cache); spread = (max - min) / median of a route's rounds; uint8 levels in and out, "
             "mid_dtype bfloat16; the new route's bytes checked against the parent's on the same inputs before any timing; %%: the packed "
             "weight's bytes / time over 8 TB/s; HIT: new / parent < 1 - the larger spread of the two; bytes: (bits / 8 + 8 / G), the packed "
             "weight's share of the int8 weight's bytes" % rounds,
             "%-4s %-22s %5s %4s %5s %5s | %8s %6s %5s | %9s %6s %6s %-4s | %8s %6s %6s %5s" % (
                 "b/G", "N x K x M", "calls", "sets", "MB", "grid", "new us", "spread", "%", "parent us", "spread", "new/p", "", "w8 us",
                 "spread", "new/w8", "bytes")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    misses = []
    for (bits, G), (N, K, residual), M in cases:
        wbytes = N * K * bits // 8 + N * (K // G) * 8
        nsets = -(-CACHE_BYTES * 5 // 4 // wbytes)
        nsets8 = -(-CACHE_BYTES * 5 // 4 // (N * K))
        iters = max(args.iters, nsets)
        codes = [torch.randint(0, 256, (N, K * bits // 8), device=dev, generator=gen, dtype=torch.uint8) for _ in range(nsets)]
        qs = torch.rand(N * (K // G), device=dev, generator=gen) * 0.02 + 0.005
        qz = torch.randint(0, 1 << bits, (N * (K // G),), device=dev, generator=gen, dtype=torch.int32)
        w8 = [torch.randint(-128, 128, (N, K), device=dev, generator=gen, dtype=torch.int8) for _ in range(nsets8)]
        w8_s = torch.rand(N, device=dev, generator=gen) * 0.002 + 0.0005
        w8_z = torch.zeros(N, dtype=torch.int32, device=dev)
        bias = torch.randn(N, device=dev, generator=gen)
        x = torch.randint(0, 256, (M, K), device=dev, generator=gen, dtype=torch.uint8)
        res = torch.randint(0, 256, (M, N), device=dev, generator=gen, dtype=torch.uint8)
        plan = E.lindec_w4_plan(M, N, K, G, bits)
        assert plan["served"] and plan["store"] == "packets"
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

        def int8(i):
            w = (w8[i % nsets8], w8_s, w8_z, bias)
            if residual:
                return ops.lsq_linear_w8_q8_dec_add_q(x, s_x, zx, *w, osc, osh, *RNG, False, torch.bfloat16, res, *tail)
            return ops.lsq_linear_w8_q8_dec_q(x, s_x, zx, *w, osc, osh, *RNG, False, torch.bfloat16)

        routes = [lambda i: packed(i, True), lambda i: packed(i, False), int8]
        with torch.no_grad():
            y = packed(0, True)
            assert y.shape == (M, N) and y.dtype == torch.uint8 and torch.equal(y, packed(0, True)), "two launches differ"
            assert torch.equal(y, packed(0, False)), "not the bytes of the composition"
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
        tn, tp, t8 = med
        mark = "HIT" if tn / tp < 1 - max(spread[0], spread[1]) else "MISS"
        name = "%d x %d%s x %d" % (N, K, "+r" if residual else "", M)
        if mark == "MISS":
            misses.append("%d/%d %s" % (bits, G, name))
        line = "%-4s %-22s %5d %4d %5.0f %5d | %8.2f %6.3f %5.1f | %9.2f %6.3f %6.2f %-4s | %8.2f %6.3f %6.2f %5.2f" % (
            "%d/%d" % (bits, G), name, iters, nsets, nsets * wbytes / 1e6, plan["grid"], tn, spread[0], 100 * wbytes / (tn * 1e-6) / PEAK,
            tp, spread[1], tn / tp, mark, t8, spread[2], tn / t8, wbytes / (N * K))
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                  # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del graphs, codes, w8
        torch.cuda.empty_cache()
    lines.append("# new / parent < 1 beyond the spread: %s" % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    lines.append("# what bounds the new kernel (the weight stream, the LDS reduction or the launch): NOT MEASURED (no counter run was made)")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
