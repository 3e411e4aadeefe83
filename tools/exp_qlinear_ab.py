#!/usr/bin/env python3
"""A/B: the linear op on packed weights (liblsq_hip_qlinear.so, torch.ops.torchlsq.lsq_linear_packed) against the two routes
a user had before it, on the same buffers.

    new  lsq_linear_packed(x, codes, scale, zero_point)            reads the codes, writes y
    (a)  p.dequantize(x.dtype) then F.linear                       what packed storage cost: write and re-read the full weight
    (b)  F.linear on a weight dequantized once beforehand           no packing at all: 4 x / 8 x the weight memory

Per case (dtype x M x weight shape x G x bits): the new route's result is held to the accuracy bound of
include/lsq_hip_qlinear.h against an fp64 product on the device and two launches are compared bit for bit; then each route
is captured as ONE graph of ITERS back-to-back calls over weight sets rotated so that the streamed working set exceeds the
256 MB Infinity Cache (every read of a weight comes from HBM; the graph keeps the host out of the numbers), and ROUNDS
rounds alternate the three graphs in one process, timed with HIP events.  Reported: the median microseconds per call of
each route, the spread of the new route's rounds ((max - min) / median), the new route's share of the 8 TB/s roofline at
N K bits / 8 + 8 N K / G + (M K + M N) sizeof(x) bytes, and the ratios new / (a) and new / (b).

    python tools/exp_qlinear_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008)]
GROUPS = [32, 128]
DTYPES = [torch.bfloat16, torch.float16]
BITS = [4, 2]
ROWS = [1, 4, 16]
ROOFLINE = 8.0e12
CACHE_BYTES = 256 << 20
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds and one weight shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_qlinear_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    op = torch.ops.torchlsq.lsq_linear_packed
    deq = torch.ops.torchlsq.lsq_dequantize_per_group
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    shapes = SHAPES[:1] if args.quick else SHAPES
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = ["# exp_qlinear_ab: lsq_linear_packed (liblsq_hip_qlinear.so) vs (a) dequantize + F.linear and (b) F.linear on a "
             "weight dequantized beforehand; %s, %d CUs" % (torch.cuda.get_device_name(0),
                                                            torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds x %d back-to-back calls in one captured graph per route, weight sets rotated past "
             "the 256 MB cache; roofline 8 TB/s; spread = (max - min) / median of the new route's rounds" % (rounds, args.iters),
             "%-8s %2s %-12s %4s %4s | %8s %6s %5s | %8s %8s | %6s %6s" % ("dtype", "M", "weight", "G", "bits", "new us", "spread",
                                                                        "roof", "(a) us", "(b) us", "new/a", "new/b")]
    print("\n".join(lines))
    for dtype in DTYPES:
        for (N, K) in shapes:
            for G in GROUPS:
                for bits in BITS:
                    esize = 2
                    code_bytes = N * K * bits // 8
                    nsets = min(args.iters, -(-CACHE_BYTES * 5 // 4 // code_bytes))
                    nsets_b = min(args.iters, -(-CACHE_BYTES * 5 // 4 // (N * K * esize)))
                    codes = [torch.randint(0, 256, (N, K * bits // 8), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nsets)]
                    qs = (torch.rand(N * K // G, device=dev, generator=gen) * 0.05 + 0.01)
                    qz = torch.randint(0, 2 ** bits, (N * K // G,), dtype=torch.int32, device=dev, generator=gen)
                    dense = [deq(codes[i], qs, qz, G, bits, dtype) for i in range(nsets_b)]
                    for M in ROWS:
                        x = torch.randn(M, K, device=dev, generator=gen).to(dtype)
                        # the bound and bit-identity, before any timing
                        y = op(x, codes[0], qs, qz, None, G, bits)
                        w64 = deq(codes[0], qs, qz, G, bits, torch.float32).double()
                        r = x.double() @ w64.t()
                        E = (K + 8) * 2.0 ** -24 * (x.double().abs() @ w64.abs().t())
                        bound = E + U[dtype] * (r.abs() + E) + (2.0 ** -24 if dtype == torch.float16 else 0.0)
                        worst = float(((y.double() - r).abs() / bound).max())
                        assert worst <= 1.0, "new route outside the bound: %.3f" % worst
                        assert torch.equal(y, op(x, codes[0], qs, qz, None, G, bits)), "two launches differ"
                        del w64, r, E, bound

                        def run_new():
                            for i in range(args.iters):
                                op(x, codes[i % nsets], qs, qz, None, G, bits)

                        def run_a():
                            for i in range(args.iters):
                                F.linear(x, deq(codes[i % nsets], qs, qz, G, bits, dtype))

                        def run_b():
                            for i in range(args.iters):
                                F.linear(x, dense[i % nsets_b])

                        graphs = []
                        for fn in (run_new, run_a, run_b):
                            side = torch.cuda.Stream()
                            side.wait_stream(torch.cuda.current_stream())
                            with torch.cuda.stream(side):
                                fn()
                            torch.cuda.current_stream().wait_stream(side)
                            g = torch.cuda.CUDAGraph()
                            with torch.cuda.graph(g):
                                fn()
                            graphs.append(g)
                        times = [[], [], []]
                        for _ in range(rounds + 1):                 # the first round warms up
                            for k, g in enumerate(graphs):
                                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                t0.record()
                                g.replay()
                                t1.record()
                                t1.synchronize()
                                times[k].append(t0.elapsed_time(t1) * 1e3 / args.iters)
                        new, a, b = (statistics.median(t[1:]) for t in times)
                        spread = (max(times[0][1:]) - min(times[0][1:])) / new
                        algo = N * K * bits / 8.0 + 8.0 * N * K / G + (M * K + M * N) * esize
                        line = "%-8s %2d %-12s %4d %4d | %8.1f %6.3f %5.2f | %8.1f %8.1f | %6.2f %6.2f" % (
                            str(dtype).replace("torch.", ""), M, "%dx%d" % (N, K), G, bits, new, spread, algo / ROOFLINE / (new * 1e-6),
                            a, b, new / a, new / b)
                        print(line, flush=True)
                        lines.append(line)
                        del graphs
                    del codes, dense
                    torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
