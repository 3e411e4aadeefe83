#!/usr/bin/env python3
"""A/B: the matrix-core GEMM on packed weights (liblsq_hip_qgemm.so, the route of torch.ops.torchlsq.lsq_linear_packed for
more than 16 rows of bfloat16 / float16 x) against the three routes the same call had or could have taken, on the same
buffers.

    new  lsq_linear_packed(x, codes, scale, zero_point)                  reads the codes, writes y
    (a)  lsq_dequantize_per_group -> float32, F.linear(x.float(), w)     the route this call took before the GEMM existed:
                                                                         the same two steps as the host code made them
    (b)  F.linear in x's dtype on a weight dequantized beforehand         what a user without packing runs; NOT accuracy-equal
                                                                         (the weight is rounded to 16 bits with its scale)
    (c)  the decode kernel, 16 rows of x at a time                        liblsq_hip_qlinear.so, ceil(M / 16) launches

Per case (dtype x M x weight shape x (bits, G)): the new route's result is held to the accuracy bound of
include/lsq_hip_qgemm.h against an fp64 product on the device, two launches are compared bit for bit and row 16 of the
call to row 16 of the 17-row call; then each route is captured as ONE graph of ITERS back-to-back calls over weight sets
rotated so that the streamed working set exceeds the 256 MB Infinity Cache where ITERS sets reach that far (a `*` after the
weight marks the cases where they do not: small code sets at few iterations), and ROUNDS rounds alternate the four graphs in
one process, timed with HIP events.  Reported: the median microseconds per call of each route, the spread of the new
route's rounds ((max - min) / median), its matrix TFLOP/s (2 M N K / time), its share of the 8 TB/s roofline at
N K bits / 8 + 8 N K / G + (M K + M N) sizeof(x) bytes, and the ratios new / (a), new / (b), new / (c).

Expectations, marked per line and summed up at the end: new / (a) < 1.0 everywhere (`a:met` / `a:MISS`); new / (c) < 1.0
from some M on (`c:met` / `c:MISS`; the crossover per weight is in the summary); new / (b) has no target.

    python tools/exp_qgemm_ab.py [--quick] [--dtype bfloat16|float16] [--out FILE]
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
FORMATS = [(4, 32), (4, 128), (2, 128)]         # (bits, G)
DTYPES = [torch.bfloat16, torch.float16]
ROWS = [17, 32, 64, 128, 512, 2048]
ROOFLINE = 8.0e12
CACHE_BYTES = 256 << 20
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, one weight shape, three row counts")
    ap.add_argument("--dtype", choices=["bfloat16", "float16"], help="one dtype only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_qgemm_ab.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    op = torch.ops.torchlsq.lsq_linear_packed
    deq = torch.ops.torchlsq.lsq_dequantize_per_group
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    shapes = SHAPES[:1] if args.quick else SHAPES
    rows = [17, 128, 2048] if args.quick else ROWS
    dtypes = [getattr(torch, args.dtype)] if args.dtype else DTYPES
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = ["# exp_qgemm_ab: lsq_linear_packed beyond 16 rows (liblsq_hip_qgemm.so) vs (a) dequantize to float32 + float32 F.linear "
             "(the route before), (b) F.linear in x's dtype on a weight dequantized beforehand, (c) the decode kernel 16 rows at a "
             "time; %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds x %d back-to-back calls in one captured graph per route, weight sets rotated past "
             "the 256 MB cache (* = the %d code sets stay below it); roofline 8 TB/s; spread = (max - min) / median of the new "
             "route's rounds" % (rounds, args.iters, args.iters),
             "%-8s %4s %-12s %4s %3s | %9s %6s %7s %5s | %9s %9s %9s | %6s %6s %6s | %s" % (
                 "dtype", "M", "weight", "bits", "G", "new us", "spread", "TFLOP/s", "roof", "(a) us", "(b) us", "(c) us", "new/a",
                 "new/b", "new/c", "expectation")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    miss_a, first_win_c, cases = [], {}, 0
    for dtype in dtypes:
        dname = str(dtype).replace("torch.", "")
        for (N, K) in shapes:
            for bits, G in FORMATS:
                code_bytes = N * K * bits // 8
                nsets = min(args.iters, -(-CACHE_BYTES * 5 // 4 // code_bytes))
                nsets_b = min(args.iters, -(-CACHE_BYTES * 5 // 4 // (N * K * 2)))
                short = "*" if nsets * code_bytes < CACHE_BYTES else ""
                codes = [torch.randint(0, 256, (N, K * bits // 8), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nsets)]
                qs = (torch.rand(N * K // G, device=dev, generator=gen) * 0.05 + 0.01)
                qz = torch.randint(0, 2 ** bits, (N * K // G,), dtype=torch.int32, device=dev, generator=gen)
                dense = [deq(codes[i], qs, qz, G, bits, dtype) for i in range(nsets_b)]
                w64 = deq(codes[0], qs, qz, G, bits, torch.float32).double()
                for M in rows:
                    assert E.qgemm_plan(dtype, M, N, K, G, bits)["form"] == "mfma"
                    x = torch.randn(M, K, device=dev, generator=gen).to(dtype)
                    # the bound and bit-identity, before any timing
                    y = op(x, codes[0], qs, qz, None, G, bits)
                    r = x.double() @ w64.t()
                    Eb = (K + 8) * 2.0 ** -24 * (x.double().abs() @ w64.abs().t())
                    bound = Eb + U[dtype] * (r.abs() + Eb) + (2.0 ** -24 if dtype == torch.float16 else 0.0)
                    worst = float(((y.double() - r).abs() / bound).max())
                    assert worst <= 1.0, "new route outside the bound: %.3f" % worst
                    assert torch.equal(y, op(x, codes[0], qs, qz, None, G, bits)), "two launches differ"
                    assert torch.equal(y[16], op(x[:17], codes[0], qs, qz, None, G, bits)[16]), "row 16 depends on M"
                    del r, Eb, bound, y

                    def run_new():
                        for i in range(args.iters):
                            op(x, codes[i % nsets], qs, qz, None, G, bits)

                    def run_a():        # as the host code made the two steps
                        for i in range(args.iters):
                            w = deq(codes[i % nsets], qs, qz, G, bits, torch.float32)
                            F.linear(x.float(), w, None).to(dtype)

                    def run_b():
                        for i in range(args.iters):
                            F.linear(x, dense[i % nsets_b])

                    def run_c():
                        for i in range(args.iters):
                            for m0 in range(0, M, 16):
                                op(x[m0:m0 + 16], codes[i % nsets], qs, qz, None, G, bits)

                    graphs = []
                    for fn in (run_new, run_a, run_b, run_c):
                        side = torch.cuda.Stream()
                        side.wait_stream(torch.cuda.current_stream())
                        with torch.cuda.stream(side):
                            fn()
                        torch.cuda.current_stream().wait_stream(side)
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            fn()
                        graphs.append(g)
                    times = [[], [], [], []]
                    for _ in range(rounds + 1):                 # the first round warms up
                        for k, g in enumerate(graphs):
                            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            t0.record()
                            g.replay()
                            t1.record()
                            t1.synchronize()
                            times[k].append(t0.elapsed_time(t1) * 1e3 / args.iters)
                    new, a, b, c = (statistics.median(t[1:]) for t in times)
                    spread = (max(times[0][1:]) - min(times[0][1:])) / new
                    algo = N * K * bits / 8.0 + 8.0 * N * K / G + (M * K + M * N) * 2
                    key = (dname, "%dx%d" % (N, K), bits, G)
                    if new / a >= 1.0:
                        miss_a.append(key + (M,))
                    if new / c < 1.0:
                        first_win_c.setdefault(key, M)
                    else:
                        first_win_c.pop(key, None)          # (c) must lose from some M ON
                    cases += 1
                    line = "%-8s %4d %-12s %4d %3d | %9.1f %6.3f %7.1f %5.2f | %9.1f %9.1f %9.1f | %6.2f %6.2f %6.2f | a:%s c:%s" % (
                        dname, M, key[1] + short, bits, G, new, spread, 2.0 * M * N * K / (new * 1e-6) / 1e12,
                        algo / ROOFLINE / (new * 1e-6), a, b, c, new / a, new / b, new / c,
                        "met" if new / a < 1.0 else "MISS", "met" if new / c < 1.0 else "MISS")
                    print(line, flush=True)
                    lines.append(line)
                    with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
                        f.write("\n".join(lines) + "\n")
                    del graphs
                del codes, dense, w64
                torch.cuda.empty_cache()
    lines.append("# new / (a) < 1.0: %d of %d cases%s" % (cases - len(miss_a), cases, "" if not miss_a else "; MISS: " + ", ".join(
        "%s %s %d bits G %d M %d" % k for k in miss_a)))
    for dtype in dtypes:
        dname = str(dtype).replace("torch.", "")
        for (N, K) in shapes:
            for bits, G in FORMATS:
                key = (dname, "%dx%d" % (N, K), bits, G)
                lines.append("# new / (c) < 1.0 for %s %s %d bits G %d: %s" % (key + (
                    "from M = %d on" % first_win_c[key] if key in first_win_c else "MISS at the largest M measured",)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-(1 + len(dtypes) * len(shapes) * len(FORMATS)):]))


if __name__ == "__main__":
    main()
