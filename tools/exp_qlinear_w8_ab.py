#!/usr/bin/env python3
"""A/B: the W8A8 linear on per-channel 8-bit weight levels (liblsq_hip_qlinear_w8.so, lsq_linear_w8_q8 / lsq_linear_w8_a8)
against the two routes a user had before it, on the same shapes.

    new  lsq_linear_w8_q8 (uint8 levels in, bfloat16 y) / lsq_linear_w8_a8 (bfloat16 x in)      N * K bytes of weight
    (a)  F.linear in bfloat16 on the dequantized weight                                         2 N K bytes: the only route
         the parent commit offers an 8-bit per-channel model
    (b)  lsq_linear_packed_q8 / lsq_linear_packed_a8 at 4 bits, G = 128, on the same shape      N K / 2 bytes, an unpack and a
         per-group fold

Per case (input form x M x weight shape): the new route's rows (the first 128 and the last 16) are compared BIT FOR BIT with
the definition -- the exact integer matrix from a float64 product on the device (|I| < 2^53), then the contract's fp32 steps
as individually rounded tensor operations -- and two launches are compared bit for bit; then each route is captured as ONE
graph of ITERS back-to-back calls over weight sets rotated so that the streamed working set exceeds the 256 MB Infinity
Cache (a `*` after the weight marks the cases where the sets of a route do not reach that far), and ROUNDS rounds alternate
the graphs in one process, timed with HIP events.  Reported: the median microseconds per call of each route, the spread of
the new route's rounds ((max - min) / median), the share of an 8 TB/s stream of the N * K weight bytes (M <= 16), the int8
TOP/s (2 M N K / time), and the ratios new / (a), new / (b).

Expectations from byte counts and MFMA rates, marked per line (`met` / `MISS`): new / (a) < 1.0 at M <= 16 and at M >= 512;
new / (b) < 1.0 at M >= 512.

    python tools/exp_qlinear_w8_ab.py [--quick] [--form levels|fused] [--out FILE]
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
ROWS = [1, 16, 128, 512, 2048]
CACHE_BYTES = 256 << 20
STREAM_BYTES_PER_S = 8e12
S_X, ZX = 0.02, 125                             # the activation quantizer: scale 0.02, shift -2.5, levels 0..255
BITS, G = 4, 128                                # route (b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, one weight shape, three row counts")
    ap.add_argument("--form", choices=["levels", "fused"], help="one input form only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_qlinear_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    shapes = SHAPES[:1] if args.quick else SHAPES
    rows = [1, 128, 2048] if args.quick else ROWS
    forms = [args.form] if args.form else ["levels", "fused"]
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x = torch.tensor([S_X], device=dev)
    zx = torch.tensor([ZX], dtype=torch.int32, device=dev)
    sc, sh = torch.tensor([S_X], device=dev), torch.tensor([-S_X * ZX], device=dev)
    lines = ["# exp_qlinear_w8_ab: the W8A8 linear on per-channel int8 weight levels (liblsq_hip_qlinear_w8.so) vs (a) bfloat16 F.linear "
             "on the dequantized weight, (b) the packed 4-bit G = 128 op on 8-bit levels (lsq_linear_packed_q8 / _a8); "
             "%s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds x %d back-to-back calls in one captured graph per route, weight sets rotated past "
             "the 256 MB cache (* = a route's sets stay below it); spread = (max - min) / median of the new route's rounds; "
             "levels: uint8 levels in, bfloat16 y; fused: bfloat16 x in; share = N K bytes / time / 8 TB/s" % (rounds, args.iters),
             "%-6s %4s %-12s %-13s | %9s %6s %6s %7s | %9s %9s | %6s %6s | %s" % (
                 "form", "M", "weight", "shape", "new us", "spread", "share", "TOP/s", "(a) us", "(b) us", "new/a", "new/b", "expectation")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    spreads, misses = [], []
    for form in forms:
        for (N, K) in shapes:
            nsets = min(args.iters, -(-CACHE_BYTES * 5 // 4 // (N * K // 2)))      # sized by the smallest route's bytes
            short = "*" if nsets * (N * K // 2) < CACHE_BYTES else ""
            lw = [torch.randint(-128, 128, (N, K), dtype=torch.int8, device=dev, generator=gen) for _ in range(nsets)]
            s_w = torch.rand(N, device=dev, generator=gen) * 0.02 + 0.001
            zw = torch.randint(-9, 10, (N,), dtype=torch.int32, device=dev, generator=gen)
            wd = [((w.float() - zw.reshape(-1, 1).float()) * s_w.reshape(-1, 1)).to(torch.bfloat16) for w in lw]
            codes = [torch.randint(0, 256, (N, K * BITS // 8), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nsets)]
            qs = torch.rand(N * K // G, device=dev, generator=gen) * 0.05 + 0.01
            qz = torch.randint(0, 2 ** BITS, (N * K // G,), dtype=torch.int32, device=dev, generator=gen)
            wz64 = (lw[0].double() - zw.reshape(-1, 1).double())
            for M in rows:
                plan = E.qlinear_w8_plan(M, N, K)
                assert plan["form"] == "mfma"
                xf = (torch.randn(M, K, device=dev, generator=gen) * 1.2 + 0.1).to(torch.bfloat16)
                lx = torch.ops.torchlsq.lsq_levels_per_tensor(xf, sc, sh, 0, 255, 0, 255, 0).view(torch.uint8)
                xq = ((lx.float() - ZX) * S_X).to(torch.bfloat16)        # x fake-quantized beforehand

                if form == "levels":
                    def new(i):
                        return torch.ops.torchlsq.lsq_linear_w8_q8(lx, s_x, zx, lw[i], s_w, zw, None, torch.bfloat16)

                    def dense(i):
                        return F.linear(xq, wd[i])

                    def packed(i):
                        return torch.ops.torchlsq.lsq_linear_packed_q8(lx, s_x, zx, codes[i], qs, qz, None, G, BITS, torch.bfloat16)
                else:
                    def new(i):
                        return torch.ops.torchlsq.lsq_linear_w8_a8(xf, sc, sh, 0, 255, 0, 255, lw[i], s_w, zw, None)

                    def dense(i):
                        return F.linear(xf, wd[i])

                    def packed(i):
                        return torch.ops.torchlsq.lsq_linear_packed_a8(xf, sc, sh, 0, 255, 0, 255, codes[i], qs, qz, None, G, BITS)

                # the bits of the definition and repeatability before any timing
                y = new(0)
                assert torch.equal(y.view(torch.int16), new(0).view(torch.int16)), "two launches differ"
                pick = torch.unique(torch.cat([torch.arange(min(M, 128)), torch.arange(max(0, M - 16), M)])).to(dev)
                I = (lx[pick].double() - ZX) @ wz64.t()                     # exact: |I| < 2^53
                want = ((s_w.reshape(1, -1) * I.float()) * s_x).to(torch.bfloat16)
                assert torch.equal(y[pick].view(torch.int16), want.view(torch.int16)), "not the bits of the definition"
                del I, want, y

                graphs = []
                for fn in (new, dense, packed):
                    def run(fn=fn):
                        for i in range(args.iters):
                            fn(i % nsets)
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        run()
                    torch.cuda.current_stream().wait_stream(side)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        run()
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
                tn, ta, tb = (statistics.median(t[1:]) for t in times)
                spread = (max(times[0][1:]) - min(times[0][1:])) / tn
                spreads.append(spread)
                marks = []
                if M <= 16 or M >= 512:
                    marks.append("a:met" if tn / ta < 1.0 else "a:MISS")
                if M >= 512:
                    marks.append("b:met" if tn / tb < 1.0 else "b:MISS")
                misses += ["%s M %d %dx%d %s" % (form, M, N, K, m[0]) for m in marks if m.endswith("MISS")]
                share = "%6.2f" % (N * K / (tn * 1e-6) / STREAM_BYTES_PER_S) if M <= 16 else "%6s" % "-"
                line = "%-6s %4d %-12s %-13s | %9.1f %6.3f %s %7.1f | %9.1f %9.1f | %6.2f %6.2f | %s" % (
                    form, M, "%dx%d%s" % (N, K, short), plan["shape"], tn, spread, share, 2.0 * M * N * K / (tn * 1e-6) / 1e12, ta, tb,
                    tn / ta, tn / tb, " ".join(marks))
                print(line, flush=True)
                lines.append(line)
                with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
                    f.write("\n".join(lines) + "\n")
                del graphs
            del lw, wd, codes, wz64
            torch.cuda.empty_cache()
    lines.append("# largest spread of the new route's rounds: %.3f" % max(spreads))
    lines.append("# expectations (new / (a) < 1.0 at M <= 16 and M >= 512, new / (b) < 1.0 at M >= 512): %s" % (
        "every case met" if not misses else "MISS: " + "; ".join(misses)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
