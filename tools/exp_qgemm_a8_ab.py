#!/usr/bin/env python3
"""A/B: the int8 matrix-core GEMM on packed weights (liblsq_hip_qgemm_a8.so, the route of lsq_linear_packed_q8 /
lsq_linear_packed_a8 from `qgemm_a8_min_rows()` rows on) against the two routes the same call has, on the same buffers.

    new  lsq_qgemm_a8_forward_levels / lsq_qgemm_a8_forward, one call      reads the codes once per 128-row tile
    (a)  the decode kernel 16 rows at a time (_launch_row_blocks)          the route before the GEMM existed: ceil(M / 16)
                                                                           launches, the SAME BITS -- a pure time comparison
    (b)  lsq_linear_packed (the float GEMM of liblsq_hip_qgemm.so) on an   what a user without the 8-bit path runs; another
         x fake-quantized beforehand (bfloat16)                            order of another sum: no bits in common

Per case (input form x M x weight shape x (bits, G)): the new route's result is compared bit for bit with route (a)'s, its
first 17 rows are held to the bound of include/lsq_hip_qlinear_a8.h against exact integer group sums in fp64 on the device,
and two launches are compared bit for bit; then each route is captured as ONE graph of ITERS back-to-back calls over weight
sets rotated so that the streamed working set exceeds the 256 MB Infinity Cache where ITERS sets reach that far (a `*` after
the weight marks the cases where they do not), and ROUNDS rounds alternate the graphs in one process, timed with HIP
events.  Reported: the median microseconds per call of each route, the spread of the new route's rounds ((max - min) /
median), its int8 TOP/s (2 M N K / time), and the ratios new / (a), new / (b).

Expectation, marked per line: new / (a) < 1.0 at M = 512 and 2048 (`met` / `MISS`).  The summary names, per input form, the
smallest measured M from which new / (a) <= 1.0 + the file's largest spread in every format: the threshold of rows.

    python tools/exp_qgemm_a8_ab.py [--quick] [--form levels|fused] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008)]
FORMATS = [(4, 32), (4, 128), (2, 128)]         # (bits, G)
ROWS = [17, 32, 64, 128, 512, 2048]
CACHE_BYTES = 256 << 20
S_X, ZX = 0.02, 125                             # the fused form's quantizer: scale 0.02, shift -2.5, levels 0..255


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, one weight shape, three row counts")
    ap.add_argument("--form", choices=["levels", "fused"], help="one input form only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_qgemm_a8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import _qlinear_a8_host as H
    from torchlsq import extension as E
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    shapes = SHAPES[:1] if args.quick else SHAPES
    rows = [17, 128, 2048] if args.quick else ROWS
    forms = [args.form] if args.form else ["levels", "fused"]
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x = torch.tensor([S_X], device=dev)
    zx = torch.tensor([ZX], dtype=torch.int32, device=dev)
    sc, sh = torch.tensor([S_X], device=dev), torch.tensor([-S_X * ZX], device=dev)
    lines = ["# exp_qgemm_a8_ab: the int8 GEMM on packed codes (liblsq_hip_qgemm_a8.so) vs (a) the decode kernel 16 rows at a time "
             "(the route before; the same bits), (b) the float GEMM lsq_linear_packed on a bfloat16 x fake-quantized beforehand; "
             "%s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds x %d back-to-back calls in one captured graph per route, weight sets rotated past "
             "the 256 MB cache (* = the %d code sets stay below it); spread = (max - min) / median of the new route's rounds; "
             "levels: uint8 levels in, bfloat16 y; fused: bfloat16 x in" % (rounds, args.iters, args.iters),
             "%-6s %4s %-12s %4s %3s | %9s %6s %7s | %9s %9s | %6s %6s | %s" % (
                 "form", "M", "weight", "bits", "G", "new us", "spread", "TOP/s", "(a) us", "(b) us", "new/a", "new/b", "expectation")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    ratios, spreads, misses = {}, [], []
    for form in forms:
        for (N, K) in shapes:
            for bits, G in FORMATS:
                code_bytes = N * K * bits // 8
                nsets = min(args.iters, -(-CACHE_BYTES * 5 // 4 // code_bytes))
                short = "*" if nsets * code_bytes < CACHE_BYTES else ""
                codes = [torch.randint(0, 256, (N, K * bits // 8), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nsets)]
                qs = (torch.rand(N * K // G, device=dev, generator=gen) * 0.05 + 0.01)
                qz = torch.randint(0, 2 ** bits, (N * K // G,), dtype=torch.int32, device=dev, generator=gen)
                per = 8 // bits
                c0 = torch.stack([(codes[0].to(torch.int32) >> (j * bits)) & (2 ** bits - 1) for j in range(per)], dim=-1)
                cz = (c0.reshape(N, K // G, G) - qz.reshape(N, K // G, 1)).double()
                del c0
                for M in rows:
                    assert E.qgemm_a8_plan(M, N, K, G, bits)["form"] == "mfma"
                    xf = (torch.randn(M, K, device=dev, generator=gen) * 1.2 + 0.1).to(torch.bfloat16)
                    lx = torch.ops.torchlsq.lsq_levels_per_tensor(xf, sc, sh, 0, 255, 0, 255, 0).view(torch.uint8)
                    xq = ((lx.float() - ZX) * S_X).to(torch.bfloat16)        # x fake-quantized beforehand

                    if form == "levels":
                        def new(i):
                            return E.qgemm_a8_forward_levels(lx, s_x, zx, codes[i], qs, qz, None, G, bits, torch.bfloat16)

                        def old(i):
                            return H._launch_row_blocks("lsq_qlinear_a8_forward_levels", E.LSQ_A8_U8, lx, (s_x.data_ptr(), zx.data_ptr()),
                                                        codes[i], qs, qz, None, G, bits, torch.bfloat16, (E.LSQ_BF16,))
                    else:
                        def new(i):
                            return E.qgemm_a8_forward(xf, sc, sh, 0, 255, 0, 255, codes[i], qs, qz, None, G, bits)

                        def old(i):
                            return H._launch_row_blocks("lsq_qlinear_a8_forward", E.LSQ_BF16, xf,
                                                        (sc.data_ptr(), sh.data_ptr(), 0, 255, 0, 255), codes[i], qs, qz, None, G, bits,
                                                        torch.bfloat16)

                    def flt(i):
                        return torch.ops.torchlsq.lsq_linear_packed(xq, codes[i], qs, qz, None, G, bits)

                    # bits, bound and repeatability before any timing
                    y = new(0)
                    assert torch.equal(y.view(torch.int16), old(0).view(torch.int16)), "new route != the decode kernel's bits"
                    assert torch.equal(y.view(torch.int16), new(0).view(torch.int16)), "two launches differ"
                    a = (lx[:17].to(torch.int64) - ZX).double().reshape(17, K // G, G)
                    I = torch.einsum("mgk,ngk->mng", a, cz)
                    r = S_X * (I * qs.double().reshape(N, K // G)).sum(-1)
                    Eb = (K // G + 8) * 2.0 ** -24 * S_X * (I.abs() * qs.double().reshape(N, K // G)).sum(-1)
                    worst = float(((y[:17].double() - r).abs() / (Eb + 2.0 ** -8 * (r.abs() + Eb))).max())
                    assert worst <= 1.0, "new route outside the bound: %.3f" % worst
                    del a, I, r, Eb, y

                    graphs = []
                    for fn in (new, old, flt):
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
                    key = (form, "%dx%d" % (N, K), bits, G)
                    ratios[key + (M,)] = tn / ta
                    mark = ""
                    if M >= 512:
                        mark = "met" if tn / ta < 1.0 else "MISS"
                        if tn / ta >= 1.0:
                            misses.append(key + (M,))
                    line = "%-6s %4d %-12s %4d %3d | %9.1f %6.3f %7.1f | %9.1f %9.1f | %6.2f %6.2f | %s" % (
                        form, M, key[1] + short, bits, G, tn, spread, 2.0 * M * N * K / (tn * 1e-6) / 1e12, ta, tb, tn / ta, tn / tb, mark)
                    print(line, flush=True)
                    lines.append(line)
                    with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
                        f.write("\n".join(lines) + "\n")
                    del graphs
                del codes, cz
                torch.cuda.empty_cache()
    worst_spread = max(spreads)
    lines.append("# largest spread of the new route's rounds: %.3f" % worst_spread)
    lines.append("# new / (a) < 1.0 at M = 512 and 2048: %s" % ("every case" if not misses else "MISS: " + ", ".join(
        "%s %s %d bits G %d M %d" % k for k in misses)))
    for form in forms:
        keys = sorted({k[:4] for k in ratios if k[0] == form})
        ok_from = None
        for M in reversed(rows):
            if all(ratios[k + (M,)] <= 1.0 + worst_spread for k in keys):
                ok_from = M
            else:
                break
        lines.append("# %s: new / (a) <= 1.0 + %.3f in every format from M = %s on" % (
            form, worst_spread, ok_from if ok_from is not None else "none of the measured M"))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-(2 + len(forms)):]))


if __name__ == "__main__":
    main()
