#!/usr/bin/env python3
"""A/B: the gated product in the epilogue of the decode-shape gate and up linears on PACKED 4- / 2-bit codes (liblsq_hip_linglu_w4.so:
lsq_linear_packed_q8_glu_q, one launch) against the parent commit's route on the same buffers: uint8 levels in and out, mid_dtype
bfloat16, SiLU, M in {1, 4, 16}, the gate_up weights [2 x 11008, 4096] and [2 x 14336, 4096] fused (one quantizer) at 4 bits with
G = 128 and G = 32 and at 2 bits with G = 128, and one case with the pair [11008, 4096] + [11008, 4096] under two quantizers.

    new      the 16-wave kernel that streams both code strips, stages x once for both and forms the product in LDS: one launch, [M, C]
             bytes written
    parent   lsq_linear_packed_q8_q (liblsq_hip_lindec_w4.so) on the fused weight ([M, 2 C] bytes written; the pair: twice, [M, C] each),
             then lsq_glu_w8_q8_q on the halves: two launches (the pair: three)

The two routes' bytes are compared for equality, with two launches of the new route and the non-vacuity of the product's quantizer,
before any timing.  Then each route is captured as ONE graph of back-to-back calls, one per WEIGHT set, over as many weight sets as
exceed the 256 MB Infinity Cache by a quarter, and ROUNDS rounds alternate the graphs in one process, timed with HIP events.  Reported:
the median microseconds per call of each route, the spread of a route's rounds ((max - min) / median), new / parent, and the weights'
bytes (codes and group constants) over the new route's time as a share of 8 TB/s.

The expectation is fixed beforehand: new / parent < 1 by more than the measured spread in every case -- one launch fewer (two for the
pair) and 3 M C bytes of traffic dropped, the weight stream unchanged.  `HIT` where new / parent < 1 - the larger of the two routes'
spreads, `MISS` otherwise.  `torchlsq.functional.W4A8_GLU_EPILOGUE_DEFAULT` becomes True only if every case is a HIT.

    python tools/exp_linglu_w4_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (C, K, G, bits, fused, M)
CASES = [(C, 4096, G, bits, True, M) for G, bits in ((128, 4), (32, 4), (128, 2)) for C in (11008, 14336) for M in (1, 4, 16)] + \
        [(11008, 4096, 128, 4, False, 4)]
CACHE_BYTES = 256 << 20
PEAK = 8e12
RNG = (0, 255, 0, 255)
MID = torch.bfloat16


def quantizer(t):
    """(scale [1], shift [1]) of a uint8 quantizer on the 2nd to 98th percentile of t, widened to hold 0"""
    t = t.flatten().double()
    lo, hi = t.quantile(0.02).clamp(max=0.0), t.quantile(0.98).clamp(min=0.0)
    sc = ((hi - lo) / 255).float().reshape(1)
    return sc, (-torch.round(-lo / sc.double()) * sc.double()).float().reshape(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, three cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r39_linglu_w4_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq import functional as F
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [CASES[0], CASES[11], CASES[18]] if args.quick else CASES
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x, zx = torch.tensor([0.0371], device=dev), torch.tensor([117], dtype=torch.int32, device=dev)
    lines = ["# exp_linglu_w4_ab: the gated product in the epilogue of the decode-shape gate and up linears on packed codes "
             "(liblsq_hip_linglu_w4.so, one launch) vs the parent's route (lsq_linear_packed_q8_q with decode once on the fused weight or "
             "twice on the pair, then lsq_glu_w8_q8_q on the halves); %s, %d CUs"
             % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` weight sets of `MB` "
             "megabytes in all (1.25 x the 256 MB cache); spread = (max - min) / median of a route's rounds; uint8 levels in and out, SiLU, "
             "mid_dtype bfloat16; the new route's bytes checked against the parent's on the same inputs before any timing; %%: weight "
             "bytes / time over 8 TB/s; HIT: new / parent < 1 - the larger spread of the two" % rounds,
             "%-34s %5s %4s %5s %5s | %8s %6s %5s | %9s %6s %6s %-4s" % (
                 "C x K x M, bits / G", "calls", "sets", "MB", "grid", "new us", "spread", "%", "parent us", "spread", "new/p", "")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    misses = []
    for C, K, G, bits, fused, M in cases:
        wbytes = 2 * C * (K * bits // 8 + K // G * 8)
        nsets = -(-CACHE_BYTES * 5 // 4 // wbytes)
        iters = max(args.iters, nsets)
        cs = [torch.randint(0, 256, (2 * C, K * bits // 8), device=dev, generator=gen, dtype=torch.uint8) for _ in range(nsets)]
        qs = [(torch.rand(2 * C * (K // G), device=dev, generator=gen) * 0.02 + 0.005) for _ in range(nsets)]
        qz = [torch.randint(0, 2 ** bits, (2 * C * (K // G),), device=dev, generator=gen, dtype=torch.int32) for _ in range(nsets)]
        bias = torch.randn(2 * C, device=dev, generator=gen)
        x = torch.randint(0, 256, (M, K), device=dev, generator=gen, dtype=torch.uint8)
        plan = E.linglu_w4_plan(M, C, K, G, bits)
        assert plan["served"] and plan["store"] == "packets"
        t = ops.lsq_linear_packed_q8(x, s_x, zx, cs[0], qs[0], qz[0], bias, G, bits, torch.float32)
        gq = quantizer(t if fused else t[:, :C])            # the pair: a quantizer each; fused: one on both halves
        uq = gq if fused else quantizer(t[:, C:])
        (s_g, z_g), (s_u, z_u) = F._act_constants(*gq, 0, 255), F._act_constants(*uq, 0, 255)
        table = F.lsq_glu_table("silu", s_g, z_g, torch.uint8, None, MID)
        gate_l = ops.lsq_levels_per_tensor(t[:, :C].contiguous(), *gq, *RNG, 0).view(torch.uint8)
        up_l = ops.lsq_levels_per_tensor(t[:, C:].contiguous(), *uq, *RNG, 0).view(torch.uint8)
        oq = quantizer(ops.lsq_glu_w8_q8(gate_l, up_l, s_u, z_u, table, torch.float32))
        del t, gate_l, up_l
        ng = C * (K // G)

        def halves(i):
            return (cs[i][:C], qs[i][:ng], qz[i][:ng], bias[:C]), (cs[i][C:], qs[i][ng:], qz[i][ng:], bias[C:])

        def new(i):
            g, u = halves(i)
            return ops.lsq_linear_packed_q8_glu_q(x, s_x, zx, *g, *gq, *RNG, *u, *uq, *RNG, G, bits, s_u, z_u, table, *oq, *RNG, MID)

        def parent(i):
            if fused:
                gu = ops.lsq_linear_packed_q8_q(x, s_x, zx, cs[i], qs[i], qz[i], bias, G, bits, *gq, *RNG, False, MID, True)
                gl, ul = gu[:, :C], gu[:, C:]
            else:
                g, u = halves(i)
                gl = ops.lsq_linear_packed_q8_q(x, s_x, zx, *g, G, bits, *gq, *RNG, False, MID, True)
                ul = ops.lsq_linear_packed_q8_q(x, s_x, zx, *u, G, bits, *uq, *RNG, False, MID, True)
            return ops.lsq_glu_w8_q8_q(gl, ul, s_u, z_u, table, *oq, *RNG, MID)

        routes = [new, parent]
        with torch.no_grad():
            y = new(0)
            assert y.shape == (M, C) and y.dtype == torch.uint8 and torch.equal(y, new(0)), "two launches differ"
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
        tn, tp = med
        mark = "HIT" if tn / tp < 1 - max(spread) else "MISS"
        name = "%s%d x %d x %d, %d / %d" % ("2 x " if fused else "pair ", C, K, M, bits, G)
        if mark == "MISS":
            misses.append("%s (%.2f)" % (name, tn / tp))
        line = "%-34s %5d %4d %5.0f %5d | %8.2f %6.3f %5.1f | %9.2f %6.3f %6.2f %-4s" % (
            name, iters, nsets, nsets * wbytes / 1e6, plan["grid"], tn, spread[0], 100 * wbytes / (tn * 1e-6) / PEAK, tp, spread[1],
            tn / tp, mark)
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                  # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del graphs, cs, qs, qz
        torch.cuda.empty_cache()
    lines.append("# expectation (new / parent < 1 beyond the spread in every case): %s"
                 % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    lines.append("# what bounds the new kernel (the weight stream, the LDS reduction or the launch): NOT MEASURED (no counter run was made)")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
