#!/usr/bin/env python3
"""A/B: the rotary embedding and the KV-cache append in the epilogue of the decode-shape qkv linear on PACKED 4- / 2-bit codes
(liblsq_hip_linrope_w4.so: lsq_linear_packed_q8_rope_q, one launch) against the parent commit's route on the same buffers: uint8
levels on every side, mid_dtype bfloat16, B = M sequences of one token in {1, 4, 16}, the qkv weights [6144, 4096] (32 q heads, 8 kv
heads, D = 128) and [12288, 4096] (64 and 16) at 4 bits with G = 128 and G = 32 and at 2 bits with G = 128, dense caches and paged pools.

    new      the 16-wave kernel that streams pairs of code strips, stages x once for both and forms the rotation in LDS: one launch,
             the qkv bytes never written
    parent   lsq_linear_packed_q8_q (liblsq_hip_lindec_w4.so), lsq_rope_w8_q8_q on q, then the scattered rotation of k and the copy of
             v (dense) or the rotation of k and lsq_kv_append_paged_w8 (paged): four launches

The qkv constants are formed once, outside both routes.  The two routes' bytes (rq and both caches) are compared for equality, with
two launches of the new route, before any timing.  Then each route is captured as ONE graph of back-to-back calls, one per WEIGHT
set, over as many weight sets as exceed the 256 MB Infinity Cache by a quarter, and ROUNDS rounds alternate the graphs in one process,
timed with HIP events.  Reported: the median microseconds per call of each route, the spread of a route's rounds ((max - min) /
median), new / parent, and the weights' bytes (codes and group constants) over the new route's time as a share of 8 TB/s.

The expectation is fixed beforehand: new / parent < 1 by more than the measured spread in every case -- three launches fewer, the
weight stream unchanged.  `HIT` where new / parent < 1 - the larger of the two routes' spreads, `MISS` otherwise.
`torchlsq.functional.W4A8_ROPE_EPILOGUE_DEFAULT` becomes True only if every case is a HIT.

    python tools/exp_linrope_w4_ab.py [--quick] [--cases A:B] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (H, Hkv, K, G, bits, paged, M); D = 128
CASES = [(H, H // 4, 4096, G, bits, paged, M) for G, bits in ((128, 4), (32, 4), (128, 2)) for H in (32, 64) for paged in (False, True)
         for M in (1, 4, 16)]
D, TMAX, PS = 128, 64, 16
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
    ap.add_argument("--cases", default=":", help="a slice A:B of the case list")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r40_linrope_w4_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq import functional as F
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    lo, hi = (int(v) if v else None for v in args.cases.split(":"))
    cases = [CASES[0], CASES[17], CASES[35]] if args.quick else CASES[lo:hi]
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x, zx = torch.tensor([0.0371], device=dev), torch.tensor([117], dtype=torch.int32, device=dev)
    lines = ["# exp_linrope_w4_ab: the rotary embedding and the KV-cache append in the epilogue of the decode-shape qkv linear on packed "
             "codes (liblsq_hip_linrope_w4.so, one launch) vs the parent's route (lsq_linear_packed_q8_q with decode, lsq_rope_w8_q8_q on q, "
             "the scattered rotation of k and the copy of v or the rotation of k and the paged append: four launches); %s, %d CUs"
             % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` weight sets of `MB` "
             "megabytes in all (1.25 x the 256 MB cache); spread = (max - min) / median of a route's rounds; uint8 levels, mid_dtype "
             "bfloat16, D = 128, R = 128, one token per sequence; the qkv constants hoisted for both routes; the new route's bytes checked "
             "against the parent's on the same buffers before any timing; %%: weight bytes / time over 8 TB/s; HIT: new / parent < 1 - the "
             "larger spread of the two" % rounds,
             "%-38s %5s %4s %5s %5s | %8s %6s %5s | %9s %6s %6s %-4s" % (
                 "N x K x M, bits / G, caches", "calls", "sets", "MB", "grid", "new us", "spread", "%", "parent us", "spread", "new/p", "")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    misses = []
    cos, sin = (t.to(dev) for t in F.lsq_rope_tables(D, TMAX, 10000.0, MID))
    for H, Hkv, K, G, bits, paged, M in cases:
        N = (H + 2 * Hkv) * D
        wbytes = N * (K * bits // 8 + K // G * 8)
        nsets = -(-CACHE_BYTES * 5 // 4 // wbytes)
        iters = max(args.iters, nsets)
        cs = [torch.randint(0, 256, (N, K * bits // 8), device=dev, generator=gen, dtype=torch.uint8) for _ in range(nsets)]
        qs = [(torch.rand(N * (K // G), device=dev, generator=gen) * 0.02 + 0.005) for _ in range(nsets)]
        qz = [torch.randint(0, 2 ** bits, (N * (K // G),), device=dev, generator=gen, dtype=torch.int32) for _ in range(nsets)]
        bias = torch.randn(N, device=dev, generator=gen)
        x = torch.randint(0, 256, (M, 1, K), device=dev, generator=gen, dtype=torch.uint8)
        pos = (torch.arange(M, dtype=torch.int32, device=dev) * 3 + 5) % TMAX
        Mp = TMAX // PS
        table = torch.randperm(M * Mp, device=dev, generator=gen).reshape(M, Mp).to(torch.int32) if paged else None
        shape = (M * Mp, Hkv, PS, D) if paged else (M, Hkv, TMAX, D)
        plan = E.linrope_w4_plan(M, 1, H, Hkv, D, K, G, bits, P=TMAX, **(dict(pages=(M * Mp, PS, Mp)) if paged else dict(Tmax=TMAX)))
        assert plan["served"]
        gq = quantizer(ops.lsq_linear_packed_q8(x.view(M, K), s_x, zx, cs[0], qs[0], qz[0], bias, G, bits, torch.float32))
        s_q, z_q = F._act_constants(*gq, 0, 255)            # hoisted: formed once for both routes
        rot = quantizer(1.3 * (torch.tensor([0.0, 255.0], device=dev) - z_q.float()) * s_q)
        bufs = [[torch.zeros((M, 1, H, D), dtype=torch.uint8, device=dev), torch.zeros(shape, dtype=torch.uint8, device=dev),
                 torch.zeros(shape, dtype=torch.uint8, device=dev)] for _ in range(2)]

        def new(i, b=bufs[0]):
            return E.linrope_w4_q(x, s_x, zx, cs[i], qs[i], qz[i], bias, G, bits, *gq, *RNG, s_q, z_q, cos, sin, *rot, *RNG, MID, H, Hkv,
                                  b[1], b[2], pos, table, out=b[0])

        def parent(i, b=bufs[1]):
            qkv = ops.lsq_linear_packed_q8_q(x, s_x, zx, cs[i], qs[i], qz[i], bias, G, bits, *gq, *RNG, False, MID, True).view(M, 1, H + 2 * Hkv, D)
            q, k, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
            r = (s_q, z_q, cos, sin, *rot, *RNG, MID, pos, False)
            E.rope_w8_q(q, *r, out=b[0])
            if paged:
                E.kv_append_paged_w8(E.rope_w8_q(k, *r), v, b[1], b[2], table, pos)
            else:
                E.rope_w8_q(k, *r, out=b[1].permute(0, 2, 1, 3), scatter=True)
                E.rope_w8_kv_copy(v, b[2].permute(0, 2, 1, 3), pos, True)

        routes = [new, parent]
        with torch.no_grad():
            new(0)
            first = [t.clone() for t in bufs[0]]
            new(0)
            parent(0)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(first, bufs[0])), "two launches differ"
            assert all(torch.equal(a, b) for a, b in zip(bufs[0], bufs[1])), "not the bytes of the parent's route"
            inside = ((first[0] > 0) & (first[0] < 255)).float().mean().item()
            assert len(first[0].unique()) > 32 and 0.25 <= inside and bool(first[1].any()) and bool(first[2].any()), \
                "a vacuous rotation quantizer (%.2f inside)" % inside
            del first
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
        name = "%d x %d x %d, %d / %d, %s" % (N, K, M, bits, G, "paged" if paged else "dense")
        if mark == "MISS":
            misses.append("%s (%.2f)" % (name, tn / tp))
        line = "%-38s %5d %4d %5.0f %5d | %8.2f %6.3f %5.1f | %9.2f %6.3f %6.2f %-4s" % (
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
