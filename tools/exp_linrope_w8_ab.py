#!/usr/bin/env python3
"""A/B: the rotary embedding and the KV-cache append in the epilogue of the decode-shape qkv linear (liblsq_hip_linrope_w8.so:
lsq_linear_w8_q8_dec_rope_q, one launch) against the parent commit's route on the same buffers: uint8 levels everywhere, int8 weight
levels, mid_dtype bfloat16, D = 128 = R, K = 4096, one token per sequence, M = B in {1, 4, 16}, the qkv weight of Llama-3-8B
[6144, 4096] (32 heads on 8 kv heads) and of a 32-head MHA [12288, 4096], into a dense cache [B, Hkv, 256, 128] and into pools of
16-slot pages.

    new      the 16-wave kernel that streams pairs of weight strips, rotates in LDS and stores rq, k and v where they go: one launch
    parent   lsq_linear_w8_q8_dec_q ([M, N] bytes written), lsq_rope_w8 on the q view, then dense: lsq_rope_w8 with scatter on the k
             view into the cache and the COPY of the v view; paged: lsq_rope_w8 of k into a buffer and lsq_kv_append_paged_w8:
             four launches

The two routes' bytes (rq, the k and the v cache) are compared for equality, with two launches of the new route and the non-vacuity
of the rotation's quantizer, before any timing.  Then each route is captured as ONE graph of back-to-back calls, one per WEIGHT set,
over as many weight sets as exceed the 256 MB Infinity Cache by a quarter, and ROUNDS rounds alternate the graphs in one process,
timed with HIP events.  Reported: the median microseconds per call of each route, the spread of a route's rounds ((max - min) /
median), new / parent, and the weight's N K bytes over the new route's time as a share of 8 TB/s.

The expectation is fixed beforehand: new / parent < 1 by more than the measured spread in every case -- three launches fewer and the
qkv bytes not re-read, the weight stream unchanged.  `HIT` where new / parent < 1 - the larger of the two routes' spreads, `MISS`
otherwise.  `torchlsq.functional.W8A8_ROPE_EPILOGUE_DEFAULT` becomes True only if every case is a HIT.  ([6144, 4096] gives 192 items
on 256 compute units where the parent's linear walks 384 tiles: what that underfill costs is read from the table, not guessed.)

    python tools/exp_linrope_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (H, Hkv, M, paged)
CASES = [(32, Hkv, M, paged) for Hkv in (8, 32) for paged in (False, True) for M in (1, 4, 16)]
D, K, TMAX, P, PS = 128, 4096, 256, 512, 16
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
    ap.add_argument("--quick", action="store_true", help="fewer rounds, four cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r37_linrope_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq import functional as F
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [CASES[0], CASES[5], CASES[8], CASES[9]] if args.quick else CASES
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x, zx = torch.tensor([0.0371], device=dev), torch.tensor([117], dtype=torch.int32, device=dev)
    cos, sin = (t.to(dev) for t in F.lsq_rope_tables(D, P, 10000.0, MID))
    lines = ["# exp_linrope_w8_ab: the rotary embedding and the KV-cache append in the epilogue of the decode-shape qkv linear "
             "(liblsq_hip_linrope_w8.so, one launch) vs the parent's route (lsq_linear_w8_q8_dec_q, lsq_rope_w8 on q, then the scattered "
             "lsq_rope_w8 of k and the COPY of v, or lsq_rope_w8 of k and lsq_kv_append_paged_w8: four launches); %s, %d CUs"
             % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` weight sets of `MB` "
             "megabytes in all (1.25 x the 256 MB cache); spread = (max - min) / median of a route's rounds; uint8 levels, int8 weight "
             "levels, D = R = 128, K = 4096, one token per sequence at positions 5 + 3 b, caches of 256 tokens (paged: pages of 16), "
             "mid_dtype bfloat16; the new route's bytes checked against the parent's on the same inputs before any timing; %%: N K bytes "
             "/ time over 8 TB/s; HIT: new / parent < 1 - the larger spread of the two" % rounds,
             "%-30s %5s %4s %5s %5s | %8s %6s %5s | %9s %6s %6s %-4s" % (
                 "N x K x M", "calls", "sets", "MB", "grid", "new us", "spread", "%", "parent us", "spread", "new/p", "")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    misses = []
    for H, Hkv, M, paged in cases:
        N, B = (H + 2 * Hkv) * D, M
        nsets = -(-CACHE_BYTES * 5 // 4 // (N * K))
        iters = max(args.iters, nsets)
        ws = [torch.randint(-128, 128, (N, K), device=dev, generator=gen, dtype=torch.int8) for _ in range(nsets)]
        w_s = torch.rand(N, device=dev, generator=gen) * 0.002 + 0.0005
        w_z = torch.zeros(N, dtype=torch.int32, device=dev)
        bias = torch.randn(N, device=dev, generator=gen)
        x = torch.randint(0, 256, (B, 1, K), device=dev, generator=gen, dtype=torch.uint8)
        pos = (5 + 3 * torch.arange(B, dtype=torch.int32)).to(dev)
        Mp = TMAX // PS
        table = torch.randperm(B * Mp, generator=torch.Generator().manual_seed(1))[:B * Mp].reshape(B, Mp).to(torch.int32).to(dev) if paged else None
        shape = (B * Mp, Hkv, PS, D) if paged else (B, Hkv, TMAX, D)
        pl = E.linrope_w8_plan(B, 1, H, Hkv, D, K, P=P, **(dict(pages=(B * Mp, PS, Mp)) if paged else dict(Tmax=TMAX)))
        assert pl["served"] and pl["grid"] == min(N // 32, torch.cuda.get_device_properties(0).multi_processor_count)
        t = ops.lsq_linear_w8_q8(x.view(B, K), s_x, zx, ws[0], w_s, w_z, bias, torch.float32)
        qq = quantizer(t)
        rq_q = quantizer(t[:, :(H + Hkv) * D])              # a rotation keeps a pair's magnitude: the same range serves its output
        s_q, z_q = F._act_constants(*qq, 0, 255)
        del t
        dests = [[torch.zeros((B, 1, H, D), dtype=torch.uint8, device=dev), torch.zeros(shape, dtype=torch.uint8, device=dev),
                  torch.zeros(shape, dtype=torch.uint8, device=dev)] for _ in range(2)]

        def new(i, d=dests[0]):
            return E.linrope_w8_q(x, s_x, zx, ws[i], w_s, w_z, bias, *qq, *RNG, s_q, z_q, cos, sin, *rq_q, *RNG, MID, H, Hkv, d[1], d[2], pos, table, out=d[0])

        def parent(i, d=dests[1]):
            qkv = ops.lsq_linear_w8_q8_dec_q(x, s_x, zx, ws[i], w_s, w_z, bias, *qq, *RNG, False, MID).view(B, 1, H + 2 * Hkv, D)
            q, k, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
            E.rope_w8_q(q, s_q, z_q, cos, sin, *rq_q, *RNG, MID, pos, False, out=d[0])
            if paged:
                E.kv_append_paged_w8(ops.lsq_rope_w8_q8_q(k, s_q, z_q, cos, sin, *rq_q, *RNG, MID, pos, False), v, d[1], d[2], table, pos)
            else:
                E.rope_w8_q(k, s_q, z_q, cos, sin, *rq_q, *RNG, MID, pos, False, out=d[1].permute(0, 2, 1, 3), scatter=True)
                E.rope_w8_kv_copy(v, d[2].permute(0, 2, 1, 3), pos, True)

        routes = [new, parent]
        with torch.no_grad():
            new(0)
            first = [t.clone() for t in dests[0]]
            for t in dests[0]:
                t.zero_()
            new(0)
            parent(0)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(first, dests[0])), "two launches differ"
            assert all(torch.equal(a, b) for a, b in zip(dests[0], dests[1])), "not the bytes of the parent's route"
            y = dests[0][0]
            inside = ((y > 0) & (y < 255)).float().mean().item()
            assert len(y.unique()) > 32 and 0.25 <= inside and bool((y == 0).any()) and bool((y == 255).any()) and \
                bool(dests[0][1].any()) and bool(dests[0][2].any()), "a vacuous output quantizer (%.2f inside)" % inside
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
        name = "%d x %d x %d %s" % (N, K, M, "paged" if paged else "dense")
        if mark == "MISS":
            misses.append("%s (%.2f)" % (name, tn / tp))
        line = "%-30s %5d %4d %5.0f %5d | %8.2f %6.3f %5.1f | %9.2f %6.3f %6.2f %-4s" % (
            name, iters, nsets, nsets * N * K / 1e6, pl["grid"], tn, spread[0], 100 * N * K / (tn * 1e-6) / PEAK, tp, spread[1], tn / tp, mark)
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                  # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del graphs, ws
        torch.cuda.empty_cache()
    lines.append("# expectation (new / parent < 1 beyond the spread in every case): %s"
                 % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    lines.append("# what bounds the new kernel (the weight stream, the LDS reduction, the 192-item grid or the launch): NOT MEASURED (no "
                 "counter run was made)")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
