#!/usr/bin/env python3
"""A/B: rotary embedding and the KV-cache append on 8-bit levels (liblsq_hip_rope_w8.so) against the parent commit's only route on the
same inputs, and against a device-to-device copy of the input; uint8 in and out, mid_dtype bfloat16.  The protocol is
tools/exp_attn_w8_ab.py's.

    new      one launch on the bytes: lsq_rope_w8_q8_q, or with a cache `rope_w8_q(out=<cache view>, scatter=True)` / lsq_kv_copy_w8
    parent   LevelsTensor.dequantize(bfloat16) -> the gather of the cos / sin rows at positions[b] + t -> the HF-style torch ops
             (x * cos + rotate_half(x) * sin; interleaved: the pairs (2 i, 2 i + 1)) -> lsq_levels_per_tensor; the cache cases add the
             index_put_ into the [B, H, Tmax, D] cache with index tensors built from `positions` in the call.  COPY: that index_put_ alone
    copy     dst.copy_(x): the input's bytes moved once

Cases: prefill B 4 / T 1024 / H 32 / D 128; the same with H 8 (the GQA k); decode B 32 / T 1 / H 32 / D 128 scattered into Tmax 2048;
partial rotary D 64 with R 32; interleaved D 64; COPY of v in the decode case.

Before any timing the BYTES are compared: the new route equals the package's CPU path (the first and the last batch index of the first
input set), two launches agree bit for bit, and the share of bytes that differ from the timed parent route is taken.  Then each
route is captured as ONE graph of back-to-back calls, one per input set, over as many sets as exceed the 256 MB Infinity Cache by a
quarter -- the decode cases 2560 sets of 128 KB, each written at a cache slot of its own in one of two 256 MB caches, so that their
writes walk as much as their reads --, with positions of its own per set, and ROUNDS rounds alternate the graphs in one process,
timed with HIP events.  Reported: the median microseconds per call of each route and the spread ((max - min) / median) of the new
route's rounds.

The one expectation fixed beforehand, marked per line: new / parent < 1.0 in every case.  new / copy is reported with no bound.

    python tools/exp_rope_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (name, B, T, H, D, R, interleaved, Tmax (None: no cache), copy)
CASES = [("prefill h32", 4, 1024, 32, 128, 128, False, None, False), ("prefill h8 gqa", 4, 1024, 8, 128, 128, False, None, False),
         ("decode scatter", 32, 1, 32, 128, 128, False, 2048, False), ("partial d64 r32", 4, 1024, 32, 64, 32, False, None, False),
         ("interleaved d64", 4, 1024, 32, 64, 64, True, None, False), ("decode copy v", 32, 1, 32, 128, 128, False, 2048, True)]
CACHE_BYTES = 256 << 20
BF16 = torch.bfloat16
U8R = (0, 255, 0, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_rope_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, lsq_rope_tables
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    gen = torch.Generator(device=dev).manual_seed(0)

    def t1(v, dtype=torch.float32):
        return torch.tensor([v], dtype=dtype, device=dev)

    def timed(fns, iters, nsets):
        """median us per call and spread of each route: one captured graph per route, rounds alternate"""
        graphs = []
        with torch.no_grad():
            for fn_ in fns:
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
        for _ in range(rounds + 1):                 # the first round warms up
            for j, g in enumerate(graphs):
                t0, t1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                g.replay()
                t1_.record()
                t1_.synchronize()
                times[j].append(t0.elapsed_time(t1_) * 1e3 / iters)
        med = [statistics.median(t[1:]) for t in times]
        return med, [(max(t[1:]) - min(t[1:])) / m for t, m in zip(times, med)]

    s_x, zx = t1(0.025), t1(131, torch.int32)
    o_s, o_b = t1(8.0 / 255), t1(-4.0)
    lines = ["# exp_rope_w8_ab: rotary embedding and the KV-cache append on 8-bit levels (liblsq_hip_rope_w8.so) vs the parent's only route "
             "(dequantize to bfloat16, gather of the cos / sin rows, HF-style torch ops, lsq_levels_per_tensor; cache cases: + index_put_) and vs "
             "a device-to-device copy of the input; %s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over as many input sets (1.25 x the 256 MB "
             "cache; decode: 2560 sets, each at a slot of its own in one of two 256 MB caches); spread = (max - min) / median of the new route's rounds; uint8 in and out, mid_dtype "
             "bfloat16; cpu: the new route against the package's CPU path, bit for bit; p.diff %%: the share of bytes that differ from the timed "
             "parent route; plan: kernel / heads per lane / workgroups" % rounds,
             "%-16s %5s %28s | %8s %6s %5s | %9s %6s %8s %4s | %8s %6s" % ("case", "calls", "plan", "new us", "spread", "cpu", "parent us", "new/p",
                                                                          "p.diff %", "<1", "copy us", "new/c")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    misses = []
    for name, B, T, H, D, R, inter, Tmax, copy in CASES:
        nsets = max(2, -(-CACHE_BYTES * 5 // 4 // (B * T * H * D)))         # decode: 2560 sets of 128 KB
        iters = nsets
        xs = [torch.randint(0, 256, (B, T, H, D), device=dev, generator=gen, dtype=torch.uint8) for _ in range(nsets)]
        P = Tmax if Tmax else T + 64
        cos, sin = lsq_rope_tables(R, P, mid_dtype=BF16, device=dev)
        cosf, sinf = (torch.cat((t, t), -1) if not inter else t for t in (cos.to(BF16), sin.to(BF16)))      # what an HF module caches
        if Tmax:        # set i writes cache i % 2 at a slot of its own per batch: the writes walk 1.25 x the 256 MB cache as the reads do
            assert nsets <= 2 * Tmax
            poss = ((torch.arange(nsets, device=dev).view(nsets, 1) // 2 * 797 + torch.randint(0, Tmax, (1, B), device=dev, generator=gen)) % Tmax).to(torch.int32)
        else:
            poss = torch.randint(0, 64, (nsets, B), device=dev, generator=gen).to(torch.int32)
        ar_t = torch.arange(T, device=dev)
        caches = [torch.zeros((B, H, Tmax, D), dtype=torch.uint8, device=dev) for _ in range(2)] if Tmax else None
        pcaches = [torch.zeros((B, H, Tmax, D), dtype=torch.uint8, device=dev) for _ in range(2)] if Tmax else None
        dst = torch.empty((B, T, H, D), dtype=torch.uint8, device=dev)
        ar_b, ar_h = torch.arange(B, device=dev).view(B, 1, 1), torch.arange(H, device=dev).view(1, 1, H)

        def put(cache, y, i):          # the parent's cache write: index tensors built from the device positions in the call
            p = (poss[i].long().view(B, 1) + ar_t.view(1, T)).view(B, T, 1)
            cache.index_put_((ar_b, ar_h, p), y)
            return cache

        def new(i):
            x = xs[i]
            if copy:
                ops.lsq_kv_copy_w8(x, caches[i % 2].permute(0, 2, 1, 3), poss[i], True)
                return caches[i % 2]
            if Tmax:
                E.rope_w8_q(x, s_x, zx, cos, sin, o_s, o_b, *U8R, BF16, poss[i], inter, out=caches[i % 2].permute(0, 2, 1, 3), scatter=True)
                return caches[i % 2]
            return ops.lsq_rope_w8_q8_q(x, s_x, zx, cos, sin, o_s, o_b, *U8R, BF16, poss[i], inter)

        def parent(i):
            if copy:
                return put(pcaches[i % 2], xs[i], i)
            d = LevelsTensor(xs[i], s_x, zx, *U8R).dequantize(BF16)
            p = poss[i].long().view(B, 1) + ar_t.view(1, T)
            c, s = cosf[p].unsqueeze(2), sinf[p].unsqueeze(2)
            rot = d[..., :R]
            if inter:
                x1, x2 = rot[..., 0::2], rot[..., 1::2]
                y = torch.stack((x1 * c - x2 * s, x2 * c + x1 * s), -1).flatten(-2)
            else:
                y = rot * c + torch.cat((-rot[..., R // 2:], rot[..., :R // 2]), -1) * s
            if R < D:
                y = torch.cat((y, d[..., R:]), -1)
            lv = ops.lsq_levels_per_tensor(y, o_s, o_b, *U8R, 0).view(torch.uint8)
            return put(pcaches[i % 2], lv, i) if Tmax else lv

        def d2d(i):
            return dst.copy_(xs[i])

        with torch.no_grad():
            y = new(0).clone()
            assert torch.equal(y, new(0)), "two launches differ"
            yp = parent(0).clone()
            pdiff = 100 * (y != yp).float().mean().item()
            for b in sorted({0, B - 1}):
                xb, pb = xs[0][b:b + 1].cpu(), poss[0][b:b + 1].cpu()
                if Tmax:
                    want = torch.zeros((1, H, Tmax, D), dtype=torch.uint8)
                    if copy:
                        ops.lsq_kv_copy_w8(xb, want.permute(0, 2, 1, 3), pb, True)
                    else:
                        E.rope_w8_q(xb, s_x.cpu(), zx.cpu(), cos.cpu(), sin.cpu(), o_s.cpu(), o_b.cpu(), *U8R, BF16, pb, inter,
                                    out=want.permute(0, 2, 1, 3), scatter=True)
                else:
                    want = ops.lsq_rope_w8_q8_q(xb, s_x.cpu(), zx.cpu(), cos.cpu(), sin.cpu(), o_s.cpu(), o_b.cpu(), *U8R, BF16, pb, inter)
                assert torch.equal(y[b:b + 1].cpu(), want), "%s: not the CPU path's bytes (batch %d)" % (name, b)
            assert len(y.unique()) > 32, "a vacuous case"
            del y, yp
        if copy:
            pl = E.rope_w8_plan(B, T, H, D, Tout=Tmax, y_strides=(H * Tmax * D, D, Tmax * D), scatter=True, copy=True)
        else:
            pl = E.rope_w8_plan(B, T, H, D, R, P, Tmax or T, y_strides=(H * Tmax * D, D, Tmax * D) if Tmax else None, interleaved=inter,
                                scatter=bool(Tmax))
        (tn, tp, tc), (sn, _, _) = timed((new, parent, d2d), iters, nsets)
        hit = "HIT" if tn / tp < 1.0 else "MISS"
        if hit == "MISS":
            misses.append(name)
        line = "%-16s %5d %28s | %8.1f %6.3f %5s | %9.1f %6.3f %8.3f %4s | %8.1f %6.2f" % (
            name, iters, "%s/%d/%d" % (pl["kernel"], pl["heads_per_lane"], pl["grid"]), tn, sn, "equal", tp, tn / tp, pdiff, hit, tc, tn / tc)
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del xs, caches, pcaches, dst
        torch.cuda.empty_cache()
    lines.append("# expectation (new / parent < 1.0 in every case): %s" % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])


if __name__ == "__main__":
    main()
