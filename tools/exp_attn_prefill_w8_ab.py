#!/usr/bin/env python3
"""A/B: prefill attention on 8-bit levels (liblsq_hip_attn_prefill_w8.so: `AttentionCoreW8Q(prefill=True)`) against the parent commit's
only way to do the same thing; uint8 levels, mid_dtype bfloat16.  The protocol is tools/exp_attn_w8_ab.py's.

    new       AttentionCoreW8Q(causal=0 or False, prefill=True)(q, k, v, key_lengths): one launch, a workgroup per (b, h, 64 rows),
              the scores and probabilities in LDS, every wave's key loops ended at its rows' largest key count, k and v of
              [B, Hkv, T, D] read in place
    parent    AttentionCoreW8Q(causal=...)(q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), key_lengths): the expansion
              (where G > 1) is inside the timing, because a user has to write it per call; then q k^T over all T x T, the masked
              softmax, p v over all T keys -- three launches, the scores and probabilities through memory
    fused     where Hkv == H and the fused kernel serves the shape: AttentionCoreW8Q(fused=True) WITHOUT a mask on the same q, k, v
              (liblsq_hip_attn_fused_w8.so) -- other bytes and all T x T of the work: the unmasked one-launch kernel as a yardstick

Cases, causal square at D 128: B 4 / H 32 / Hkv 8 / T 512; the same at T 1024; B 2 / H 32 / Hkv 8 / T 2048; B 4 / H 32 / Hkv 32 /
T 1024 (G = 1: the mask's gain without the grouped-query gain); and ViT-sized B 32 / H 12 / T 197 / D 64 with key_lengths only
(spread over 1..197), not causal.

Before any timing the BYTES of new and parent are compared for equality on the first input set (the probabilities quantizer has
shift 0, so they are equal by the definition), two launches of the new route agree, and the result is not vacuous.  Then each route
is captured as ONE graph of back-to-back calls, one per input set, over as many sets (q, k and v) as exceed the 256 MB Infinity
Cache by a quarter (at least two sets and ITERS calls), and ROUNDS rounds alternate the graphs in one process, timed with HIP events.
Reported: the median microseconds per call of each route, the spread ((max - min) / median) of each route's rounds, new / parent and
new / fused.

Expectation, fixed beforehand and marked per line: new / parent < 1.0 in every case, beyond the run's spread (new x (1 + the larger
spread) < parent).  A miss is reported as a miss; `prefill=False` stays the default either way.

    python tools/exp_attn_prefill_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (name, B, H, Hkv, T, D, causal, lengths: None or "spread" over 1..T)
CASES = [("gqa4 t512", 4, 32, 8, 512, 128, True, None), ("gqa4 t1024", 4, 32, 8, 1024, 128, True, None),
         ("gqa4 t2048", 2, 32, 8, 2048, 128, True, None), ("mha t1024", 4, 32, 32, 1024, 128, True, None),
         ("vit t197 lengths", 32, 12, 12, 197, 64, False, "spread")]
CACHE_BYTES = 256 << 20
BF16 = torch.bfloat16
QKV_S, QKV_Z = 0.03, 125


def trained(lo, hi):
    """a per-tensor quint8 LSQFakeQuantizer that has seen one batch, its scale and shift set to cover lo..hi, observer off, eval"""
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    q = LSQFakeQuantizer(observer=MovingAverageMinMaxObserver, otype="activation").train()
    q(torch.tensor([float(lo), float(hi)]))
    with torch.no_grad():
        q.scale.fill_((hi - lo) / (q.quant_max - q.quant_min))
        q.shift.fill_(lo)
    q.disable_observer()
    return q.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, the two smallest cases only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_attn_prefill_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import AttentionCoreW8Q
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [CASES[4], CASES[0]] if args.quick else CASES
    gen = torch.Generator(device=dev).manual_seed(0)

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

    s_in, z_in = torch.tensor([QKV_S], device=dev), torch.tensor([QKV_Z], dtype=torch.int32, device=dev)
    lines = ["# exp_attn_prefill_w8_ab: prefill attention on 8-bit levels (liblsq_hip_attn_prefill_w8.so, AttentionCoreW8Q(prefill=True)) vs "
             "the parent's only route (AttentionCoreW8Q(causal=...) with key_lengths on repeat_interleave'd k and v, the expansion inside "
             "the timing) and, where Hkv == H, vs the UNMASKED fused kernel (AttentionCoreW8Q(fused=True), all T x T); %s, %d CUs"
             % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` input sets (q, k "
             "and v, 1.25 x the 256 MB cache, at least two); spread = (max - min) / median of a route's rounds; uint8 levels, mid_dtype "
             "bfloat16; bytes: new and parent compared before any timing; plan: threads / rows / LDS bytes of a workgroup; "
             "expectation: new x (1 + the larger spread) < parent" % rounds,
             "%-17s %5s %4s %5s %16s | %8s %6s | %9s %6s %6s %5s | %5s | %8s %6s" % (
                 "case", "calls", "sets", "grid", "plan", "new us", "spread", "parent us", "spread", "new/p", "<1", "bytes", "fused us", "new/f")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    misses = []
    for name, B, H, Hkv, T, D, causal, how in cases:
        G = H // Hkv
        span = 6.0 * QKV_S * QKV_S * 74 * 74 * D ** 0.5          # six sigma of a score of uniform levels
        core = AttentionCoreW8Q(trained(-span, span), trained(0.0, 1.0), trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16,
                                causal=causal).to(dev)
        pre, fus = copy.deepcopy(core), copy.deepcopy(core)
        pre.prefill, fus.fused, fus.causal = True, True, False
        per_set = B * (H + 2 * Hkv) * T * D
        nsets = max(2, -(-CACHE_BYTES * 5 // 4 // per_set))
        iters = max(args.iters, nsets)
        sets = [[torch.randint(0, 256, shape, device=dev, generator=gen, dtype=torch.uint8)
                 for shape in ((B, T, H, D), (B, Hkv, T, D), (B, Hkv, T, D))] for _ in range(nsets)]
        lens = None if how is None else torch.linspace(1, T, B, device=dev).round().to(torch.int32)

        def lt(t):
            return LevelsTensor(t, s_in, z_in, 0, 255)

        def new(i):
            q, k, v = sets[i]
            return pre(lt(q.permute(0, 2, 1, 3)), lt(k), lt(v), key_lengths=lens).levels

        def parent(i):
            q, k, v = sets[i]
            if G > 1:
                k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
            return core(lt(q.permute(0, 2, 1, 3)), lt(k), lt(v), key_lengths=lens).levels

        def fused(i):
            q, k, v = sets[i]
            return fus(lt(q.permute(0, 2, 1, 3)), lt(k), lt(v)).levels

        pl = E.attn_prefill_w8_plan(B, H, Hkv, T, T, D, q_strides=(T * H * D, D, H * D), causal=bool(causal), causal_offset=0,
                                    has_lengths=lens is not None)
        assert pl["family"] == "prefill", pl
        with_fused = G == 1 and E.attn_fused_w8_plan(B, H, T, T, D, q_strides=(T * H * D, D, H * D))["family"] == "fused"
        with torch.no_grad():
            y = new(0).clone()
            assert torch.equal(y, new(0)), "%s: two launches differ" % name
            same = torch.equal(y, parent(0))
            assert len(y.unique()) > 16, "%s: a vacuous case" % name
            del y
        assert same, "%s: the two routes' bytes differ" % name
        med, spread = timed((new, parent) + ((fused,) if with_fused else ()), iters, nsets)
        tn, tp, sn, sp = med[0], med[1], spread[0], spread[1]
        hit = "HIT" if tn * (1 + max(sn, sp)) < tp else "MISS"
        if hit == "MISS":
            misses.append(name)
        line = "%-17s %5d %4d %5d %16s | %8.1f %6.3f | %9.1f %6.3f %6.2f %5s | %5s | %8s %6s" % (
            name, iters, nsets, pl["grid"], "%d/%d/%d" % (pl["threads"], pl["rows"], pl["lds_bytes"]), tn, sn, tp, sp, tn / tp, hit, "equal",
            "%.1f" % med[2] if with_fused else "-", "%.2f" % (tn / med[2]) if with_fused else "-")
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del sets
        torch.cuda.empty_cache()
    lines.append("# expectation (new / parent < 1.0 in every case, beyond the run's spread): %s"
                 % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])


if __name__ == "__main__":
    main()
