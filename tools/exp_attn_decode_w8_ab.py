#!/usr/bin/env python3
"""A/B: decode attention on 8-bit levels against a grouped-query KV cache (liblsq_hip_attn_decode_w8.so: `AttentionCoreW8Q(decode=True)`)
against the parent commit's only way to do the same thing; uint8 levels, mid_dtype bfloat16, D = 128.  The protocol is
tools/exp_attn_w8_ab.py's.

    new       AttentionCoreW8Q(causal=True, decode=True)(q, k, v, key_lengths): one launch, one workgroup per (b, kv head), the G
              query heads of a kv head share its k and v reads, every key loop ends at the batch's key count
    parent    AttentionCoreW8Q(causal=True)(q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), key_lengths): the expansion
              (where G > 1) is inside the timing, because a user has to write it per step; then q k^T over all Tk slots, the masked
              softmax, p v over all Tk slots -- three launches, the scores and probabilities through memory
    copy      a device-to-device copy of the bytes the definition needs, sum_b 2 Hkv n_b D: no bound, a yardstick

Cases: B 32 / H 32 / Hkv 32 / Tq 1 / Tk 2048 with lengths spread over 1..2048 (profiles/r26_attn_mask_w8_ab.txt's decode case); the
same with Hkv 8; B 8 / H 32 / Hkv 8 / Tk 8192 with full lengths; B 32 / H 32 / Hkv 8 / Tq 4 / Tk 2048 (16 rows per workgroup); and
B 1 / H 32 / Hkv 8 / Tk 8192, whose grid is eight workgroups: expected to be weak, reported as it is.

Before any timing the BYTES of the two routes are compared for equality on the first input set (the probabilities quantizer has shift
0, so they are equal by the definition), two launches of the new route agree, and the result is not vacuous.  Then each route is
captured as ONE graph of back-to-back calls, one per input set, over as many sets (q and both caches) as exceed the 256 MB Infinity
Cache by a quarter (at least two sets and ITERS calls), and ROUNDS rounds alternate the graphs in one process, timed with HIP events.
Reported: the median microseconds per call of each route, the spread ((max - min) / median) of each route's rounds, new / parent, the
copy's time and the share of 8 TB/s that the needed bytes per new call imply.

Expectation, fixed beforehand and marked per line: new / parent < 1.0 in every case, beyond the run's spread (new x (1 + the larger
spread) < parent).  A miss is reported as a miss; `decode=False` stays the default either way.

    python tools/exp_attn_decode_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (name, B, H, Hkv, Tq, Tk, lengths: "spread" over 1..Tk or "full")
CASES = [("mha tk2048", 32, 32, 32, 1, 2048, "spread"), ("gqa4 tk2048", 32, 32, 8, 1, 2048, "spread"), ("gqa4 tk8192", 8, 32, 8, 1, 8192, "full"),
         ("gqa4 tq4 tk2048", 32, 32, 8, 4, 2048, "spread"), ("gqa4 b1 tk8192", 1, 32, 8, 1, 8192, "full")]
D = 128
CACHE_BYTES = 256 << 20
PEAK = 8e12
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_attn_decode_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor
    from torchlsq.quantized import AttentionCoreW8Q
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [CASES[4], CASES[2]] if args.quick else CASES
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

    span = 6.0 * QKV_S * QKV_S * 74 * 74 * D ** 0.5          # six sigma of a score of uniform levels
    core = AttentionCoreW8Q(trained(-span, span), trained(0.0, 1.0), trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16, causal=True).to(dev)
    dec = copy.deepcopy(core)
    dec.decode = True
    s_in, z_in = torch.tensor([QKV_S], device=dev), torch.tensor([QKV_Z], dtype=torch.int32, device=dev)
    lines = ["# exp_attn_decode_w8_ab: decode attention on 8-bit levels against a grouped-query KV cache (liblsq_hip_attn_decode_w8.so, "
             "AttentionCoreW8Q(decode=True)) vs the parent's only route (AttentionCoreW8Q(causal=True) with key_lengths on repeat_interleave'd "
             "k and v, the expansion inside the timing); %s, %d CUs" % (torch.cuda.get_device_name(0),
                                                                          torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` input sets (q and both "
             "caches, 1.25 x the 256 MB cache, at least two); spread = (max - min) / median of a route's rounds; uint8 levels, mid_dtype "
             "bfloat16, D = %d; bytes: the two routes' results compared before any timing; plan: threads / rows / LDS bytes of a workgroup; "
             "need MB: sum_b 2 Hkv n_b D, the bytes of k and v the definition needs; copy us: a device-to-device copy of that many bytes; "
             "%%peak: need / new us against 8 TB/s; expectation: new x (1 + the larger spread) < parent" % (rounds, D),
             "%-16s %5s %4s %5s %16s | %8s %6s | %9s %6s %6s %5s | %5s | %8s %8s %6s %6s" % (
                 "case", "calls", "sets", "grid", "plan", "new us", "spread", "parent us", "spread", "new/p", "<1", "bytes", "need MB", "copy us",
                 "new/c", "%peak")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    misses = []
    for name, B, H, Hkv, Tq, Tk, how in cases:
        G = H // Hkv
        per_set = B * (H * Tq + 2 * Hkv * Tk) * D
        nsets = max(2, -(-CACHE_BYTES * 5 // 4 // per_set))
        iters = max(args.iters, nsets)
        sets = [[torch.randint(0, 256, shape, device=dev, generator=gen, dtype=torch.uint8)
                 for shape in ((B, Tq, H, D), (B, Hkv, Tk, D), (B, Hkv, Tk, D))] for _ in range(nsets)]
        lens = (torch.linspace(1, Tk, B, device=dev).round() if how == "spread" else torch.full((B,), Tk, device=dev)).to(torch.int32)
        need = int(2 * Hkv * D * lens.to(torch.int64).clamp(0, Tk).sum().item())          # read once, outside every timing
        src = [torch.empty(need, dtype=torch.uint8, device=dev) for _ in range(max(2, -(-CACHE_BYTES * 5 // 4 // need)))]
        dst = torch.empty(need, dtype=torch.uint8, device=dev)

        def lt(t):
            return LevelsTensor(t, s_in, z_in, 0, 255)

        def new(i):
            q, k, v = sets[i]
            return dec(lt(q.permute(0, 2, 1, 3)), lt(k), lt(v), key_lengths=lens).levels

        def parent(i):
            q, k, v = sets[i]
            if G > 1:
                k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
            return core(lt(q.permute(0, 2, 1, 3)), lt(k), lt(v), key_lengths=lens).levels

        def copy_(i):
            dst.copy_(src[i % len(src)])

        pl = E.attn_decode_w8_plan(B, H, Hkv, Tq, Tk, D, q_strides=(Tq * H * D, D, H * D), causal=True, causal_offset=Tk - Tq)
        assert pl["family"] == "decode", pl
        with torch.no_grad():
            y = new(0).clone()
            assert torch.equal(y, new(0)), "%s: two launches differ" % name
            same = torch.equal(y, parent(0))
            assert len(y.unique()) > 16, "%s: a vacuous case" % name
            del y
        assert same, "%s: the two routes' bytes differ" % name
        (tn, tp, tc), (sn, sp, _) = timed((new, parent, copy_), iters, nsets)
        hit = "HIT" if tn * (1 + max(sn, sp)) < tp else "MISS"
        if hit == "MISS":
            misses.append(name)
        line = "%-16s %5d %4d %5d %16s | %8.1f %6.3f | %9.1f %6.3f %6.2f %5s | %5s | %8.1f %8.1f %6.2f %6.1f" % (
            name, iters, nsets, pl["grid"], "%d/%d/%d" % (pl["threads"], pl["rows"], pl["lds_bytes"]), tn, sn, tp, sp, tn / tp, hit, "equal",
            need / 1e6, tc, tn / tc, 100 * need / (tn * 1e-6) / PEAK)
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del sets, src, dst
        torch.cuda.empty_cache()
    lines.append("# expectation (new / parent < 1.0 in every case, beyond the run's spread): %s"
                 % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])


if __name__ == "__main__":
    main()
