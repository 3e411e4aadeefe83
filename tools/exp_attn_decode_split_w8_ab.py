#!/usr/bin/env python3
"""A/B: split-key decode attention on 8-bit levels (liblsq_hip_attn_decode_split_w8.so: one kv head's keys dealt to several workgroups,
three launches and a workspace) against the parent commit's route for the same call; uint8 levels, mid_dtype bfloat16, D = 128, H 32 on
Hkv 8, one query row.  The protocol is tools/exp_attn_w8_ab.py's, as tools/exp_attn_decode_w8_ab.py applies it.

    new       torch.ops.torchlsq.lsq_attention_decode_split_w8_q8_q(..., splits): `splits` = 0, the library's own chunk, in the case
              lines; Tk / chunk in the sweep lines.  The workspace's torch.empty is inside the captured graph, as in every call.
    parent    lsq_attention_decode_w8_q(..., split=None): up to Tk = 8192 the single-launch decode kernel, one workgroup per (b, kv
              head) (its binary is the parent commit's: profiles/r30_attn_decode_split_w8_sha256.txt); above, the composition --
              repeat_interleave of the cache, three launches, the scores and probabilities through memory
    copy      a device-to-device copy of the bytes the definition needs, 2 B Hkv Tk D: no bound, a yardstick

Cases: B 1 / Tk 8192 (DESIGN.md 9.20's MISS: eight workgroups), B 1 / Tk 2048, B 4 and B 8 / Tk 8192, B 32 / Tk 2048 (256 workgroups:
the grid fills the part), B 1 / Tk 16384 and 32768 (beyond the single-launch kernel), full key lengths; and the chunk sweep
{128, 256, 512, 1024, 2048} on the first case and on B 4 / Tk 8192, all six routes alternating in one run each.

Before any timing the BYTES of the two routes are compared for equality on the first input set, two launches of the new route agree, and
the result is not vacuous.  Then each route is captured as ONE graph of back-to-back calls, one per input set, over as many sets (q and
both caches) as exceed the 256 MB Infinity Cache by a quarter (at least two sets and ITERS calls), and ROUNDS rounds alternate the
graphs in one process, timed with HIP events.  Reported: the median microseconds per call of each route, the spread ((max - min) /
median) of each route's rounds, new / parent, the copy's time and the share of 8 TB/s that the needed bytes per new call imply.

Expectation, fixed beforehand and marked per line: new / parent < 1.0 beyond the run's spread (new x (1 + the larger spread) < parent)
in every case where `split="auto"` chooses the split family; the other cases are marked WIN / LOSS by the same rule and say that
"auto" keeps the single launch.  The last lines name the largest measured B Hkv per CU at which the split form still wins beyond the
spread -- the threshold of `split="auto"` -- and the sweep's best chunk.  A miss is reported as a miss; `split=None` stays the default
either way.

    python tools/exp_attn_decode_split_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (name, B, Tk)
CASES = [("b1 tk8192", 1, 8192), ("b1 tk2048", 1, 2048), ("b4 tk8192", 4, 8192), ("b8 tk8192", 8, 8192), ("b32 tk2048", 32, 2048),
         ("b1 tk16384", 1, 16384), ("b1 tk32768", 1, 32768)]
SWEEP = (128, 256, 512, 1024, 2048)
SWEEP_CASES = ("b1 tk8192", "b4 tk8192")        # the first: where the chunk's floor binds; the second: where the workgroups per CU decide
H, HKV, TQ, D = 32, 8, 1, 128
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
    ap.add_argument("--quick", action="store_true", help="fewer rounds, the first two cases and no sweep")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_attn_decode_split_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq._attn_decode_split_w8_host import auto_splits
    from torchlsq.functional import LevelsTensor, lsq_attention_decode_w8_q
    from torchlsq.quantized import AttentionCoreW8Q
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rounds = 3 if args.quick else args.rounds
    cases = CASES[:2] if args.quick else CASES
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
    sides = (core.scores._out("output"), core.softmax._out("output"), core.context._out("output"))
    table = core.softmax.table
    s_in, z_in = torch.tensor([QKV_S], device=dev), torch.tensor([QKV_Z], dtype=torch.int32, device=dev)
    lines = ["# exp_attn_decode_split_w8_ab: split-key decode attention on 8-bit levels (liblsq_hip_attn_decode_split_w8.so, three launches "
             "and a workspace) vs the parent's route (split=None: the single-launch decode kernel up to Tk 8192, the composition above); "
             "%s, %d CUs" % (torch.cuda.get_device_name(0), cus),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` input sets (q and both "
             "caches, 1.25 x the 256 MB cache, at least two); spread = (max - min) / median of a route's rounds; uint8 levels, mid_dtype "
             "bfloat16, H %d on Hkv %d, Tq %d, D %d, full key lengths; bytes: the two routes' results compared before any timing; plan: "
             "chunk / splits / workgroups of launches 1 and 2 / workspace KB; need MB: 2 B Hkv Tk D; copy us: a device-to-device copy of "
             "that many bytes; %%peak: need / new us against 8 TB/s; mark: new x (1 + the larger spread) < parent -- HIT / MISS where "
             "split=\"auto\" takes the split family (the expectation), WIN / LOSS where it keeps the single launch"
             % (rounds, H, HKV, TQ, D),
             "%-16s %5s %4s %6s %22s | %8s %6s | %9s %6s %6s %5s %6s | %5s | %8s %8s %6s %6s" % (
                 "case", "calls", "sets", "p grid", "plan", "new us", "spread", "parent us", "spread", "new/p", "mark", "auto", "bytes",
                 "need MB", "copy us", "new/c", "%peak")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save():
        with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    misses, wins = [], []
    for name, B, Tk in cases:
        per_set = B * (H * TQ + 2 * HKV * Tk) * D
        nsets = max(2, -(-CACHE_BYTES * 5 // 4 // per_set))
        iters = max(args.iters, nsets)
        sets = [[torch.randint(0, 256, shape, device=dev, generator=gen, dtype=torch.uint8)
                 for shape in ((B, TQ, H, D), (B, HKV, Tk, D), (B, HKV, Tk, D))] for _ in range(nsets)]
        lens = torch.full((B,), Tk, device=dev, dtype=torch.int32)
        need = 2 * B * HKV * Tk * D
        src = [torch.empty(need, dtype=torch.uint8, device=dev) for _ in range(max(2, -(-CACHE_BYTES * 5 // 4 // need)))]
        dst = torch.empty(need, dtype=torch.uint8, device=dev)

        def lt(t):
            return LevelsTensor(t, s_in, z_in, 0, 255)

        def new(i, splits=0):
            q, k, v = sets[i]
            return torch.ops.torchlsq.lsq_attention_decode_split_w8_q8_q(q.permute(0, 2, 1, 3), s_in, z_in, k, s_in, z_in, v, s_in, z_in, table,
                                                                         *sides[0], *sides[1], *sides[2], BF16, True, Tk - TQ, lens, splits)

        def parent(i):
            q, k, v = sets[i]
            return lsq_attention_decode_w8_q(lt(q.permute(0, 2, 1, 3)), lt(k), lt(v), table, *sides, BF16, causal=True, key_lengths=lens).levels

        def copy_(i):
            dst.copy_(src[i % len(src)])

        kw = dict(q_strides=(TQ * H * D, D, H * D), causal=True, causal_offset=Tk - TQ)
        pl = E.attn_decode_split_w8_plan(B, H, HKV, TQ, Tk, D, 0, **kw)
        ppl = E.attn_decode_w8_plan(B, H, HKV, TQ, Tk, D, **kw)
        auto = auto_splits(B, H, HKV, TQ, Tk, D, cus, **kw)
        assert pl["family"] == "split" and (ppl["family"] == "decode") == (Tk <= 8192), (pl, ppl)
        with torch.no_grad():
            y = new(0).clone()
            assert torch.equal(y, new(0)), "%s: two launches differ" % name
            same = torch.equal(y, parent(0))
            assert len(y.unique()) > 16, "%s: a vacuous case" % name
        assert same, "%s: the two routes' bytes differ" % name
        (tn, tp, tc), (sn, sp, _) = timed((new, parent, copy_), iters, nsets)
        won = tn * (1 + max(sn, sp)) < tp
        mark = ("HIT" if won else "MISS") if auto else ("WIN" if won else "LOSS")
        if auto and not won:
            misses.append(name)
        if won and ppl["family"] == "decode":
            wins.append(B * HKV / cus)
        line = "%-16s %5d %4d %6s %22s | %8.1f %6.3f | %9.1f %6.3f %6.2f %5s %6s | %5s | %8.1f %8.1f %6.2f %6.1f" % (
            name, iters, nsets, ppl["grid"] if ppl["family"] == "decode" else "comp", "%d/%d/%d/%d" % (
                pl["chunk"], pl["splits"], pl["grid"], pl["workspace_bytes"] // 1024), tn, sn, tp, sp, tn / tp, mark, "split" if auto else "single",
            "equal", need / 1e6, tc, tn / tc, 100 * need / (tn * 1e-6) / PEAK)
        print(line, flush=True)
        lines.append(line)
        save()
        if name in SWEEP_CASES and not args.quick:
            # the chunk sweep: every chunk's bytes against the first result, then the six routes alternating in one run
            with torch.no_grad():
                for chunk in SWEEP:
                    assert torch.equal(new(0, Tk // chunk), y), "chunk %d: the bytes differ" % chunk
            fns = [parent] + [lambda i, s=Tk // chunk: new(i, s) for chunk in SWEEP]
            med, spr = timed(fns, iters, nsets)
            best = min(range(len(SWEEP)), key=lambda j: med[1 + j])
            for j, chunk in enumerate(SWEEP):
                spl = E.attn_decode_split_w8_plan(B, H, HKV, TQ, Tk, D, Tk // chunk, **kw)
                assert spl["chunk"] == chunk
                sweep_line = "%-16s %5d %4d %6s %22s | %8.1f %6.3f | %9.1f %6.3f %6.2f %5s %6s | %5s |" % (
                    "  sweep c%d" % chunk, iters, nsets, ppl["grid"], "%d/%d/%d/%d" % (chunk, spl["splits"], spl["grid"], spl["workspace_bytes"] // 1024),
                    med[1 + j], spr[1 + j], med[0], spr[0], med[1 + j] / med[0], "best" if j == best else "", "", "equal")
                print(sweep_line, flush=True)
                lines.append(sweep_line)
            lines.append("# sweep on %s: the best chunk is %d keys (%d workgroups, %.2f a CU); the library's own choice there is %d"
                         % (name, SWEEP[best], B * HKV * Tk // SWEEP[best], B * HKV * Tk / SWEEP[best] / cus, pl["chunk"]))
            save()
        del sets, src, dst, y
        torch.cuda.empty_cache()
    lines.append("# the largest measured B Hkv per CU (Tk <= 8192) at which the split form wins beyond the spread: %s"
                 % ("%.4f (%d workgroups of the single-launch kernel on %d CUs)" % (max(wins), round(max(wins) * cus), cus) if wins else "none"))
    lines.append("# expectation (new / parent < 1.0 beyond the run's spread wherever split=\"auto\" takes the split family): %s"
                 % ("every such case HIT" if not misses else "MISS: " + "; ".join(misses)))
    save()
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
