#!/usr/bin/env python3
"""A/B: decode attention on 8-bit levels against a PAGED KV cache (liblsq_hip_attn_paged_w8.so: the split-key decode's three launches
reading the pools through a block table) against the route a paged user had before it, and against the split-key decode on a
contiguous cache of the same geometry; uint8 levels, mid_dtype bfloat16, D = 128, H 32 on Hkv 8, one query row.  The protocol is
tools/exp_attn_w8_ab.py's, as tools/exp_attn_decode_split_w8_ab.py applies it.

    new       torch.ops.torchlsq.lsq_attention_decode_paged_w8_q8_q(..., splits=0): the pools [B Mp, Hkv, ps, D] and a SHUFFLED block
              table (a random permutation of the pages); the workspace's torch.empty is inside the captured graph, as in every call.
    parent    what a paged user does today: lsq_kv_gather_paged_w8 of BOTH pools (torch ops: an index and a dense copy each), then
              lsq_attention_decode_w8_q(..., split="auto").  The gather is INSIDE the timing.
    dense     torch.ops.torchlsq.lsq_attention_decode_split_w8_q8_q(..., splits=0) on contiguous caches [B, Hkv, Tk, D] that hold the
              gathered keys: the same chunk, the same three launches without the indirection.

Cases: B 1 / 4 / 8 / 32 x Tk 2048 / 8192 / 16384 / 32768 x page size 16 / 128, full key lengths; and one chunk sweep, 256 against 512 keys,
on B 1 and B 4 at Tk 8192 with pages of 16, the routes alternating in one run.

Before any timing the BYTES of the three routes are compared for equality on the first input set, two launches of the new route
agree, and the result is not vacuous.  Then each route is captured as ONE graph of back-to-back calls, one per input set, over as many
sets (q and both pools) as exceed the 256 MB Infinity Cache by a quarter (at least two sets and ITERS calls), and ROUNDS rounds
alternate the graphs in one process, timed with HIP events.  Reported: the median microseconds per call of each route, the spread
((max - min) / median) of each route's rounds, new / parent with its mark, and new / dense.

Expectations, fixed before the run:
  1. new / parent < 1.0 beyond the run's spread (new x (1 + the larger spread) < parent) in EVERY case: HIT / MISS as it falls.
  2. new / dense is the price of the indirection.  No bound is fixed; the ratios are reported.
The sweep confirms or replaces the chunk constants inherited from the split library (floor 256): the last line says which.  No counter
run is made and no cause is claimed.

    python tools/exp_attn_paged_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

BATCHES = (1, 4, 8, 32)
KEYS = (2048, 8192, 16384, 32768)
PAGES = (16, 128)
SWEEP = (256, 512)
SWEEP_CASES = ((1, 8192, 16), (4, 8192, 16))
H, HKV, TQ, D = 32, 8, 1, 128
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
    ap.add_argument("--quick", action="store_true", help="fewer rounds, B 1 and 4 at Tk 2048 and 8192, no sweep")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_attn_paged_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, lsq_attention_decode_w8_q, lsq_kv_gather_paged_w8
    from torchlsq.quantized import AttentionCoreW8Q
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rounds = 3 if args.quick else args.rounds
    cases = [(B, Tk, ps) for B in (BATCHES[:2] if args.quick else BATCHES) for Tk in (KEYS[:2] if args.quick else KEYS) for ps in PAGES]
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
        spread = [(max(t[1:]) - min(t[1:])) / m for t, m in zip(times, med)]
        del graphs
        return med, spread

    span = 6.0 * QKV_S * QKV_S * 74 * 74 * D ** 0.5          # six sigma of a score of uniform levels
    core = AttentionCoreW8Q(trained(-span, span), trained(0.0, 1.0), trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16, causal=True).to(dev)
    sides = (core.scores._out("output"), core.softmax._out("output"), core.context._out("output"))
    table = core.softmax.table
    s_in, z_in = torch.tensor([QKV_S], device=dev), torch.tensor([QKV_Z], dtype=torch.int32, device=dev)
    lines = ["# exp_attn_paged_w8_ab: decode attention against a paged KV cache (liblsq_hip_attn_paged_w8.so: three launches reading the pools "
             "through a shuffled block table) vs the parent's route (lsq_kv_gather_paged_w8 of both pools inside the timing, then "
             "lsq_attention_decode_w8_q(split=\"auto\")) and vs the split-key decode on a contiguous cache of the same geometry (dense); "
             "%s, %d CUs" % (torch.cuda.get_device_name(0), cus),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` input sets (q and both "
             "pools, 1.25 x the 256 MB cache, at least two); spread = (max - min) / median of a route's rounds; uint8 levels, mid_dtype "
             "bfloat16, H %d on Hkv %d, Tq %d, D %d, full key lengths; bytes: the three routes' results compared before any timing; plan: "
             "chunk / splits / workgroups of launches 1 and 2 / workspace KB; mark: new x (1 + the larger spread) < parent -- HIT / MISS "
             "(expectation 1: every case); new/d: the price of the indirection (expectation 2: no bound)" % (rounds, H, HKV, TQ, D),
             "%-20s %5s %4s %22s | %8s %6s | %9s %6s %6s %5s | %8s %6s %6s | %5s" % (
                 "case", "calls", "sets", "plan", "new us", "spread", "parent us", "spread", "new/p", "mark", "dense us", "spread", "new/d", "bytes")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save():
        with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    misses, ratios, sweep_notes = [], [], []
    for B, Tk, ps in cases:
        name = "b%d tk%d ps%d" % (B, Tk, ps)
        Mp = Tk // ps
        Np = B * Mp
        per_set = B * (H * TQ + 2 * HKV * Tk) * D
        nsets = max(2, -(-CACHE_BYTES * 5 // 4 // per_set))
        iters = max(args.iters, nsets)
        bt = torch.randperm(Np, device=dev, generator=gen).to(torch.int32).reshape(B, Mp)          # shuffled: no two neighbours in order
        sets = [[torch.randint(0, 256, shape, device=dev, generator=gen, dtype=torch.uint8)
                 for shape in ((B, TQ, H, D), (Np, HKV, ps, D), (Np, HKV, ps, D))] for _ in range(nsets)]
        lens = torch.full((B,), Tk, device=dev, dtype=torch.int32)

        def lt(t):
            return LevelsTensor(t, s_in, z_in, 0, 255)

        dense_sets = [[lsq_kv_gather_paged_w8(lt(p), bt).levels for p in s[1:]] for s in sets]

        def new(i, splits=0):
            q, kp, vp = sets[i]
            return torch.ops.torchlsq.lsq_attention_decode_paged_w8_q8_q(q.permute(0, 2, 1, 3), s_in, z_in, kp, s_in, z_in, vp, s_in, z_in, bt,
                                                                         table, *sides[0], *sides[1], *sides[2], BF16, True, Tk - TQ, lens,
                                                                         splits)

        def parent(i):
            q, kp, vp = sets[i]
            k, v = lsq_kv_gather_paged_w8(lt(kp), bt), lsq_kv_gather_paged_w8(lt(vp), bt)
            return lsq_attention_decode_w8_q(lt(q.permute(0, 2, 1, 3)), k, v, table, *sides, BF16, causal=True, key_lengths=lens,
                                             split="auto").levels

        def dense(i, splits=0):
            q = sets[i][0]
            k, v = dense_sets[i]
            return torch.ops.torchlsq.lsq_attention_decode_split_w8_q8_q(q.permute(0, 2, 1, 3), s_in, z_in, k, s_in, z_in, v, s_in, z_in, table,
                                                                         *sides[0], *sides[1], *sides[2], BF16, True, Tk - TQ, lens, splits)

        pl = E.attn_paged_w8_plan(B, H, HKV, TQ, D, Np, ps, Mp, 0, q_strides=(TQ * H * D, D, H * D), causal=True, causal_offset=Tk - TQ)
        assert pl["family"] == "paged", pl
        with torch.no_grad():
            y = new(0).clone()
            assert torch.equal(y, new(0)), "%s: two launches differ" % name
            same = torch.equal(y, parent(0)) and torch.equal(y, dense(0))
            assert len(y.unique()) > 16, "%s: a vacuous case" % name
        assert same, "%s: the routes' bytes differ" % name
        (tn, tp, td), (sn, sp, sd) = timed((new, parent, dense), iters, nsets)
        won = tn * (1 + max(sn, sp)) < tp
        if not won:
            misses.append(name)
        ratios.append((name, tn / tp, tn / td))
        line = "%-20s %5d %4d %22s | %8.1f %6.3f | %9.1f %6.3f %6.2f %5s | %8.1f %6.3f %6.2f | %5s" % (
            name, iters, nsets, "%d/%d/%d/%d" % (pl["chunk"], pl["splits"], pl["grid"], pl["workspace_bytes"] // 1024), tn, sn, tp, sp, tn / tp,
            "HIT" if won else "MISS", td, sd, tn / td, "equal")
        print(line, flush=True)
        lines.append(line)
        save()
        if (B, Tk, ps) in SWEEP_CASES and not args.quick:
            with torch.no_grad():
                for chunk in SWEEP:
                    assert torch.equal(new(0, Tk // chunk), y), "chunk %d: the bytes differ" % chunk
            fns = [lambda i, s=Tk // chunk: new(i, s) for chunk in SWEEP] + [lambda i, s=Tk // chunk: dense(i, s) for chunk in SWEEP]
            med, spr = timed(fns, iters, nsets)
            for j, chunk in enumerate(SWEEP):
                spl = E.attn_paged_w8_plan(B, H, HKV, TQ, D, Np, ps, Mp, Tk // chunk, q_strides=(TQ * H * D, D, H * D), causal=True,
                                           causal_offset=Tk - TQ)
                assert spl["chunk"] == chunk
                sweep_line = "%-20s %5d %4d %22s | %8.1f %6.3f | %9s %6s %6s %5s | %8.1f %6.3f %6.2f | %5s" % (
                    "  sweep c%d" % chunk, iters, nsets, "%d/%d/%d/%d" % (chunk, spl["splits"], spl["grid"], spl["workspace_bytes"] // 1024),
                    med[j], spr[j], "", "", "", "", med[2 + j], spr[2 + j], med[j] / med[2 + j], "equal")
                print(sweep_line, flush=True)
                lines.append(sweep_line)
            lo, hi = med[0], med[1]
            beyond = hi * (1 + max(spr[0], spr[1])) < lo            # 512 beats 256 beyond the spread
            sweep_notes.append("%s: chunk 256 %.1f us, chunk 512 %.1f us (spreads %.3f, %.3f): %s; the library's own choice there is %d"
                               % (name, lo, hi, spr[0], spr[1], "512 wins beyond the spread" if beyond else "512 does not win beyond the spread",
                                  pl["chunk"]))
            save()
        del sets, dense_sets, y
        torch.cuda.empty_cache()
    np_ = [r[1] for r in ratios]
    nd = [r[2] for r in ratios]
    lines.append("# new / parent: %.2f .. %.2f over %d cases; new / dense (the price of the indirection): %.2f .. %.2f, median %.2f"
                 % (min(np_), max(np_), len(ratios), min(nd), max(nd), statistics.median(nd)))
    for ps in PAGES:
        sel = [r[2] for r in ratios if r[0].endswith("ps%d" % ps)]
        if sel:
            lines.append("#   new / dense at pages of %d: %.2f .. %.2f, median %.2f" % (ps, min(sel), max(sel), statistics.median(sel)))
    lines.append("# expectation 1 (new / parent < 1.0 beyond the run's spread in every case): %s"
                 % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    for note in sweep_notes:
        lines.append("# sweep on " + note)
    if sweep_notes:
        replaced = all("512 wins" in n for n in sweep_notes)
        lines.append("# the chunk floor of 256 inherited from the split library is %s"
                     % ("REPLACED by the sweep: 512 wins beyond the spread in every swept case" if replaced
                        else "CONFIRMED by the sweep: 512 wins beyond the spread in no swept case" if not any("512 wins" in n for n in sweep_notes)
                        else "NOT SETTLED by the sweep: 512 wins beyond the spread in some swept cases only"))
    save()
    print("\n".join(lines[-(5 + len(sweep_notes)):]))


if __name__ == "__main__":
    main()
