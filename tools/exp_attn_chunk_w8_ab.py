#!/usr/bin/env python3
"""A/B: chunked prefill attention on 8-bit levels (liblsq_hip_attn_chunk_w8.so: the split-key decode's three launches with the query
rows of a kv head dealt to row tiles of 16) against what the parent commit does with the same call; uint8 levels, mid_dtype bfloat16,
D = 128, H 32 on Hkv 8.  The protocol is tools/exp_attn_w8_ab.py's, as tools/exp_attn_decode_split_w8_ab.py and
tools/exp_attn_paged_w8_ab.py apply it.

    new       torch.ops.torchlsq.lsq_attention_chunk_w8_q8_q / lsq_attention_chunk_paged_w8_q8_q(..., splits=0), causal with the offset
              Tk - Tq and full key lengths; the workspace's torch.empty is inside the captured graph, as in every call.
    parent    dense: lsq_attention_prefill_w8_q, which beyond 2048 keys COMPOSES (repeat_interleave of k and v, the [B, H, Tq, Tk] score
              tensor through memory twice, a torch.where, p v over all Tk keys).  Pools: lsq_attention_decode_paged_w8_q, which for more
              than 16 rows gathers both pools and composes -- what AttentionCoreW8Q(prefill=True) does today with a block table.  The
              gather is INSIDE the timing.

EXPECTATION, fixed before the run: new / parent < 1.0 beyond the run's spread (new x (1 + the larger spread) < parent) in EVERY case
where the parent composes: a 512-token chunk whose last row sees 4096, 8192 and 32768 keys, at B 1 and B 4, on a dense cache and
through pages of 16 and of 128.  HIT / MISS as it falls.

YARDSTICKS, reported as measured with no expectation attached: whole causal prompts of T 512, 1024 and 2048 (B 1) through the chunk
kernels, the prefill kernel (lsq_attention_prefill_w8_q: "prefill") and the masked three launches (AttentionCoreW8Q(causal=True) on k
and v repeated outside the timing), and a device copy of the bytes the call needs (q, k, v in, y out).

SWEEP of the forced split count, the routes alternating in one run; workgroups per CU, the chunk floor and the split limit all act
through the split count S of a shape (shipped: 4 workgroups per CU on 256 CUs, a chunk floor of 512 keys, at most 64 splits).  Two
kinds of shape: a 512-token chunk at B 1 and B 4 on 8192 and 32768 keys, where the tiles fill the part and the rule gives S = 1
(S = 1, 2, 4, 8, 16 against it); and a 16-token chunk at B 1 on the same keys -- 64 rows per kv head, 32 tile workgroups --, where the
rule splits 32 ways and the three constants act (S = 1, 4, 8, 16, 32, 64, 128: 8 / 16 / 32 / 64 are 1 / 2 / 4 / 8 workgroups per CU,
32, 64 and 128 at 8192 keys lie below the shipped chunk floor of 512, 128 beyond the split limit).  No counter run is made and no cause is claimed.

Before any timing the BYTES of the routes are compared for equality on the first input set, two launches of the new route agree, and
the result is not vacuous.  Then each route is captured as ONE graph of back-to-back calls, one per input set, over as many sets as
exceed the 256 MB Infinity Cache by a quarter (at least two sets and ITERS calls), and ROUNDS rounds alternate the graphs in one
process, timed with HIP events.  Reported: the median microseconds per call of each route and the spread ((max - min) / median).

    python tools/exp_attn_chunk_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

BATCHES = (1, 4)
KEYS = (4096, 8192, 32768)
LAYOUTS = (0, 16, 128)                  # 0: a dense cache; else the page size
PROMPTS = (512, 1024, 2048)
SWEEP = (1, 2, 4, 8, 16)
SWEEP_KEYS = (8192, 32768)
SPLIT_TQ = 16                           # R = 64 rows per kv head: 32 tile workgroups at B 1, where the library's rule splits
SPLIT_SWEEP = (1, 4, 8, 16, 32, 64, 128)
H, HKV, TQ, D = 32, 8, 512, 128
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
    ap.add_argument("--quick", action="store_true", help="fewer rounds, B 1 at 4096 keys, the 512-token prompt, no sweep")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_attn_chunk_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=4)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, lsq_attention_decode_paged_w8_q, lsq_attention_prefill_w8_q
    from torchlsq.quantized import AttentionCoreW8Q
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rounds = 3 if args.quick else args.rounds
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
        torch.cuda.empty_cache()
        return med, spread

    span = 6.0 * QKV_S * QKV_S * 74 * 74 * D ** 0.5          # six sigma of a score of uniform levels
    core = AttentionCoreW8Q(trained(-span, span), trained(0.0, 1.0), trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16, causal=True).to(dev)
    sides = (core.scores._out("output"), core.softmax._out("output"), core.context._out("output"))
    table = core.softmax.table
    s_in, z_in = torch.tensor([QKV_S], device=dev), torch.tensor([QKV_Z], dtype=torch.int32, device=dev)

    def lt(t):
        return LevelsTensor(t, s_in, z_in, 0, 255)

    lines = ["# exp_attn_chunk_w8_ab: chunked prefill attention (liblsq_hip_attn_chunk_w8.so: three launches over row tiles of 16) vs the "
             "parent commit's route for the same call (dense: lsq_attention_prefill_w8_q, which composes beyond 2048 keys; pools: "
             "lsq_attention_decode_paged_w8_q, the gather of both pools inside the timing and that composition); %s, %d CUs"
             % (torch.cuda.get_device_name(0), cus),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over `sets` input sets (q, k, v "
             "or both pools: 1.25 x the 256 MB cache, at least two); spread = (max - min) / median of a route's rounds; uint8 levels, "
             "mid_dtype bfloat16, H %d on Hkv %d, D %d, causal at the offset Tk - Tq, full key lengths; bytes: the routes' results compared "
             "before any timing; plan: tiles / chunk / splits / workgroups of launches 1 and 2 / workspace MB; mark: new x (1 + the larger "
             "spread) < parent -- HIT / MISS (the expectation: every case where the parent composes)" % (rounds, H, HKV, D),
             "%-24s %5s %4s %26s | %9s %6s | %10s %6s %6s %5s | %5s" % (
                 "case", "calls", "sets", "plan", "new us", "spread", "parent us", "spread", "new/p", "mark", "bytes")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save():
        with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    def add(line):
        print(line, flush=True)
        lines.append(line)
        save()

    def operands(B, Tq, Tk, ps):
        """(nsets, iters, the input sets (q, k, v) -- pools where ps --, the block table or None, the lengths)"""
        per_set = B * (H * Tq + 2 * HKV * Tk) * D
        nsets = max(2, -(-CACHE_BYTES * 5 // 4 // per_set))
        iters = max(args.iters, nsets)
        kv = (B * (Tk // ps), HKV, ps, D) if ps else (B, HKV, Tk, D)
        sets = [[torch.randint(0, 256, shape, device=dev, generator=gen, dtype=torch.uint8) for shape in ((B, Tq, H, D), kv, kv)]
                for _ in range(nsets)]
        bt = torch.randperm(B * (Tk // ps), device=dev, generator=gen).to(torch.int32).reshape(B, Tk // ps) if ps else None
        return nsets, iters, sets, bt, torch.full((B,), Tk, device=dev, dtype=torch.int32)

    def plan_text(pl):
        return "%d/%d/%d/%d/%d" % (pl["tiles"], pl["chunk"], pl["splits"], pl["grid"], pl["workspace_bytes"] >> 20)

    # ---- the expectation: a 512-token chunk against a long cache
    misses, ratios = [], []
    cases = [(B, Tk, ps) for ps in LAYOUTS for B in BATCHES for Tk in KEYS]
    if args.quick:
        cases = [(1, 4096, ps) for ps in LAYOUTS]
    for B, Tk, ps in cases:
        name = "b%d tq%d tk%d %s" % (B, TQ, Tk, "ps%d" % ps if ps else "dense")
        nsets, iters, sets, bt, lens = operands(B, TQ, Tk, ps)

        def new(i, splits=0):
            q, k, v = sets[i]
            head = (q.permute(0, 2, 1, 3), s_in, z_in, k, s_in, z_in, v, s_in, z_in)
            tail = (table, *sides[0], *sides[1], *sides[2], BF16, 1, Tk - TQ, lens, splits)
            if ps:
                return torch.ops.torchlsq.lsq_attention_chunk_paged_w8_q8_q(*head, bt, *tail)
            return torch.ops.torchlsq.lsq_attention_chunk_w8_q8_q(*head, *tail)

        def parent(i):
            q, k, v = sets[i]
            if ps:
                return lsq_attention_decode_paged_w8_q(lt(q.permute(0, 2, 1, 3)), lt(k), lt(v), bt, table, *sides, BF16, causal=True,
                                                       key_lengths=lens).levels
            return lsq_attention_prefill_w8_q(lt(q.permute(0, 2, 1, 3)), lt(k), lt(v), table, *sides, BF16, causal=True, key_lengths=lens).levels

        kw = dict(q_strides=(TQ * H * D, D, H * D), causal=1, causal_offset=Tk - TQ)
        pl = E.attn_chunk_paged_w8_plan(B, H, HKV, TQ, D, B * (Tk // ps), ps, Tk // ps, 0, **kw) if ps else \
            E.attn_chunk_w8_plan(B, H, HKV, TQ, Tk, D, 0, **kw)
        assert pl["family"] == "chunk", pl
        if ps:
            assert E.attn_paged_w8_plan(B, H, HKV, TQ, D, B * (Tk // ps), ps, Tk // ps, 0, q_strides=kw["q_strides"], causal=True,
                                        causal_offset=Tk - TQ)["family"] == "composition"
        else:
            assert E.attn_prefill_w8_plan(B, H, HKV, TQ, Tk, D, q_strides=kw["q_strides"], causal=True, causal_offset=Tk - TQ)["family"] == \
                "composition"
        with torch.no_grad():
            y = new(0).clone()
            assert torch.equal(y, new(0)), "%s: two launches differ" % name
            same = torch.equal(y, parent(0))
            assert len(y.unique()) > 16, "%s: a vacuous case" % name
        assert same, "%s: the routes' bytes differ" % name
        (tn, tp), (sn, sp) = timed((new, parent), iters, nsets)
        won = tn * (1 + max(sn, sp)) < tp
        if not won:
            misses.append(name)
        ratios.append((name, tn / tp))
        add("%-24s %5d %4d %26s | %9.1f %6.3f | %10.1f %6.3f %6.2f %5s | %5s" % (name, iters, nsets, plan_text(pl), tn, sn, tp, sp, tn / tp,
                                                                                  "HIT" if won else "MISS", "equal"))
        if not ps and Tk in SWEEP_KEYS and not args.quick:
            with torch.no_grad():
                for s in SWEEP:
                    assert torch.equal(new(0, s), y), "splits %d: the bytes differ" % s
            med, spr = timed([lambda i, s=s: new(i, s) for s in (0,) + SWEEP], iters, nsets)
            best = min(range(len(med)), key=lambda j: med[j])
            for j, s in enumerate((0,) + SWEEP):
                spl = E.attn_chunk_w8_plan(B, H, HKV, TQ, Tk, D, s, **kw)
                add("%-24s %5d %4d %26s | %9.1f %6.3f |" % ("  sweep splits=%d%s" % (s, " (own)" if s == 0 else ""), iters, nsets,
                                                             plan_text(spl), med[j], spr[j]))
            beyond = med[best] * (1 + max(spr[best], spr[0])) < med[0]
            add("#   sweep on %s: the library's choice (S = %d) %.1f us; the fastest forced count S = %d %.1f us: %s"
                % (name, pl["splits"], med[0], ((0,) + SWEEP)[best] or pl["splits"], med[best],
                   "FASTER beyond the spread" if beyond else "not faster beyond the spread"))
        del sets, y
        torch.cuda.empty_cache()
    r = [x[1] for x in ratios]
    add("# new / parent: %.3f .. %.3f over %d cases" % (min(r), max(r), len(r)))
    add("# the expectation (new / parent < 1.0 beyond the run's spread wherever the parent composes): %s"
        % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))

    # ---- the sweep where the rule DOES split: few tiles, so the three constants act
    if not args.quick:
        add("# sweep where the rule splits: a %d-token chunk at B 1 (R = %d rows per kv head: %d tile workgroups), dense; workgroups per CU "
            "1 / 2 / 4 / 8 are S = 8 / 16 / 32 / 64, a chunk floor of F keys forbids S > Tk / F (shipped: 512), the split limit forbids S > 64"
            % (SPLIT_TQ, SPLIT_TQ * H // HKV, HKV * (SPLIT_TQ * H // HKV // 16)))
        for Tk in SWEEP_KEYS:
            name = "b1 tq%d tk%d dense" % (SPLIT_TQ, Tk)
            nsets, iters, sets, _, lens = operands(1, SPLIT_TQ, Tk, 0)

            def few(i, splits=0):
                q, k, v = sets[i]
                return torch.ops.torchlsq.lsq_attention_chunk_w8_q8_q(q.permute(0, 2, 1, 3), s_in, z_in, k, s_in, z_in, v, s_in, z_in, table,
                                                                      *sides[0], *sides[1], *sides[2], BF16, 1, Tk - SPLIT_TQ, lens, splits)

            kw = dict(q_strides=(SPLIT_TQ * H * D, D, H * D), causal=1, causal_offset=Tk - SPLIT_TQ)
            pl = E.attn_chunk_w8_plan(1, H, HKV, SPLIT_TQ, Tk, D, 0, **kw)
            assert pl["family"] == "chunk" and pl["splits"] > 1, pl
            with torch.no_grad():
                y = few(0).clone()
                assert len(y.unique()) > 16, "%s: a vacuous case" % name
                for s_ in SPLIT_SWEEP:
                    assert torch.equal(few(0, s_), y), "splits %d: the bytes differ" % s_
            med, spr = timed([lambda i, s_=s_: few(i, s_) for s_ in (0,) + SPLIT_SWEEP], iters, nsets)
            best = min(range(len(med)), key=lambda j: med[j])
            for j, s_ in enumerate((0,) + SPLIT_SWEEP):
                spl = E.attn_chunk_w8_plan(1, H, HKV, SPLIT_TQ, Tk, D, s_, **kw)
                add("%-24s %5d %4d %26s | %9.1f %6.3f |" % ("  %s splits=%d%s" % (name if s_ == 0 else "  sweep", s_, " (own)" if s_ == 0 else ""),
                                                             iters, nsets, plan_text(spl), med[j], spr[j]))
            beyond = med[best] * (1 + max(spr[best], spr[0])) < med[0]
            add("#   sweep on %s: the library's choice (S = %d) %.1f us; the fastest forced count S = %d %.1f us: %s"
                % (name, pl["splits"], med[0], ((0,) + SPLIT_SWEEP)[best] or pl["splits"], med[best],
                   "FASTER beyond the spread" if beyond else "not faster beyond the spread"))
            del sets, y
            torch.cuda.empty_cache()

    # ---- yardsticks: whole causal prompts, B 1
    add("# yardsticks, as measured: whole causal prompts (B 1, Tq = Tk = T) through the chunk kernels, the prefill kernel, the masked three "
        "launches on k and v repeated outside the timing, and a device copy of the bytes the call needs (q, k, v in, y out)")
    add("%-24s %5s %4s %26s | %9s %6s | %10s %6s | %10s %6s | %9s %6s | %5s" % (
        "case", "calls", "sets", "plan", "chunk us", "spread", "prefill us", "spread", "masked us", "spread", "copy us", "spread", "bytes"))
    masked = AttentionCoreW8Q(trained(-span, span), trained(0.0, 1.0), trained(-1.0, 1.0), alpha=D ** -0.5, mid_dtype=BF16, causal=True).to(dev)
    for T in (PROMPTS[:1] if args.quick else PROMPTS):
        name = "b1 whole prompt T%d" % T
        nsets, iters, sets, _, lens = operands(1, T, T, 0)
        rep = [[x.repeat_interleave(H // HKV, dim=1) for x in s[1:]] for s in sets]
        need = [torch.empty(sum(x.numel() for x in s) + T * H * D, dtype=torch.uint8, device=dev) for s in sets[:2]]

        def new(i):
            q, k, v = sets[i]
            return torch.ops.torchlsq.lsq_attention_chunk_w8_q8_q(q.permute(0, 2, 1, 3), s_in, z_in, k, s_in, z_in, v, s_in, z_in, table, *sides[0],
                                                                  *sides[1], *sides[2], BF16, 1, 0, lens, 0)

        def prefill(i):
            q, k, v = sets[i]
            return lsq_attention_prefill_w8_q(lt(q.permute(0, 2, 1, 3)), lt(k), lt(v), table, *sides, BF16, causal=True, key_lengths=lens).levels

        def three(i):
            return masked(lt(sets[i][0].permute(0, 2, 1, 3)), lt(rep[i][0]), lt(rep[i][1]), key_lengths=lens).levels

        def copy(i):
            return need[1].copy_(need[0])

        pl = E.attn_chunk_w8_plan(1, H, HKV, T, T, D, 0, q_strides=(T * H * D, D, H * D), causal=1, causal_offset=0)
        fam = E.attn_prefill_w8_plan(1, H, HKV, T, T, D, q_strides=(T * H * D, D, H * D), causal=True, causal_offset=0)["family"]
        with torch.no_grad():
            y = new(0)
            same = torch.equal(y, prefill(0)) and torch.equal(y, three(0))
        assert same and len(y.unique()) > 16, "%s: the routes' bytes differ" % name
        med, spr = timed((new, prefill, three, copy), iters, nsets)
        add("%-24s %5d %4d %26s | %9.1f %6.3f | %10.1f %6.3f | %10.1f %6.3f | %9.1f %6.3f | %5s   (prefill plan: %s; chunk / prefill %.2f, "
            "chunk / masked %.2f)" % (name, iters, nsets, plan_text(pl), med[0], spr[0], med[1], spr[1], med[2], spr[2], med[3], spr[3], "equal",
                                      fam, med[0] / med[1], med[0] / med[2]))
        del sets, rep, need, y
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
