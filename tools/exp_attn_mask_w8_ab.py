#!/usr/bin/env python3
"""A/B: the masked softmax on 8-bit levels (liblsq_hip_attn_mask_w8.so: lsq_softmax_mask_w8_q8_q) against the parent commit's only route
for a causal or key-length mask, and against the unmasked lsq_softmax_w8_q8_q on the same shape; uint8 scores and probabilities, rows
padded to 16 bytes, mid_dtype bfloat16.  The protocol is tools/exp_attn_w8_ab.py's.

    new       one launch on the bytes: row r reads and looks up its first n_r keys, and writes all Tk
    parent    LevelsTensor.dequantize(bfloat16) -> masked_fill(-inf) (the boolean mask built once, outside the timing) -> torch.softmax
              -> lsq_levels_per_tensor
    unmasked  lsq_softmax_w8_q8_q on the same scores: the same bytes written, all of them read and looked up

Cases: causal B 4 / H 12 / T 1024, B 2 / H 12 / T 2048 and ViT-B-sized B 32 / H 12 / T 197; key lengths spread over 1..197 on
B 32 / H 12 / T 197; decode B 32 / H 32 / Tq 1 / Tk 2048 with lengths spread over 1..2048.  The whole masked core (q k^T, the masked
softmax, p v; D = 64) against the parent-route core is timed too, with no bound.

Before any timing the BYTES are compared: the new route equals the package's CPU path (the first and the last batch index of the first
input set), two launches agree bit for bit, the new route is held to within ONE level of the float composition on the float32
dequantized scores (`f32`: the share of levels that differ; asserted at once, as tools/exp_attn_w8_ab.py does for the unmasked op), and
the largest difference in levels against the TIMED parent route, whose scores are rounded to bfloat16 first, is taken: the expectation
fixed for it beforehand is at most ONE level too; it is checked at the end of the run, after everything measured is written, and the
run then ends with a non-zero status where it is missed.  Then each route is captured as
ONE graph of back-to-back calls, one per input set, over as many sets as exceed the 256 MB Infinity Cache by a quarter (at least ITERS
calls), and ROUNDS rounds alternate the graphs in one process, timed with HIP events.  Reported: the median microseconds per call of
each route and the spread ((max - min) / median) of the new and the unmasked route's rounds.

Expectations, marked per line: new / parent < 1.0 in every case; for the square causal cases masked <= unmasked * (1 + the larger of
the two routes' spreads in that case).  A miss is reported as a miss.

    python tools/exp_attn_mask_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (name, B, H, Tq, Tk, causal, lengths, square causal)
CASES = [("causal t1024", 4, 12, 1024, 1024, True, False), ("causal t2048", 2, 12, 2048, 2048, True, False),
         ("causal vit-b", 32, 12, 197, 197, True, False), ("lengths vit-b", 32, 12, 197, 197, False, True),
         ("decode tk2048", 32, 32, 1, 2048, False, True)]
D = 64
CACHE_BYTES = 256 << 20
BF16 = torch.bfloat16
S8, U8R = (-128, 127, -128, 127), (0, 255, 0, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, the ViT-B-sized cases only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_attn_mask_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, _act_constants, lsq_softmax_table
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = CASES[2:4] if args.quick else CASES
    gen = torch.Generator(device=dev).manual_seed(0)

    def t1(v, dtype=torch.float32):
        return torch.tensor([v], dtype=dtype, device=dev)

    def lv(y, s, b, rng):
        return ops.lsq_levels_per_tensor(y, s, b, *rng, 0)

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

    s_in, z_in = t1(0.04), t1(128, torch.int32)
    sc_s = t1(0.05)                                  # the scores' quantizer: zero point 128, 1 / sqrt(D) folded into the table
    sc_b = -128 * sc_s
    s_s, s_z = _act_constants(sc_s, sc_b, 0, 255)
    p_s, p_b = t1(1.0 / 255), t1(0.0)
    pr_s, pr_z = _act_constants(p_s, p_b, 0, 255)
    alpha = 1.0
    table = lsq_softmax_table(s_s, alpha)
    table_cpu = table.cpu()
    lines = ["# exp_attn_mask_w8_ab: the masked softmax on 8-bit levels (liblsq_hip_attn_mask_w8.so) vs the parent's only route (dequantize to "
             "bfloat16, masked_fill(-inf), torch.softmax, lsq_levels_per_tensor) and vs the unmasked lsq_softmax_w8_q8_q on the same shape; "
             "%s, %d CUs" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over as many input sets (1.25 x the "
             "256 MB cache); spread = (max - min) / median of a route's rounds; uint8 scores and probabilities (rows 16-byte padded), mid_dtype "
             "bfloat16; cpu: the new route against the package's CPU path, bit for bit; f32: the share of levels that differ from the float "
             "composition on the float32 dequantized scores (never more than one level: asserted); p.diff %% / max: the share and the largest difference in "
             "levels against the timed parent route (expected: at most 1); plan: lanes x packets per row / rows per workgroup; core: q k^T, the "
             "softmax, p v with D = 64, new (three launches) and parent route, no bound" % rounds,
             "%-14s %5s %10s | %8s %6s %5s %7s | %9s %6s %8s %3s %4s | %9s %6s %6s %4s | %9s %9s %6s" % (
                 "case", "calls", "plan", "new us", "spread", "cpu", "f32", "parent us", "new/p", "p.diff %", "max", "<1", "unmask us", "spread", "m/u",
                 "<=", "core us", "p.core us", "c/p")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    misses, far = [], []
    for name, B, H, Tq, Tk, causal, has_len in cases:
        Tp = (Tk + 15) // 16 * 16
        nsets = -(-CACHE_BYTES * 5 // 4 // (B * H * Tq * Tp))
        iters = max(args.iters, nsets)
        scores = [(128 + 32 * torch.randn(B, H, Tq, Tp, device=dev, generator=gen)).round().clamp(0, 255).to(torch.uint8) for _ in range(nsets)]
        off = Tk - Tq
        lens = torch.linspace(1, Tk, B, device=dev).round().to(torch.int32) if has_len else None
        cols = torch.arange(Tk, device=dev).view(1, 1, 1, Tk)
        n = torch.full((B, 1, Tq, 1), Tk, device=dev, dtype=torch.int64)
        if causal:
            n = torch.minimum(n, (torch.arange(Tq, device=dev) + 1 + off).view(1, 1, Tq, 1))
        if has_len:
            n = torch.minimum(n, lens.to(torch.int64).view(B, 1, 1, 1))
        dead = cols >= n                             # [B, 1, Tq, Tk], built once: the parent route's mask

        def new_softmax(i, x=None):
            return ops.lsq_softmax_mask_w8_q8_q(scores[i][..., :Tk] if x is None else x, table, p_s, p_b, *U8R, BF16, causal, off, lens, 16)

        def unmasked(i):
            return ops.lsq_softmax_w8_q8_q(scores[i][..., :Tk], table, p_s, p_b, *U8R, BF16, 16)

        def par_softmax(i, x=None):
            xd = LevelsTensor(scores[i][..., :Tk] if x is None else x, s_s, s_z, *U8R).dequantize(BF16)
            return lv(torch.softmax(xd.masked_fill(dead, float("-inf")), -1), p_s, p_b, U8R).view(torch.uint8)

        with torch.no_grad():
            y = new_softmax(0).clone()
            assert torch.equal(y, new_softmax(0)), "two launches differ"
            for b in sorted({0, B - 1}):
                want = ops.lsq_softmax_mask_w8_q8_q(scores[0][b:b + 1, ..., :Tk].cpu(), table_cpu, p_s.cpu(), p_b.cpu(), *U8R, BF16, causal, off,
                                                    None if lens is None else lens[b:b + 1].cpu(), 1)
                assert torch.equal(y[b:b + 1].cpu(), want), "%s: not the CPU path's bytes (batch %d)" % (name, b)
            assert bool((y[dead.expand_as(y)] == 0).all()) and len(y.unique()) > 32, "a vacuous case"
            xd = LevelsTensor(scores[0][..., :Tk], s_s, s_z, *U8R).dequantize(torch.float32)
            ref = lv(torch.softmax(xd.masked_fill(dead, float("-inf")), -1).to(BF16), p_s, p_b, U8R).view(torch.uint8)
            d = (y.to(torch.int16) - ref.to(torch.int16)).abs()
            assert int(d.max()) <= 1, "%s: more than one level from the float32 composition" % name
            f32 = "%.3f%%" % (100 * (d > 0).float().mean().item())
            del xd, ref
            d = (y.to(torch.int16) - par_softmax(0).to(torch.int16)).abs()
            pdiffer, pmax = 100 * (d > 0).float().mean().item(), int(d.max())
            del y, d
        if pmax > 1:
            far.append("%s (%d levels)" % (name, pmax))
        pl = E.attn_mask_w8_plan_softmax(B * H * Tq, Tk, Tq, Tp, Tp, causal=causal, causal_offset=off, rows_per_length=H * Tq if has_len else None)
        (tn, tp, tu), (sn, _, su) = timed((new_softmax, par_softmax, unmasked), iters, nsets)
        hit_p = "HIT" if tn / tp < 1.0 else "MISS"
        square = causal and Tq == Tk
        hit_u = ("HIT" if tn <= tu * (1 + max(sn, su)) else "MISS") if square else "-"
        for mark, what in ((hit_p, "new/parent"), (hit_u, "masked/unmasked")):
            if mark == "MISS":
                misses.append("%s %s" % (name, what))
        del scores
        torch.cuda.empty_cache()

        # the whole core: q, k, v of D = 64, as many sets as exceed the cache by a quarter
        csets = max(2, min(48, -(-CACHE_BYTES * 5 // 4 // (B * H * (Tq + 2 * Tk) * D))))
        qkv = [[(128 + 32 * torch.randn(B, H, T, D, device=dev, generator=gen)).round().clamp(0, 255).to(torch.uint8) for T in (Tq, Tk, Tk)]
               for _ in range(csets)]
        q0, k0, v0 = qkv[0]
        sf = ops.lsq_bmm_w8_q8(q0, s_in, z_in, k0, s_in, z_in, True, torch.float32)
        k_s = (6 * sf.std() / 127).reshape(1)       # the core's scores quantizer, fitted to the first set: zero point 128
        k_b = -128 * k_s
        del sf
        ks_s, ks_z = _act_constants(k_s, k_b, 0, 255)
        ktable = lsq_softmax_table(ks_s, D ** -0.5)
        ks_alpha = ks_s * D ** -0.5
        tmp = torch.empty(B, H, Tq, Tp, dtype=torch.uint8, device=dev)
        ctx = torch.empty(B, Tq, H * D, dtype=torch.int8, device=dev)
        ctx_view = ctx.view(B, Tq, H, D).permute(0, 2, 1, 3)

        def core_probs(i):
            q, k, _ = qkv[i]
            s = E.attn_w8_bmm_q(q, s_in, z_in, k, s_in, z_in, True, k_s, k_b, *U8R, BF16, out=tmp[..., :Tk])
            return ops.lsq_softmax_mask_w8_q8_q(s, ktable, p_s, p_b, *U8R, BF16, causal, off, lens, 16)

        cf = ops.lsq_bmm_w8_q8(core_probs(0), pr_s, pr_z, v0, s_in, z_in, False, torch.float32)
        c_s = (6 * cf.std() / 127).reshape(1)
        c_b = 128 * c_s
        del cf

        def new_core(i):
            E.attn_w8_bmm_q(core_probs(i), pr_s, pr_z, qkv[i][2], s_in, z_in, False, c_s, c_b, *S8, BF16, out=ctx_view)
            return ctx

        def par_core(i):
            q, k, v = qkv[i]
            qd, kd, vd = (LevelsTensor(t, s_in, z_in, *U8R).dequantize(BF16) for t in (q, k, v))
            s = lv(torch.matmul(qd, kd.transpose(-1, -2)), k_s, k_b, U8R).view(torch.uint8)
            xd = LevelsTensor(s, ks_alpha, ks_z, *U8R).dequantize(BF16)
            p = lv(torch.softmax(xd.masked_fill(dead, float("-inf")), -1), p_s, p_b, U8R).view(torch.uint8)
            pd = LevelsTensor(p, pr_s, pr_z, *U8R).dequantize(BF16)
            return lv(torch.matmul(pd, vd).permute(0, 2, 1, 3).reshape(B, Tq, H * D), c_s, c_b, S8)

        with torch.no_grad():
            yc = new_core(0).clone()
            assert torch.equal(yc, new_core(0)) and len(yc.unique()) > 32, "the core: two launches differ, or a vacuous quantizer"
            del yc
        (tc, tpc), _ = timed((new_core, par_core), max(args.iters, csets), csets)
        line = "%-14s %5d %10s | %8.1f %6.3f %5s %7s | %9.1f %6.2f %8.3f %3d %4s | %9.1f %6.3f %6.2f %4s | %9.1f %9.1f %6.2f" % (
            name, iters, "%dx%d/%d" % (pl["lanes_per_row"], pl["packets_per_lane"], pl["rows_per_workgroup"]), tn, sn, "equal", f32, tp, tn / tp,
            pdiffer, pmax, hit_p, tu, su, tn / tu, hit_u, tc, tpc, tc / tpc)
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del qkv, tmp, ctx
        torch.cuda.empty_cache()
    lines.append("# expectations (new / parent < 1.0 in every case; square causal cases: masked <= unmasked x (1 + spread)): %s"
                 % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    lines.append("# at most one level from the parent route: %s" % ("holds in every case" if not far else "MISSED by " + "; ".join(far)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))
    assert not far, "more than one level from the parent route: " + "; ".join(far)


if __name__ == "__main__":
    main()
