#!/usr/bin/env python3
"""A/B: the attention core on 8-bit levels (liblsq_hip_attn_w8.so: lsq_bmm_w8_q8_q, lsq_softmax_w8_q8_q) against the route of the
parent commit on the same inputs, levels as a QAT model has them (uint8 q, k, v as views of one qkv buffer, int8 scores, uint8
probabilities, int8 context), mid_dtype bfloat16: the scores q k^T (NT), the softmax and the context p v (NN), and the whole core, at
ViT-B (B 32, H 12, T 197, D 64), ViT-L (H 16) and one long case (B 4, H 12, T 1024, D 64).

    new     one launch per op on the bytes (the core: three), operands read in place, rows of T bytes padded to 16
    parent  LevelsTensor.dequantize(bfloat16) -> torch.matmul / torch.softmax -> lsq_levels_per_tensor, 1 / sqrt(D) folded into the
            scale the scores are dequantized with
    copy    a plain device-to-device copy of the op's input bytes: the yardstick of a bandwidth kernel

Before any timing the BYTES of the routes are compared.  The matmuls' new route is held bit for bit to the definition computed with
exact float64 sums of the integer products (they fit 53 bits) and the same float32 steps; the softmax's to the float composition on
the float32 dequantized values within ONE level; against the timed parent route (bfloat16 arithmetic: another definition) the share
of levels that differ and the largest difference are reported, not bounded.  Two launches of the new route are compared bit for bit,
and every output quantizer is held to non-vacuity.  Then each route is captured as ONE graph of back-to-back calls, one per input
set, over as many sets as exceed the 256 MB Infinity Cache by a quarter (at least ITERS calls), and ROUNDS rounds alternate the graphs
in one process, timed with HIP events.  Reported: the median microseconds per call of each route, the spread of the new route's
rounds ((max - min) / median), new / parent, new / copy, the int8 TOP/s of the matmuls (2 B H M N K / time).

Expectation from byte counts, marked per line (`HIT` / `MISS`): new / parent < 1.0 in every case.  No bound is fixed on new / copy or
on the TOP/s.

    python tools/exp_attn_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (name, B, H, T, D)
MODELS = [("vit-b", 32, 12, 197, 64), ("vit-l", 32, 16, 197, 64), ("t1024", 4, 12, 1024, 64)]
CACHE_BYTES = 256 << 20
BF16 = torch.bfloat16
S8, U8R = (-128, 127, -128, 127), (0, 255, 0, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, ViT-B only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_attn_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, _act_constants, lsq_softmax_table
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    models = MODELS[:1] if args.quick else MODELS
    gen = torch.Generator(device=dev).manual_seed(0)

    def t1(v, dtype=torch.float32):
        return torch.tensor([v], dtype=dtype, device=dev)

    s_in, z_in = t1(0.04), t1(128, torch.int32)
    lines = ["# exp_attn_w8_ab: batched matmul and softmax on 8-bit levels (liblsq_hip_attn_w8.so) vs the parent's route (dequantize to "
             "bfloat16, torch.matmul / torch.softmax, lsq_levels_per_tensor) and vs a device-to-device copy of the op's input bytes; %s, %d CUs"
             % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over as many input sets (1.25 x "
             "the 256 MB cache); spread = (max - min) / median of the new route's rounds; uint8 q, k, v views of one qkv buffer, int8 "
             "scores, uint8 probabilities (rows 16-byte padded), int8 context, mid_dtype bfloat16; def: the new route against its "
             "definition (matmuls: exact sums, bit for bit; softmax: the float32 composition, share of levels that differ, never more than "
             "one); p.diff %% / max: the share and the largest difference in levels against the timed parent route (bfloat16 arithmetic)"
             % rounds,
             "%-16s %5s | %8s %6s %7s | %9s %6s %8s %3s | %8s %6s | %7s | %s" % (
                 "case", "calls", "new us", "spread", "def", "parent us", "new/p", "p.diff %", "max", "copy us", "new/c", "TOP/s", "new/p < 1")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    spreads, misses = [], []
    for model, B, H, T, D in models:
        Tp = (T + 15) // 16 * 16
        alpha = D ** -0.5
        nsets = -(-CACHE_BYTES * 5 // 4 // (2 * B * H * T * D))
        iters = max(args.iters, nsets)
        qkv = [(128 + 32 * torch.randn(B, T, 3, H, D, device=dev, generator=gen)).round().clamp(0, 255).to(torch.uint8) for _ in range(nsets)]

        def heads(i):
            return [qkv[i][:, :, j].permute(0, 2, 1, 3) for j in range(3)]

        # the quantizers, fitted once to the first set: scores symmetric int8 over six sigma, probabilities 1 / 255, context symmetric int8
        q0, k0, v0 = heads(0)
        sf = ops.lsq_bmm_w8_q8(q0, s_in, z_in, k0, s_in, z_in, True, torch.float32)
        sc_s = (6 * sf.std() / 127).reshape(1)
        sc_b = 128 * sc_s
        del sf
        s_s, s_z = _act_constants(sc_s, sc_b, -128, 127)
        p_s, p_b = t1(1.0 / 255), t1(0.0)
        pr_s, pr_z = _act_constants(p_s, p_b, 0, 255)
        table = lsq_softmax_table(s_s, alpha)
        s_s_alpha = s_s * alpha

        def new_scores(i, out=None):
            q, k, _ = heads(i)
            y = scores[i] if out is None else out
            return E.attn_w8_bmm_q(q, s_in, z_in, k, s_in, z_in, True, sc_s, sc_b, *S8, BF16, out=y[..., :T])

        def new_softmax(i, x=None):
            return ops.lsq_softmax_w8_q8_q(scores[i][..., :T] if x is None else x, table, p_s, p_b, *U8R, BF16, 16)

        scores = [torch.empty(B, H, T, Tp, dtype=torch.int8, device=dev) for _ in range(nsets)]
        for i in range(nsets):
            new_scores(i)
        probs = [new_softmax(i) for i in range(nsets)]
        cf = ops.lsq_bmm_w8_q8(probs[0], pr_s, pr_z, heads(0)[2], s_in, z_in, False, torch.float32)
        c_s = (6 * cf.std() / 127).reshape(1)
        c_b = 128 * c_s
        del cf
        ctx = torch.empty(B, T, H * D, dtype=torch.int8, device=dev)
        ctx_view = ctx.view(B, T, H, D).permute(0, 2, 1, 3)
        tmp_scores = torch.empty(B, H, T, Tp, dtype=torch.int8, device=dev)

        def new_context(i, p=None):
            E.attn_w8_bmm_q(probs[i] if p is None else p, pr_s, pr_z, heads(i)[2], s_in, z_in, False, c_s, c_b, *S8, BF16, out=ctx_view)
            return ctx

        def new_core(i):
            return new_context(i, new_softmax(i, new_scores(i, tmp_scores)))

        def lv(y, s, b, rng):
            return ops.lsq_levels_per_tensor(y, s, b, *rng, 0)

        def par_scores(i):
            q, k, _ = heads(i)
            qd, kd = (LevelsTensor(t, s_in, z_in, *U8R).dequantize(BF16) for t in (q, k))
            return lv(torch.matmul(qd, kd.transpose(-1, -2)), sc_s, sc_b, S8)

        def par_softmax(i, x=None):
            xd = LevelsTensor(scores[i][..., :T] if x is None else x, s_s_alpha, s_z, *S8).dequantize(BF16)
            return lv(torch.softmax(xd, -1), p_s, p_b, U8R).view(torch.uint8)

        def par_context(i, p=None):
            pd = LevelsTensor(probs[i] if p is None else p, pr_s, pr_z, *U8R).dequantize(BF16)
            vd = LevelsTensor(heads(i)[2], s_in, z_in, *U8R).dequantize(BF16)
            return lv(torch.matmul(pd, vd).permute(0, 2, 1, 3).reshape(B, T, H * D), c_s, c_b, S8)

        def par_core(i):
            return par_context(i, par_softmax(i, par_scores(i)))

        def exact_bmm(a, sa, za, b, sb, zb, nt, s, sh):
            """the definition: exact sums in float64, the float32 steps, one rounding to bfloat16, the levels op"""
            da, db = a.double() - za.double(), b.double() - zb.double()
            I = torch.matmul(da, db.transpose(-1, -2) if nt else db)
            return lv(((sb * I.float()) * sa).to(BF16), s, sh, S8)

        def def_scores():
            q, k, _ = heads(0)
            ok = torch.equal(new_scores(0), exact_bmm(q, s_in, z_in, k, s_in, z_in, True, sc_s, sc_b))
            assert ok, "scores: not the definition's bytes"
            return "exact"

        def def_softmax():
            xd = LevelsTensor(scores[0][..., :T], s_s_alpha, s_z, *S8).dequantize(torch.float32)
            ref = lv(torch.softmax(xd, -1).to(BF16), p_s, p_b, U8R).view(torch.uint8)
            d = (new_softmax(0).to(torch.int16) - ref.to(torch.int16)).abs()
            assert int(d.max()) <= 1, "softmax: more than one level from the float composition"
            return "%.3f%%" % (100 * (d > 0).float().mean().item())

        def def_context():
            got = new_context(0)
            want = exact_bmm(probs[0], pr_s, pr_z, heads(0)[2], s_in, z_in, False, c_s, c_b).permute(0, 2, 1, 3).reshape(B, T, H * D)
            assert torch.equal(got, want), "context: not the definition's bytes"
            return "exact"

        pool = torch.randint(0, 256, (nsets, B * H * T * (T + D)), device=dev, generator=gen, dtype=torch.uint8)    # what the copies read
        mm_ops = 2.0 * B * H * T * T * D
        # (case, new, parent, definition check, the op's input bytes, matmul operations)
        cases = [("scores", new_scores, par_scores, def_scores, 2 * B * H * T * D, mm_ops),
                 ("softmax", new_softmax, par_softmax, def_softmax, B * H * T * T, 0.0),
                 ("context", new_context, par_context, def_context, B * H * T * (T + D), mm_ops),
                 ("core", new_core, par_core, lambda: "-", 3 * B * H * T * D, 2 * mm_ops)]
        for case, new, parent, check, in_bytes, flops in cases:
            name = "%s %s" % (model, case)
            dst = torch.empty(in_bytes, dtype=torch.uint8, device=dev)

            def copy(i, dst=dst, n=in_bytes):
                return dst.copy_(pool[i, :n])

            with torch.no_grad():
                y = new(0).clone()
                assert torch.equal(y, new(0)), "two launches differ"
                how = check()
                yl = y[..., :T] if case == "softmax" else y
                inside = ((yl.to(torch.int16) > yl.to(torch.int16).min()) & (yl.to(torch.int16) < yl.to(torch.int16).max())).float().mean().item()
                assert len(yl.unique()) > 32 and inside >= 0.05, "a vacuous output quantizer (%.2f inside)" % inside
                pl = parent(0)
                d = (yl.reshape(pl.shape).to(torch.int16) - pl.to(torch.int16)).abs()
                pdiffer, pmax = 100 * (d > 0).float().mean().item(), int(d.max())
                del y, yl, pl, d
                graphs = []
                for fn_ in (new, parent, copy):
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
            tn, tp, tc = (statistics.median(t[1:]) for t in times)
            spread = (max(times[0][1:]) - min(times[0][1:])) / tn
            spreads.append(spread)
            mark = "HIT" if tn / tp < 1.0 else "MISS"
            if mark == "MISS":
                misses.append(name)
            line = "%-16s %5d | %8.1f %6.3f %7s | %9.1f %6.2f %8.3f %3d | %8.1f %6.2f | %7s | %s" % (
                name, iters, tn, spread, how, tp, tn / tp, pdiffer, pmax, tc, tn / tc, "%.1f" % (flops / (tn * 1e-6) / 1e12) if flops else "-", mark)
            print(line, flush=True)
            lines.append(line)
            with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
                f.write("\n".join(lines) + "\n")
            del graphs, dst
        del qkv, scores, probs, pool, ctx, tmp_scores
        torch.cuda.empty_cache()
    lines.append("# largest spread of the new route's rounds: %.3f" % max(spreads))
    lines.append("# expectation (new / parent < 1.0 in every case): %s" % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
