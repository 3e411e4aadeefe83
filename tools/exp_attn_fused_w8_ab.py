#!/usr/bin/env python3
"""A/B: the fused attention core on 8-bit levels (liblsq_hip_attn_fused_w8.so: `AttentionCoreW8Q(fused=True)`, one launch, the scores
and probabilities in LDS) against the parent's three-launch `AttentionCoreW8Q` (liblsq_hip_attn_w8.so) on the same inputs, levels as
a QAT model has them: uint8 q, k, v as views of one qkv buffer, int8 scores, uint8 probabilities, int8 context, mid_dtype bfloat16.

    new     AttentionCoreW8Q(fused=True): lsq_attention_w8_q, plan family "fused"
    parent  AttentionCoreW8Q(fused=False): lsq_bmm_w8_q (NT) -> lsq_softmax_w8_q (rows padded to 16) -> lsq_bmm_w8_q (NN)
    copy    a plain device-to-device copy of the core's input bytes (3 B H T D): the yardstick of a bandwidth kernel

Before any timing the BYTES of the two routes are compared for equality on every input set's first use, two launches of the new
route are compared, and the output is held to non-vacuity.  Then each route is captured as ONE graph of back-to-back calls, one per
input set, over as many sets as exceed the 256 MB Infinity Cache by a quarter (at least ITERS calls), and ROUNDS rounds alternate the
graphs in one process, timed with HIP events.  Reported: the median microseconds per call of each route, the spread of the new
route's rounds ((max - min) / median), new / parent, new / copy, the int8 TOP/s of the two matmuls (4 B H T T D / time), and the
fused plan's grid and LDS (with the workgroups a CU's 160 KB of LDS hold).

Expectation from byte counts alone, marked per line (`HIT` / `MISS`): new / parent < 1.0 -- the fused route neither writes nor
re-reads the B H T ceil(T / 16) 16 score and probability bytes and saves two launches.  No other figure is fixed in advance.

    python tools/exp_attn_fused_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

# (name, B, H, T, D)
MODELS = [("vit-b", 32, 12, 197, 64), ("vit-l", 32, 16, 197, 64), ("t1024", 4, 12, 1024, 64), ("t2048", 2, 12, 2048, 64),
          ("t512-d128", 8, 16, 512, 128), ("vit-b batch 1", 1, 12, 197, 64)]
CACHE_BYTES = 256 << 20
CU_LDS = 160 << 10
BF16 = torch.bfloat16
S8, U8R = (-128, 127, -128, 127), (0, 255, 0, 255)


def trained(lo, hi):
    """a per-tensor LSQFakeQuantizer that has seen one batch; its constants are overwritten below"""
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer
    fq = LSQFakeQuantizer(observer=MovingAverageMinMaxObserver, otype="activation").train()
    fq(torch.tensor([lo, hi]))
    fq.disable_observer()
    return fq.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, ViT-B only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_attn_fused_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, _act_constants, lsq_softmax_table
    from torchlsq.quantized import AttentionCoreW8Q
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    models = MODELS[:1] if args.quick else MODELS
    gen = torch.Generator(device=dev).manual_seed(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def t1(v, dtype=torch.float32):
        return torch.tensor([v], dtype=dtype, device=dev)

    s_in, z_in = t1(0.04), t1(128, torch.int32)
    lines = ["# exp_attn_fused_w8_ab: AttentionCoreW8Q(fused=True) (liblsq_hip_attn_fused_w8.so, one launch) vs the parent's three-launch "
             "AttentionCoreW8Q (liblsq_hip_attn_w8.so) on the same inputs and vs a device-to-device copy of the core's input bytes; %s, %d CUs"
             % (torch.cuda.get_device_name(0), cus),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over as many input sets (1.25 x "
             "the 256 MB cache); spread = (max - min) / median of the new route's rounds; uint8 q, k, v views of one qkv buffer, int8 "
             "scores, uint8 probabilities, int8 context, mid_dtype bfloat16; the two routes' bytes are equal on every input set (checked "
             "before the timing); wgs: the fused grid; lds: its bytes per workgroup; /cu: the workgroups a CU's 160 KB hold" % rounds,
             "%-16s %5s | %8s %6s | %9s %6s | %8s %6s | %7s | %6s %7s %3s | %s" % (
                 "case", "calls", "new us", "spread", "parent us", "new/p", "copy us", "new/c", "TOP/s", "wgs", "lds", "/cu", "new/p < 1")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    spreads, misses, ratios = [], [], []
    for model, B, H, T, D in models:
        alpha = D ** -0.5
        in_bytes = 3 * B * H * T * D
        nsets = -(-CACHE_BYTES * 5 // 4 // in_bytes)
        iters = max(args.iters, nsets)
        qkv = [(128 + 32 * torch.randn(B, T, 3, H, D, device=dev, generator=gen)).round().clamp(0, 255).to(torch.uint8) for _ in range(nsets)]

        def heads(i):
            return [LevelsTensor(qkv[i][:, :, j].permute(0, 2, 1, 3), s_in, z_in, *U8R) for j in range(3)]

        # the quantizers, fitted once to the first set: scores symmetric int8 over six sigma, probabilities 1 / 255, context symmetric int8
        q0, k0, v0 = heads(0)
        sf = ops.lsq_bmm_w8_q8(q0.levels, s_in, z_in, k0.levels, s_in, z_in, True, torch.float32)
        sc_s = (6 * sf.std() / 127).reshape(1)
        sc_b = 128 * sc_s
        del sf
        s_s, _ = _act_constants(sc_s, sc_b, -128, 127)
        p_s, p_b = t1(1.0 / 255), t1(0.0)
        pr_s, pr_z = _act_constants(p_s, p_b, 0, 255)
        table = lsq_softmax_table(s_s, alpha)
        s0 = ops.lsq_bmm_w8_q8_q(q0.levels, s_in, z_in, k0.levels, s_in, z_in, True, sc_s, sc_b, *S8, BF16)
        p0 = ops.lsq_softmax_w8_q8_q(s0, table, p_s, p_b, *U8R, BF16, 1)
        cf = ops.lsq_bmm_w8_q8(p0, pr_s, pr_z, v0.levels, s_in, z_in, False, torch.float32)
        c_s = (6 * cf.std() / 127).reshape(1)
        c_b = 128 * c_s
        del cf, s0, p0
        # the module, with those constants in its buffers
        three = AttentionCoreW8Q(trained(-1.0, 1.0), trained(0.0, 1.0), trained(-1.0, 1.0), alpha=alpha, mid_dtype=BF16).to(dev)
        for sub, (sc, sh, rng) in ((three.scores, (sc_s, sc_b, S8)), (three.softmax, (p_s, p_b, U8R)), (three.context, (c_s, c_b, S8))):
            sub.output_scale.copy_(sc)
            sub.output_shift.copy_(sh)
            sub.output_range = rng
        three.softmax.table.copy_(table)
        fused = copy.deepcopy(three)
        fused.fused = True
        pl = E.attn_fused_w8_plan(B, H, T, T, D)
        assert pl["family"] == "fused", pl

        def new(i):
            return fused(*heads(i)).levels

        def parent(i):
            return three(*heads(i)).levels

        pool = torch.randint(0, 256, (nsets, in_bytes), device=dev, generator=gen, dtype=torch.uint8)      # what the copies read
        dst = torch.empty(in_bytes, dtype=torch.uint8, device=dev)

        def copy_(i):
            return dst.copy_(pool[i])

        flops = 4.0 * B * H * T * T * D
        with torch.no_grad():
            for i in range(nsets):
                y = new(i)
                assert y.dtype == torch.int8 and torch.equal(y, parent(i)), "%s: the two routes' bytes differ on set %d" % (model, i)
            y = new(0).clone()
            assert torch.equal(y, new(0)), "two launches differ"
            y16 = y.to(torch.int16)
            inside = ((y16 > y16.min()) & (y16 < y16.max())).float().mean().item()
            assert len(y.unique()) > 32 and inside >= 0.05, "a vacuous output quantizer (%.2f inside)" % inside
            del y, y16
            graphs = []
            for fn_ in (new, parent, copy_):
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
        ratios.append(tn / tp)
        per_cu = CU_LDS // pl["lds_bytes"]
        mark = "HIT" if tn / tp < 1.0 else "MISS"
        if mark == "MISS":
            # the figures a miss can come from: the CUs the grid leaves idle, and the workgroups (of four waves) a CU's LDS holds
            mark += " (%d workgroups for %d CUs; %d KB of LDS a workgroup: %d workgroup%s of 4 waves a CU)" % (
                pl["grid"], cus, pl["lds_bytes"] // 1024, per_cu, "" if per_cu == 1 else "s")
            misses.append(model)
        line = "%-16s %5d | %8.1f %6.3f | %9.1f %6.2f | %8.1f %6.2f | %7.1f | %6d %7d %3d | %s" % (
            model, iters, tn, spread, tp, tn / tp, tc, tn / tc, flops / (tn * 1e-6) / 1e12, pl["grid"], pl["lds_bytes"], per_cu, mark)
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del graphs, dst, qkv, pool, three, fused
        torch.cuda.empty_cache()
    lines.append("# largest spread of the new route's rounds: %.3f" % max(spreads))
    lines.append("# new / parent from %.2f to %.2f" % (min(ratios), max(ratios)))
    lines.append("# expectation (new / parent < 1.0 in every case): %s" % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))


if __name__ == "__main__":
    main()
