#!/usr/bin/env python3
"""A/B: N single lsq_per_group calls against one fused lsq_foreach_per_group call, on whole models' weight sets.

Sets (the [out, numel / out] view of every weight, as LSQFakeQuantizer(group_size=G) quantizes it):
  vit_b_f32 / vit_b_bf16   ViT-B/16's 48 linear weights (12 x qkv 2304x768, proj 768x768, fc1 3072x768, fc2 768x3072), G = 128
  resnet18_f32             ResNet-18's 16 3x3 convolutions as [out, in * 9] and its 1000x512 classifier, G = 64
  tinyllama_bf16           a TinyLlama-1.1B-like stack: 22 layers x q/o 2048x2048, k/v 256x2048, gate/up 5632x2048,
                           down 2048x5632, G = 128
  llama7b_layer_bf16       one Llama-7B layer: q/k/v/o 4096x4096, gate/up 11008x4096, down 4096x11008, G = 128 (large
                           weights: the no-regression check)

One step = the autograd forward of every weight + backward with a fixed upstream gradient (parameter gradients reset to
None between steps, so no accumulation kernels run).  The two routes alternate in one process: ROUNDS rounds of STEPS
steps each; reported is the median wall time per step (host included, synchronised at the end of a round) and the
spread (max - min over rounds).  Before timing, both routes' outputs and gradients are compared bit for bit.

Kernel time: a separate run under rocprofv3 per set, then --kernel-stats reads the traces back:
    rocprofv3 --kernel-trace --stats -d DIR/SET -o k -- python tools/exp_group_foreach_ab.py --quick --only SET
    python tools/exp_group_foreach_ab.py --kernel-stats DIR [--out FILE]
It sums the group kernels' durations per route (single: fwd_grp_kernel / bwd_grp_kernel; fused: *_grp_multi_kernel) and
divides by the steps the --quick run made per route; the roofline share counts per element forward 8 + 8/G and backward
12 + 16/G bytes for fp32 (16-bit storage: half the element bytes) against 8 TB/s.
"""
import argparse
import glob
import os
import sqlite3
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

ROOFLINE = 8.0e12
WARMUP = 3
QUICK_ROUNDS, QUICK_STEPS = 2, 5


def weight_sets():
    vit = []
    for _ in range(12):
        vit += [(2304, 768), (768, 768), (3072, 768), (768, 3072)]
    r18 = [(64, 64 * 9)] * 4 + [(128, 64 * 9)] + [(128, 128 * 9)] * 3 + [(256, 128 * 9)] + [(256, 256 * 9)] * 3 + \
          [(512, 256 * 9)] + [(512, 512 * 9)] * 3 + [(1000, 512)]
    tl = []
    for _ in range(22):
        tl += [(2048, 2048), (256, 2048), (256, 2048), (2048, 2048), (5632, 2048), (5632, 2048), (2048, 5632)]
    l7 = [(4096, 4096)] * 4 + [(11008, 4096), (11008, 4096), (4096, 11008)]
    return {"vit_b_f32": (vit, 128, torch.float32), "vit_b_bf16": (vit, 128, torch.bfloat16),
            "resnet18_f32": (r18, 64, torch.float32), "tinyllama_bf16": (tl, 128, torch.bfloat16),
            "llama7b_layer_bf16": (l7, 128, torch.bfloat16)}


def algorithmic_bytes(shapes, G, dtype):
    eb = torch.tensor([], dtype=dtype).element_size()
    n = sum(a * b for a, b in shapes)
    return n * (2 * eb + 8.0 / G), n * (3 * eb + 16.0 / G)


def make(shapes, G, dtype, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    ws, ss, bs, gs = [], [], [], []
    for o, k in shapes:
        ws.append((torch.randn((o, k), generator=gen, device=dev) * 0.02).to(dtype))
        ss.append((torch.rand((o, k // G), generator=gen, device=dev) * 0.004 + 0.001).requires_grad_(True))
        bs.append(torch.zeros((o, k // G), device=dev, requires_grad=True))
        gs.append(torch.randn((o, k), generator=gen, device=dev).to(dtype))
    return ws, ss, bs, gs


def step(route, ws, ss, bs, gs, G):
    from torchlsq.functional import lsq_foreach_per_group, lsq_per_group
    for t in ss + bs:
        t.grad = None
    if route == "fused":
        ys = lsq_foreach_per_group(ws, ss, bs, G, -8, 7, -128, 127, is_affine=False)
    else:
        ys = [lsq_per_group(w, s, b, G, -8, 7, -128, 127, is_affine=False) for w, s, b in zip(ws, ss, bs)]
    torch.autograd.backward(ys, gs)
    return ys


def run_sets(names, rounds, steps, say):
    dev = torch.device("cuda:0")
    sets = weight_sets()
    say("%-20s %5s %4s | %10s %8s | %10s %8s | %6s" % ("set", "n_w", "G", "single us", "spread", "fused us", "spread",
                                                       "f/s"))
    for name in names:
        shapes, G, dtype = sets[name]
        ws, ss, bs, gs = make(shapes, G, dtype, dev)
        for w in ws:
            w.requires_grad_(True)
        got = {}
        for route in ("single", "fused"):
            for w in ws:
                w.grad = None
            ys = step(route, ws, ss, bs, gs, G)
            got[route] = [y.detach().clone() for y in ys] + [t.grad.clone() for t in ws + ss + bs]
            del ys
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got["single"], got["fused"])), name + ": routes disagree"
        del got
        for w in ws:
            w.grad = None
            w.requires_grad_(False)         # the weights' own gradients are a GEMM's business, not the quantizer's
        for route in ("single", "fused"):
            for _ in range(WARMUP):
                step(route, ws, ss, bs, gs, G)
        torch.cuda.synchronize()
        times = {"single": [], "fused": []}
        for _ in range(rounds):
            for route in ("single", "fused"):
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(route, ws, ss, bs, gs, G)
                torch.cuda.synchronize()
                times[route].append((time.perf_counter() - t0) * 1e6 / steps)
        ts, tf = statistics.median(times["single"]), statistics.median(times["fused"])
        say("%-20s %5d %4d | %10.1f %8.1f | %10.1f %8.1f | %6.2f" %
            (name, len(shapes), G, ts, max(times["single"]) - min(times["single"]), tf,
             max(times["fused"]) - min(times["fused"]), tf / ts))
        del ws, ss, bs, gs
        torch.cuda.empty_cache()


def kernel_stats(root, say):
    sets = weight_sets()
    steps = WARMUP + 1 + QUICK_ROUNDS * QUICK_STEPS        # per route: the check step, warm-up, the timed rounds
    say("# kernel time per step from rocprofv3 --kernel-trace (one run per set, %d steps per route)" % steps)
    say("%-20s | %10s %6s %5s | %10s %6s %5s | %6s | %s" % ("set", "single us", "launch", "roof", "fused us", "launch",
                                                           "roof", "f/s", "fused kernels: us per step"))
    for name in sets:
        dbs = sorted(glob.glob(os.path.join(root, name, "**", "*.db"), recursive=True))
        if not dbs:
            continue
        shapes, G, dtype = sets[name]
        fb, bb = algorithmic_bytes(shapes, G, dtype)
        cur = sqlite3.connect(dbs[-1]).cursor()
        rows = list(cur.execute("select s.display_name, count(*), sum(d.end - d.start) from rocpd_kernel_dispatch d join "
                                "rocpd_info_kernel_symbol s on d.kernel_id = s.id group by s.display_name"))
        acc = {"single": [0.0, 0], "fused": [0.0, 0]}
        parts = []
        for kname, calls, ns in rows:
            route = "fused" if "grp_multi_kernel" in kname else ("single" if "_grp_kernel" in kname else None)
            if route:
                acc[route][0] += ns / 1e3 / steps
                acc[route][1] += calls / steps
                if route == "fused":
                    parts.append("%s %.1f" % ("fwd" if "fwd_" in kname else "bwd", ns / 1e3 / steps))
        us = {r: acc[r][0] for r in acc}
        say("%-20s | %10.1f %6.0f %5.2f | %10.1f %6.0f %5.2f | %6.2f | %s" %
            (name, us["single"], acc["single"][1], (fb + bb) / (us["single"] * 1e-6) / ROOFLINE, us["fused"], acc["fused"][1],
             (fb + bb) / (us["fused"] * 1e-6) / ROOFLINE, us["fused"] / us["single"], ", ".join(parts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="few rounds (the rocprofv3 runs)")
    ap.add_argument("--only", default=None, help="one set")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="summarise the rocprofv3 runs under DIR/<set>/")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.kernel_stats:
        kernel_stats(a.kernel_stats, say)
    else:
        import torchlsq  # noqa: F401
        props = torch.cuda.get_device_properties(0)
        rounds, steps = (QUICK_ROUNDS, QUICK_STEPS) if a.quick else (a.rounds, a.steps)
        say("# exp_group_foreach_ab: %s, %d CUs; wall us per autograd forward + backward step of every weight, median of %d "
            "alternating rounds x %d steps" % (props.name, props.multi_processor_count, rounds, steps))
        run_sets([a.only] if a.only else list(weight_sets()), rounds, steps, say)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
