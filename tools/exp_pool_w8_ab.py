#!/usr/bin/env python3
"""A/B: pooling on 8-bit levels (liblsq_hip_pool_w8.so: lsq_max_pool2d_q8, lsq_avg_pool2d_q8_q) against the route of the parent
commit on the same inputs, at batch 32 (the global pools at batch 256 too): the ResNet stem's 3 x 3 stride-2 max pool on 64@112^2
and on 64@56^2, the global average pool on 512@7^2 and 2048@7^2, a 2 x 2 average pool on 256@56^2.

    new     one launch on the bytes: one byte read per activation, the output's bytes written
    parent  LevelsTensor.dequantize(bfloat16) in channels-last memory -> F.max_pool2d / F.avg_pool2d -> lsq_levels_per_tensor with
            the input's quantizer (max) or the output quantizer (average): the activation as floats twice and more launches
    copy    a plain device-to-device copy (hipMemcpyAsync) of the input's bytes: the yardstick of a bandwidth kernel
    pixN    (max pool only, when tools/_tune/liblsq_hip_pool_w8_pixN.so exists: --build-variants compiles them) the max kernel
            with N adjacent output pixels per lane, which keeps column maxima in registers across them (-DLSQ_POOL_W8_MAX_PIX=N)

Before any timing the max pool's bytes are compared with the parent route's (its definition re-expressed) and the average pool's
levels with the CPU path of the op (its definition; the parent route sums rounded floats and is a different function), and two
launches are compared bit for bit.  Then each route is captured as ONE graph of back-to-back calls, one per input set, over as
many sets as exceed the 256 MB Infinity Cache by a quarter (at least ITERS calls), and ROUNDS rounds alternate the graphs in one
process, timed with HIP events.  Reported: the median microseconds per call of each route, the spread of the new route's rounds
((max - min) / median), new / parent, and the algorithmic bytes (input + output) over the time as a share of 8 TB/s for the new
route and (twice the input) for the copy.

Expectation from byte counts, marked per line (`HIT` / `MISS`): new / parent < 1.0 in every case.

    python tools/exp_pool_w8_ab.py [--quick] [--out FILE] [--build-variants]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

# (name, kind, batch, C, H = W, kernel, stride, padding)
CASES = [("max 3/2/1 64@112", "max", 32, 64, 112, 3, 2, 1), ("max 3/2/1 64@56", "max", 32, 64, 56, 3, 2, 1),
         ("gap 512@7", "avg", 32, 512, 7, 7, 7, 0), ("gap 2048@7", "avg", 32, 2048, 7, 7, 7, 0),
         ("gap 512@7 B256", "avg", 256, 512, 7, 7, 7, 0), ("gap 2048@7 B256", "avg", 256, 2048, 7, 7, 7, 0),
         ("avg 2/2/0 256@56", "avg", 32, 256, 56, 2, 2, 0)]
CACHE_BYTES = 256 << 20
PEAK = 8e12
RNG = (0, 255, 0, 255)
CL = torch.channels_last
TUNE = os.path.join(ROOT, "tools", "_tune")
VARIANTS = (2, 4)


def build_variants():
    """the max kernel with 2 and 4 output pixels per lane, with the Makefile's flags, into tools/_tune/"""
    os.makedirs(TUNE, exist_ok=True)
    src = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "csrc", "pool_w8", "lsq_pool_w8.hip")
    for n in VARIANTS:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                               "-fhip-fp32-correctly-rounded-divide-sqrt", "-DLSQ_POOL_W8_MAX_PIX=%d" % n, "-shared", src, "-o",
                               os.path.join(TUNE, "liblsq_hip_pool_w8_pix%d.so" % n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, three cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_pool_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--build-variants", action="store_true", help="compile the pixN variants of the max kernel and exit")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [CASES[1], CASES[2], CASES[6]] if args.quick else CASES
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x = torch.tensor([1 / 32], device=dev)
    zx = torch.tensor([128], dtype=torch.int32, device=dev)
    x_shift = -zx.float() * s_x
    alts = {}
    for n in VARIANTS:
        path = os.path.join(TUNE, "liblsq_hip_pool_w8_pix%d.so" % n)
        if os.path.isfile(path):
            lib = ctypes.CDLL(path)
            lib.lsq_pool_w8_max.restype = ctypes.c_int
            lib.lsq_pool_w8_max.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(E.LsqPoolW8Geom), ctypes.c_void_p, ctypes.c_void_p]
            alts[n] = lib
    lines = ["# exp_pool_w8_ab: pooling on 8-bit levels (liblsq_hip_pool_w8.so) vs the parent's route (dequantize to bfloat16, "
             "F.max_pool2d / F.avg_pool2d, lsq_levels_per_tensor) and vs a device-to-device copy of the input; %s, %d CUs" % (
                 torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over as many input sets "
             "(1.25 x the 256 MB cache); spread = (max - min) / median of the new route's rounds; uint8 levels in and out, mid_dtype "
             "bfloat16; the max pool's bytes checked against the parent's route and the average pool's levels against the CPU path "
             "before any timing; %%: (input + output bytes) / time over 8 TB/s (copy: twice the input)" % rounds,
             "%-18s %5s %-14s %5s | %8s %6s %5s | %9s %6s | %8s %5s | %s | %s" % (
                 "case", "calls", "family", "lanes", "new us", "spread", "%", "parent us", "new/p", "copy us", "%", "new/p < 1", "pixN us")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    spreads, misses = [], []
    for name, kind, B, C, HW, k, st, pd in cases:
        x_bytes = B * C * HW * HW
        nsets = -(-CACHE_BYTES * 5 // 4 // x_bytes)
        iters = max(args.iters, nsets)
        lx = [(128 + 32 * torch.randn((B, C, HW, HW), device=dev, generator=gen)).round().clamp(0, 255).to(torch.uint8)
              .contiguous(memory_format=CL) for _ in range(nsets)]
        geo = ([k, k], [st, st], [pd, pd])
        dst = torch.empty_like(lx[0])
        if kind == "max":
            plan = E.pool_w8_plan_max(B, C, HW, HW, k, st, pd)
            lanes = plan["pixels_per_lane"]

            def new(i):
                return ops.lsq_max_pool2d_q8(lx[i], *geo, [1, 1], False)

            def parent(i):
                y = F.max_pool2d(LevelsTensor(lx[i], s_x, zx, *RNG).dequantize(torch.bfloat16), k, st, pd)
                return ops.lsq_levels_per_tensor(y, s_x, x_shift, *RNG, 0).view(torch.uint8)
        else:
            plan = E.pool_w8_plan_avg(B, C, HW, HW, k, st, pd)
            lanes = plan["lanes_per_window"]
            v = ops.lsq_avg_pool2d_q8(lx[0], s_x, zx, *geo, False, True, None, torch.float32)
            sd = 1.4826 * (v - v.median()).abs().median()
            osc = (sd / 64).reshape(1)
            osh = -128 * osc

            def new(i):
                return ops.lsq_avg_pool2d_q8_q(lx[i], s_x, zx, *geo, False, True, None, osc, osh, *RNG, torch.bfloat16)

            def parent(i):
                y = F.avg_pool2d(LevelsTensor(lx[i], s_x, zx, *RNG).dequantize(torch.bfloat16), k, st, pd)
                return ops.lsq_levels_per_tensor(y, osc, osh, *RNG, 0).view(torch.uint8)
        assert plan["family"] != "generic"

        def copy(i):
            return dst.copy_(lx[i])

        routes = [new, parent, copy]
        with torch.no_grad():
            y = new(0)
            y_bytes = y.numel()
            assert torch.equal(y, new(0)), "two launches differ"
            if kind == "max":
                assert torch.equal(y, parent(0)), "not the bytes of the parent's route"
            else:
                want = ops.lsq_avg_pool2d_q8_q(lx[0].cpu(), s_x.cpu(), zx.cpu(), *geo, False, True, None, osc.cpu(), osh.cpu(), *RNG, torch.bfloat16)
                assert torch.equal(y.cpu(), want), "not the levels of the CPU path"
                inside = ((y > 0) & (y < 255)).float().mean().item()
                assert 0.25 <= inside and bool((y == 0).any()) and bool((y == 255).any()), "a vacuous output quantizer (%.2f inside)" % inside
            for n, lib in alts.items() if kind == "max" else ():
                geom = E.LsqPoolW8Geom(B, C, HW, HW, k, k, st, st, pd, pd, 1, 1, 0)
                out = torch.empty_like(y)

                def alt(i, lib=lib, geom=geom, out=out):
                    rc = lib.lsq_pool_w8_max(0, lx[i].data_ptr(), ctypes.byref(geom), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
                    assert rc == 0, rc
                    return out
                assert torch.equal(alt(0), y), "pix%d: not the default kernel's bytes" % n
                routes.append(alt)
            del y
            graphs = []
            for fn in routes:
                def run(fn=fn):
                    for i in range(iters):
                        fn(i % nsets)
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
        for _ in range(rounds + 1):                     # the first round warms up
            for j, g in enumerate(graphs):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                g.replay()
                t1.record()
                t1.synchronize()
                times[j].append(t0.elapsed_time(t1) * 1e3 / iters)
        med = [statistics.median(t[1:]) for t in times]
        tn, tp, tc = med[:3]
        spread = (max(times[0][1:]) - min(times[0][1:])) / tn
        spreads.append(spread)
        mark = "HIT" if tn / tp < 1.0 else "MISS"
        if mark == "MISS":
            misses.append(name)
        line = "%-18s %5d %-14s %5d | %8.1f %6.3f %5.1f | %9.1f %6.2f | %8.1f %5.1f | %-9s | %s" % (
            name, iters, plan["family"], lanes, tn, spread, 100 * (x_bytes + y_bytes) / (tn * 1e-6) / PEAK, tp, tn / tp, tc,
            100 * 2 * x_bytes / (tc * 1e-6) / PEAK, mark,
            " ".join("pix%d %.1f" % (n, t) for n, t in zip(alts, med[3:])) if len(med) > 3 else "-")
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                  # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del graphs, lx, dst
        torch.cuda.empty_cache()
    lines.append("# largest spread of the new route's rounds: %.3f" % max(spreads))
    lines.append("# expectation (new / parent < 1.0 in every case): %s" % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
