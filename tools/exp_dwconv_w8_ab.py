#!/usr/bin/env python3
"""A/B: the W8A8 depthwise conv2d on 8-bit levels (liblsq_hip_dwconv_w8.so: lsq_dwconv2d_w8_q8_q) against the route of the parent
commit on the same inputs, at batch 32, uint8 levels in and out, int8 weights, mid_dtype bfloat16, ReLU6: MobileNetV2's depthwise
layers (32@112^2 s1, 96@112^2 s2, 144@56^2 s1 and s2, 192@28^2, 384@14^2, 960@7^2) and one 5 x 5 (240@28^2).

    new     one launch on the bytes: one byte read per activation, one written
    parent  LevelsTensor.dequantize(bfloat16) in channels-last memory -> F.conv2d(groups=C) on the dequantized bfloat16 weight ->
            F.relu6 -> lsq_levels_per_tensor with the output quantizer: the activation as floats three times and four launches
    copy    a plain device-to-device copy of the input's bytes: the floor of a bandwidth kernel
    variants (when tools/_tune/liblsq_hip_dwconv_w8_<name>.so exists: --build-variants compiles them) the same entry point built
            with -DLSQ_DWCONV_W8_DOT4=0 (`plain`: a byte product per channel and tap as the compiler schedules it, no register
            cap) and N = 1, 2, 4 output pixels per lane of the unrolled 3 x 3 kernels (-DLSQ_DWCONV_W8_PIX_S1=N
            -DLSQ_DWCONV_W8_PIX_S2=N): plain_p1, plain_p2, plain_p4.  The library itself is `dot4`, one pixel per lane.

Before any timing the new route's levels of the first two images are compared with the CPU path of the op (its definition; the
parent route rounds its sums in bfloat16 steps of its own and is a different function), every variant with the library's bytes,
and two launches bit for bit.  Then each route is captured as ONE graph of back-to-back calls, one per input set, over as many sets
as exceed the 256 MB Infinity Cache by a quarter (at least ITERS calls), and ROUNDS rounds alternate the graphs in one process,
timed with HIP events.  Reported: the median microseconds per call of each route, the spread of the new route's rounds
((max - min) / median), new / parent, and the algorithmic bytes (input + output + weight) over the time as a share of 8 TB/s for the
new route and (twice the input) for the copy.

Expectation from byte counts, marked per line (`HIT` / `MISS`): new / parent < 1.0 in every case.

    python tools/exp_dwconv_w8_ab.py [--quick] [--out FILE] [--build-variants] [--no-parent]
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

# (name, batch, C, H = W, kernel, stride, padding)
CASES = [("3x3 s1 32@112", 32, 32, 112, 3, 1, 1), ("3x3 s2 96@112", 32, 96, 112, 3, 2, 1), ("3x3 s1 144@56", 32, 144, 56, 3, 1, 1),
         ("3x3 s2 144@56", 32, 144, 56, 3, 2, 1), ("3x3 s1 192@28", 32, 192, 28, 3, 1, 1), ("3x3 s1 384@14", 32, 384, 14, 3, 1, 1),
         ("3x3 s1 960@7", 32, 960, 7, 3, 1, 1), ("5x5 s1 240@28", 32, 240, 28, 5, 1, 2)]
CACHE_BYTES = 256 << 20
PEAK = 8e12
RNG = (0, 255, 0, 255)
CL = torch.channels_last
TUNE = os.path.join(ROOT, "tools", "_tune")
VARIANTS = {"plain_p1": ("-DLSQ_DWCONV_W8_DOT4=0",),
            "plain_p2": ("-DLSQ_DWCONV_W8_DOT4=0", "-DLSQ_DWCONV_W8_PIX_S1=2", "-DLSQ_DWCONV_W8_PIX_S2=2"),
            "plain_p4": ("-DLSQ_DWCONV_W8_DOT4=0", "-DLSQ_DWCONV_W8_PIX_S1=4", "-DLSQ_DWCONV_W8_PIX_S2=4")}


def build_variants():
    """the build variants of the library, with the Makefile's flags, into tools/_tune/"""
    os.makedirs(TUNE, exist_ok=True)
    src = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "csrc", "dwconv_w8", "lsq_dwconv_w8.hip")
    for name, flags in VARIANTS.items():
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                               "-fhip-fp32-correctly-rounded-divide-sqrt", *flags, "-shared", src, "-o",
                               os.path.join(TUNE, "liblsq_hip_dwconv_w8_%s.so" % name)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, three cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_dwconv_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--build-variants", action="store_true", help="compile the build variants of the library and exit")
    ap.add_argument("--no-parent", action="store_true", help="leave the parent's route out (its column reads 0)")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [CASES[2], CASES[3], CASES[7]] if args.quick else CASES
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x = torch.tensor([1 / 32], device=dev)
    zx = torch.tensor([128], dtype=torch.int32, device=dev)
    alts = {}
    for name in VARIANTS:
        path = os.path.join(TUNE, "liblsq_hip_dwconv_w8_%s.so" % name)
        if os.path.isfile(path):
            lib = ctypes.CDLL(path)
            lib.lsq_dwconv_w8_forward_levels.restype = ctypes.c_int
            lib.lsq_dwconv_w8_forward_levels.argtypes = E.C_ABI_DWCONV_W8["lsq_dwconv_w8_forward_levels"][1]
            lib.lsq_dwconv_w8_plan.restype = ctypes.c_int
            lib.lsq_dwconv_w8_plan.argtypes = E.C_ABI_DWCONV_W8["lsq_dwconv_w8_plan"][1]
            alts[name] = lib
    lines = ["# exp_dwconv_w8_ab: the W8A8 depthwise conv2d on 8-bit levels (liblsq_hip_dwconv_w8.so) vs the parent's route (dequantize to "
             "bfloat16, F.conv2d(groups=C), F.relu6, lsq_levels_per_tensor) and vs a device-to-device copy of the input; %s, %d CUs" % (
                 torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over as many input sets "
             "(1.25 x the 256 MB cache); spread = (max - min) / median of the new route's rounds; batch 32, uint8 levels in and out, "
             "int8 weights, mid_dtype bfloat16, ReLU6; the new route's levels of two images checked against the CPU path and every variant "
             "against the library's bytes before any timing; %%: (input + output + weight bytes) / time over 8 TB/s (copy: twice the "
             "input); variants: name(pixels per lane the variant's plan chose) us" % rounds,
             "%-14s %5s %-8s %4s | %8s %6s %5s | %9s %6s | %8s %5s %6s | %s | %s" % (
                 "case", "calls", "family", "unr", "new us", "spread", "%", "parent us", "new/p", "copy us", "%", "new/c", "new/p < 1", "variants")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    spreads, misses, far = [], [], (0.0, "")
    for name, B, C, HW, k, st, pd in cases:
        x_bytes = B * C * HW * HW
        nsets = -(-CACHE_BYTES * 5 // 4 // x_bytes)
        iters = max(args.iters, nsets)
        lx = [(128 + 32 * torch.randn((B, C, HW, HW), device=dev, generator=gen)).round().clamp(0, 255).to(torch.uint8)
              .contiguous(memory_format=CL) for _ in range(nsets)]
        wl = torch.randint(-128, 128, (k, k, C), device=dev, generator=gen).to(torch.int8)
        w_s = torch.rand(C, device=dev, generator=gen) * 0.004 + 0.001
        w_z = torch.zeros(C, dtype=torch.int32, device=dev)
        bias = torch.randn(C, device=dev, generator=gen)
        geo = ([st, st], [pd, pd], [1, 1])
        plan = E.dwconv_w8_plan(B, C, HW, HW, k, st, pd)
        assert plan["family"] == "packets"
        osc = torch.tensor([6.0 / 255], device=dev)
        osh = torch.zeros(1, device=dev)
        # the parent's operands: the dequantized bfloat16 weight as F.conv2d takes it
        w_bf = ((wl.float() - w_z.float()) * w_s).permute(2, 0, 1).unsqueeze(1).to(torch.bfloat16).contiguous(memory_format=CL)
        b_bf = bias.to(torch.bfloat16)
        dst = torch.empty_like(lx[0])

        def new(i):
            return ops.lsq_dwconv2d_w8_q8_q(lx[i], s_x, zx, wl, w_s, w_z, bias, *geo, osc, osh, *RNG, 2, torch.bfloat16)

        def parent(i):
            y = F.relu6(F.conv2d(LevelsTensor(lx[i], s_x, zx, *RNG).dequantize(torch.bfloat16), w_bf, b_bf, st, pd, 1, C))
            return ops.lsq_levels_per_tensor(y, osc, osh, *RNG, 0).view(torch.uint8)

        def copy(i):
            return dst.copy_(lx[i])

        routes = [new, copy] if args.no_parent else [new, copy, parent]
        chosen = []
        with torch.no_grad():
            y = new(0)
            y_bytes = y.numel()
            assert torch.equal(y, new(0)), "two launches differ"
            want = ops.lsq_dwconv2d_w8_q8_q(lx[0][:2].cpu(), s_x.cpu(), zx.cpu(), wl.cpu(), w_s.cpu(), w_z.cpu(), bias.cpu(), *geo, osc.cpu(),
                                            osh.cpu(), *RNG, 2, torch.bfloat16)
            assert torch.equal(y[:2].cpu(), want), "not the levels of the CPU path"
            inside = ((y > 0) & (y < 255)).float().mean().item()
            assert 0.25 <= inside and bool((y == 0).any()) and bool((y == 255).any()), "a vacuous output quantizer (%.2f inside)" % inside
            geom = E.LsqQconvW8Geom(B, C, HW, HW, C, k, k, st, st, pd, pd, 1, 1)
            oq = E.LsqDwconvW8Out(osc.data_ptr(), osh.data_ptr(), *RNG, 2, E.LSQ_BF16)
            for vname, lib in alts.items():
                out8 = (ctypes.c_int32 * 8)()
                assert lib.lsq_dwconv_w8_plan(ctypes.byref(geom), 1, 1, ctypes.byref(out8)) == 0
                chosen.append("%s(%d)" % (vname, out8[3]))
                out = torch.empty_like(y)

                def alt(i, lib=lib, out=out):
                    rc = lib.lsq_dwconv_w8_forward_levels(0, lx[i].data_ptr(), s_x.data_ptr(), zx.data_ptr(), ctypes.byref(geom), 1, wl.data_ptr(),
                                                          w_s.data_ptr(), w_z.data_ptr(), bias.data_ptr(), E.LSQ_F32, ctypes.byref(oq),
                                                          out.data_ptr(), torch.cuda.current_stream().cuda_stream)
                    assert rc == 0, rc
                    return out
                assert torch.equal(alt(0), y), "%s: not the library's bytes" % vname
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
        if args.no_parent:
            med.insert(2, 0.0)
        tn, tc, tp = med[:3]
        spread = (max(times[0][1:]) - min(times[0][1:])) / tn
        spreads.append(spread)
        mark = "-" if tp == 0 else "HIT" if tn / tp < 1.0 else "MISS"
        if mark == "MISS":
            misses.append(name)
        if tn / tc > far[0]:
            far = (tn / tc, name)
        line = "%-14s %5d %-8s %4d | %8.1f %6.3f %5.1f | %9.1f %6.2f | %8.1f %5.1f %6.2f | %-9s | %s" % (
            name, iters, plan["family"], plan["unrolled_window"], tn, spread, 100 * (x_bytes + y_bytes + wl.numel()) / (tn * 1e-6) / PEAK, tp,
            tn / tp if tp else 0.0, tc, 100 * 2 * x_bytes / (tc * 1e-6) / PEAK, tn / tc, mark,
            " ".join("%s %.1f" % (n, t) for n, t in zip(chosen, med[3:])) if len(med) > 3 else "-")
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:                  # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
        del graphs, lx, dst
        torch.cuda.empty_cache()
    lines.append("# largest spread of the new route's rounds: %.3f" % max(spreads))
    lines.append("# furthest from the copy: %s, new / copy = %.2f" % (far[1], far[0]))
    lines.append("# expectation (new / parent < 1.0 in every case): %s" % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))


if __name__ == "__main__":
    main()
