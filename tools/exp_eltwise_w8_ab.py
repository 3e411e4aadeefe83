#!/usr/bin/env python3
"""A/B: the elementwise ops on 8-bit levels (liblsq_hip_eltwise_w8.so: lsq_lut_w8, lsq_mul_gate_w8_q8_q) against the route of the
parent commit on the same inputs, at batch 32, uint8 levels in and out, mid_dtype bfloat16: the table op as hardswish on 16@112^2,
240@28^2, 960@7^2 and as SiLU on 32@112^2, 144@56^2; the gate multiply on 96@28^2, 480@14^2, 960@7^2.

    new     one launch on the bytes: one byte read and one written per activation (the table is built once, outside the timing)
    parent  table op: LevelsTensor.dequantize(bfloat16) -> the torch function -> lsq_levels_per_tensor;
            gate multiply: the two dequantize(bfloat16), torch.mul, lsq_levels_per_tensor: the activation as floats twice and more
    copy    a plain device-to-device copy of the input's bytes: the yardstick of a bandwidth kernel
    variants (table op only, when tools/_tune/liblsq_hip_eltwise_w8_<v>.so exists: --build-variants compiles them) p1, p4: at most
            1 / 4 packets per lane (-DLSQ_ELTWISE_W8_LUT_P; the library: 2); c2, c4: 2 / 4 copies of the table in LDS, one per group
            of 32 lanes in turn (-DLSQ_ELTWISE_W8_LUT_COPIES; the library: 1)

Before any timing the new route's bytes are compared with the parent route's (the definition on the same device), two launches are
compared bit for bit, and the gate multiply's output quantizer is held to the non-vacuity conditions.  Then each route is captured
as ONE graph of back-to-back calls, one per input set, over as many sets as exceed the 256 MB Infinity Cache by a quarter (at
least ITERS calls), and ROUNDS rounds alternate the graphs in one process, timed with HIP events.  Reported: the median
microseconds per call of each route, the spread of the new route's rounds ((max - min) / median), new / parent, new / copy, and the
algorithmic bytes (input + output) over the time as a share of 8 TB/s for the new route and (twice the input) for the copy.

Expectation from byte counts, marked per line (`HIT` / `MISS`): new / parent < 1.0 in every case.

    python tools/exp_eltwise_w8_ab.py [--quick] [--out FILE] [--build-variants]
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

# (name, kind, function, batch, C, H = W)
CASES = [("hardswish 16@112", "lut", "hardswish", 32, 16, 112), ("hardswish 240@28", "lut", "hardswish", 32, 240, 28),
         ("hardswish 960@7", "lut", "hardswish", 32, 960, 7), ("silu 32@112", "lut", "silu", 32, 32, 112),
         ("silu 144@56", "lut", "silu", 32, 144, 56), ("gate 96@28", "mul", None, 32, 96, 28), ("gate 480@14", "mul", None, 32, 480, 14),
         ("gate 960@7", "mul", None, 32, 960, 7)]
CACHE_BYTES = 256 << 20
PEAK = 8e12
RNG = (0, 255, 0, 255)
CL = torch.channels_last
TUNE = os.path.join(ROOT, "tools", "_tune")
VARIANTS = {"p1": "-DLSQ_ELTWISE_W8_LUT_P=1", "p4": "-DLSQ_ELTWISE_W8_LUT_P=4", "c2": "-DLSQ_ELTWISE_W8_LUT_COPIES=2",
            "c4": "-DLSQ_ELTWISE_W8_LUT_COPIES=4"}


def build_variants():
    """the table kernel's variants, with the Makefile's flags, into tools/_tune/"""
    os.makedirs(TUNE, exist_ok=True)
    src = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "csrc", "eltwise_w8", "lsq_eltwise_w8.hip")
    for name, flag in VARIANTS.items():
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                               "-fhip-fp32-correctly-rounded-divide-sqrt", flag, "-shared", src, "-o",
                               os.path.join(TUNE, "liblsq_hip_eltwise_w8_%s.so" % name)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, three cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_eltwise_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--build-variants", action="store_true", help="compile the variants of the table kernel and exit")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, lsq_act_table
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [CASES[1], CASES[4], CASES[6]] if args.quick else CASES
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x = torch.tensor([0.0371], device=dev)
    zx = torch.tensor([128], dtype=torch.int32, device=dev)
    s_g = torch.tensor([1 / 255], device=dev)
    zg = torch.tensor([0], dtype=torch.int32, device=dev)
    alts = {}
    for name in VARIANTS:
        path = os.path.join(TUNE, "liblsq_hip_eltwise_w8_%s.so" % name)
        if os.path.isfile(path):
            lib = ctypes.CDLL(path)
            lib.lsq_eltwise_w8_lut.restype = ctypes.c_int
            lib.lsq_eltwise_w8_lut.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
            alts[name] = lib
    lines = ["# exp_eltwise_w8_ab: the table op and the gate multiply on 8-bit levels (liblsq_hip_eltwise_w8.so) vs the parent's route "
             "(dequantize to bfloat16, the torch op, lsq_levels_per_tensor) and vs a device-to-device copy of the input; %s, %d CUs" % (
                 torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over as many input sets "
             "(1.25 x the 256 MB cache); spread = (max - min) / median of the new route's rounds; batch 32, uint8 levels in and out, "
             "mid_dtype bfloat16; the new route's bytes checked against the parent's route on the same inputs before any timing; "
             "%%: (input + output bytes) / time over 8 TB/s (copy: twice the input); per: packets (table op) / pixels (gate) per lane" % rounds,
             "%-17s %5s %-8s %3s | %8s %6s %5s | %9s %6s | %8s %5s %6s | %s | %s" % (
                 "case", "calls", "family", "per", "new us", "spread", "%", "parent us", "new/p", "copy us", "%", "new/c", "new/p < 1", "variants us")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    spreads, misses = [], []
    for name, kind, fn, B, C, HW in cases:
        x_bytes = B * C * HW * HW
        nsets = -(-CACHE_BYTES * 5 // 4 // x_bytes)
        iters = max(args.iters, nsets)
        lx = [torch.randint(0, 256, (B, C, HW, HW), device=dev, generator=gen, dtype=torch.uint8).contiguous(memory_format=CL)
              for _ in range(nsets)]
        dst = torch.empty_like(lx[0])
        if kind == "lut":
            plan = E.eltwise_w8_plan_lut(x_bytes)
            per = plan["packets_per_lane"]
            call = {"hardswish": F.hardswish, "silu": F.silu}[fn]
            v = call(LevelsTensor(lx[0], s_x, zx, *RNG).dequantize(torch.float32))
            osc = ((v.max() - v.min()) / 255).reshape(1)
            osh = v.min().reshape(1).clone()
            table = lsq_act_table(fn, s_x, zx, torch.uint8, osc, osh, 0, 255, mid_dtype=torch.bfloat16)

            def new(i):
                return ops.lsq_lut_w8(lx[i], table, torch.uint8)

            def parent(i):
                y = call(LevelsTensor(lx[i], s_x, zx, *RNG).dequantize(torch.bfloat16))
                return ops.lsq_levels_per_tensor(y, osc, osh, *RNG, 0).view(torch.uint8)
        else:
            plan = E.eltwise_w8_plan_mul(B, C, HW, HW)
            per = plan["pixels_per_lane"]
            lg = [torch.randint(0, 256, (B, C, 1, 1), device=dev, generator=gen, dtype=torch.uint8) for _ in range(nsets)]
            v = ops.lsq_mul_gate_w8_q8(lx[0], s_x, zx, lg[0], s_g, zg, torch.float32)
            sd = 1.4826 * (v - v.median()).abs().median()
            osc = (sd / 64).reshape(1)
            osh = -128 * osc

            def new(i):
                return ops.lsq_mul_gate_w8_q8_q(lx[i], s_x, zx, lg[i], s_g, zg, osc, osh, *RNG, torch.bfloat16)

            def parent(i):
                y = torch.mul(LevelsTensor(lx[i], s_x, zx, *RNG).dequantize(torch.bfloat16),
                              LevelsTensor(lg[i], s_g, zg, *RNG).dequantize(torch.bfloat16))
                return ops.lsq_levels_per_tensor(y, osc, osh, *RNG, 0).view(torch.uint8)
        assert plan["family"] == "packets"

        def copy(i):
            return dst.copy_(lx[i])

        routes = [new, parent, copy]
        names = []
        with torch.no_grad():
            y = new(0)
            assert y.is_contiguous(memory_format=CL) and torch.equal(y, new(0)), "two launches differ"
            assert torch.equal(y, parent(0)), "not the bytes of the parent's route"
            inside = ((y > 0) & (y < 255)).float().mean().item()
            assert len(y.unique()) > 32 and (kind == "lut" or (0.25 <= inside and bool((y == 0).any()) and bool((y == 255).any()))), \
                "a vacuous output quantizer (%.2f inside)" % inside
            for vname, lib in alts.items() if kind == "lut" else ():
                out = torch.empty_like(y)

                def alt(i, lib=lib, out=out):
                    rc = lib.lsq_eltwise_w8_lut(lx[i].data_ptr(), table.data_ptr(), x_bytes, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
                    assert rc == 0, rc
                    return out
                assert torch.equal(alt(0), y), "%s: not the default kernel's bytes" % vname
                routes.append(alt)
                names.append(vname)
            del y
            graphs = []
            for fn_ in routes:
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
        line = "%-17s %5d %-8s %3d | %8.1f %6.3f %5.1f | %9.1f %6.2f | %8.1f %5.1f %6.2f | %-9s | %s" % (
            name, iters, plan["family"], per, tn, spread, 100 * 2 * x_bytes / (tn * 1e-6) / PEAK, tp, tn / tp, tc,
            100 * 2 * x_bytes / (tc * 1e-6) / PEAK, tn / tc, mark,
            " ".join("%s %.1f" % (n, t) for n, t in zip(names, med[3:])) if names else "-")
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
