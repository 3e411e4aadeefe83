#!/usr/bin/env python3
"""A/B: LayerNorm and RMSNorm on 8-bit levels (liblsq_hip_norm_w8.so: lsq_layer_norm_w8_q8_q, lsq_rms_norm_w8_q8_q) against the route
of the parent commit on the same inputs, uint8 levels in and out, mid_dtype bfloat16, float32 w and bias: ConvNeXt-T's four stages
at batch 32 (96@56^2, 192@28^2, 384@14^2, 768@7^2, LayerNorm over C per pixel of channels-last levels), ViT-B [64 * 197, 768] and
ViT-L [64 * 197, 1024] (LayerNorm), and RMSNorm on [2048, 4096].

    new     one launch on the bytes: one byte read and one written per activation
    parent  LevelsTensor.dequantize(bfloat16) -> F.layer_norm (RMS: the composition x * rsqrt(mean(x^2) + eps) * w in bfloat16's
            float32 arithmetic) -> lsq_levels_per_tensor: about 10 bytes per activation and three launches or more
    copy    a plain device-to-device copy of the input's bytes: the yardstick of a bandwidth kernel
    variants (when tools/_tune/liblsq_hip_norm_w8_<v>.so exists: --build-variants compiles them) k1, k16: a group walks at most
            1 / 16 rows (-DLSQ_NORM_W8_MAX_ROWS; the library: 8); wide: the fewest packets per lane whatever lanes that masks
            (-DLSQ_NORM_W8_WIDE=1)

Before any timing the new route's levels are compared with the float composition on the float32 dequantized values (F.layer_norm
or the RMS formula, one rounding to bfloat16, lsq_levels_per_tensor): the two are NOT the same definition, so the
share of levels that differ is reported, and no level may differ by more than one.  The timed parent route dequantizes to bfloat16
first, which moves every input by up to 2^-9 of its value before the norm: against it the share and the largest difference are
reported, not bounded.  Two launches of the new route are
compared bit for bit; and the output quantizer is held to the non-vacuity conditions.  Then each route is captured as ONE graph of
back-to-back calls, one per input set, over as many sets as exceed the 256 MB Infinity Cache by a quarter (at least ITERS calls),
and ROUNDS rounds alternate the graphs in one process, timed with HIP events.  Reported: the median microseconds per call of each
route, the spread of the new route's rounds ((max - min) / median), new / parent, new / copy, and the algorithmic bytes (input +
output) over the time as a share of 8 TB/s for the new route and (twice the input) for the copy.

Expectation from byte counts, marked per line (`HIT` / `MISS`): new / parent < 1.0 in every case.

    python tools/exp_norm_w8_ab.py [--quick] [--out FILE] [--build-variants]
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

# (name, kind, shape of the levels, dim)
CASES = [("convnext 96@56", "layer", (32, 96, 56, 56), 1), ("convnext 192@28", "layer", (32, 192, 28, 28), 1),
         ("convnext 384@14", "layer", (32, 384, 14, 14), 1), ("convnext 768@7", "layer", (32, 768, 7, 7), 1),
         ("vit-b 12608x768", "layer", (64 * 197, 768), -1), ("vit-l 12608x1024", "layer", (64 * 197, 1024), -1),
         ("rms 2048x4096", "rms", (2048, 4096), -1)]
CACHE_BYTES = 256 << 20
PEAK = 8e12
RNG = (0, 255, 0, 255)
CL = torch.channels_last
TUNE = os.path.join(ROOT, "tools", "_tune")
VARIANTS = {"k1": "-DLSQ_NORM_W8_MAX_ROWS=1", "k16": "-DLSQ_NORM_W8_MAX_ROWS=16", "wide": "-DLSQ_NORM_W8_WIDE=1"}
EPS = {"layer": 1e-6, "rms": 1e-6}


def build_variants():
    """the kernels' variants, with the Makefile's flags, into tools/_tune/"""
    os.makedirs(TUNE, exist_ok=True)
    src = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "csrc", "norm_w8", "lsq_norm_w8.hip")
    for name, flag in VARIANTS.items():
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                               "-fhip-fp32-correctly-rounded-divide-sqrt", flag, "-shared", src, "-o",
                               os.path.join(TUNE, "liblsq_hip_norm_w8_%s.so" % name)])


def levels(n_rows, C, gen, dev):
    """the tests' construction: a row mean uniform in 0..255, a row spread uniform in 1..80, rounded and clamped"""
    mean = torch.rand(n_rows, 1, device=dev, generator=gen) * 255
    spread = 1 + torch.rand(n_rows, 1, device=dev, generator=gen) * 79
    return (mean + spread * torch.randn(n_rows, C, device=dev, generator=gen)).round().clamp(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, three cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_norm_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--build-variants", action="store_true", help="compile the variants of the kernels and exit")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq._abi import LsqNormW8Consts, LsqNormW8Geom
    from torchlsq.functional import LevelsTensor, lsq_layer_norm_w8, lsq_layer_norm_w8_q, lsq_rms_norm_w8, lsq_rms_norm_w8_q
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    cases = [CASES[1], CASES[4], CASES[6]] if args.quick else CASES
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x = torch.tensor([0.02], device=dev)
    zx = torch.tensor([128], dtype=torch.int32, device=dev)
    alts = {}
    for name in VARIANTS:
        path = os.path.join(TUNE, "liblsq_hip_norm_w8_%s.so" % name)
        if os.path.isfile(path):
            lib = ctypes.CDLL(path)
            lib.lsq_norm_w8.restype = ctypes.c_int
            lib.lsq_norm_w8.argtypes = [ctypes.c_void_p] * 5
            alts[name] = lib
    lines = ["# exp_norm_w8_ab: LayerNorm and RMSNorm on 8-bit levels (liblsq_hip_norm_w8.so) vs the parent's route (dequantize to "
             "bfloat16, F.layer_norm or the RMS composition, lsq_levels_per_tensor) and vs a device-to-device copy of the input; %s, %d CUs" % (
                 torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over as many input sets "
             "(1.25 x the 256 MB cache); spread = (max - min) / median of the new route's rounds; uint8 levels in and out, mid_dtype "
             "bfloat16, float32 w and bias (the parent's F.layer_norm takes them as bfloat16: torch's GPU kernel wants the input's dtype); "
             "diff %%: the share of levels where the new route differs from the float composition on the float32 dequantized values "
             "(F.layer_norm / the RMS formula, one rounding to bfloat16, the levels op), never by more than one level: asserted before any "
             "timing; p.diff %% / max: the same against the timed parent route, whose dequantize to bfloat16 moves every input by up to "
             "2^-9 of its value before the norm, and the largest difference in levels; %%: (input + output bytes) / time over 8 TB/s (copy: twice the input); LxP: lanes per "
             "row x packets per lane, rows: per workgroup, par: where w and bias live" % rounds,
             "%-17s %5s %-5s %4s %-4s | %8s %6s %5s %6s | %9s %6s %8s %3s | %8s %5s %6s | %s | %s" % (
                 "case", "calls", "LxP", "rows", "par", "new us", "spread", "%", "diff %", "parent us", "new/p", "p.diff %", "max", "copy us", "%",
                 "new/c", "new/p < 1", "variants us")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    spreads, misses = [], []
    for name, kind, shape, dim in cases:
        C = shape[1] if dim == 1 else shape[-1]
        x_bytes = 1
        for v in shape:
            x_bytes *= v
        n_rows = x_bytes // C
        nsets = -(-CACHE_BYTES * 5 // 4 // x_bytes)
        iters = max(args.iters, nsets)
        lx = []
        for _ in range(nsets):
            lv = levels(n_rows, C, gen, dev)
            lx.append(lv.reshape(shape[0], shape[2], shape[3], C).permute(0, 3, 1, 2) if dim == 1 else lv)
        assert dim != 1 or lx[0].is_contiguous(memory_format=CL)
        dst = torch.empty_like(lx[0])
        w = 1 + 0.2 * torch.randn(C, device=dev, generator=gen)
        b = 0.3 * torch.randn(C, device=dev, generator=gen) if kind == "layer" else None
        w16, b16 = w.to(torch.bfloat16), None if b is None else b.to(torch.bfloat16)
        eps = EPS[kind]
        fq, ff = (lsq_layer_norm_w8_q, lsq_layer_norm_w8) if kind == "layer" else (lsq_rms_norm_w8_q, lsq_rms_norm_w8)
        plan = E.norm_w8_plan(n_rows, C, has_bias=b is not None, kind=kind)
        v = ff(LevelsTensor(lx[0], s_x, zx, *RNG), w, b, eps, torch.float32, dim=dim)
        sd = 1.4826 * (v - v.median()).abs().median()
        osc = (sd / 64).reshape(1)
        osh = -128 * osc
        del v

        def rows_of(t):                                 # channels-last [B, C, H, W] as the dense view [B, H, W, C]
            return t.permute(0, 2, 3, 1) if dim == 1 else t

        def back(t):
            return t.permute(0, 3, 1, 2) if dim == 1 else t

        op = ops.lsq_layer_norm_w8_q8_q if kind == "layer" else ops.lsq_rms_norm_w8_q8_q
        assert torch.equal(fq(LevelsTensor(lx[0], s_x, zx, *RNG), w, b, eps, osc, osh, 0, 255, mid_dtype=torch.bfloat16, dim=dim).levels,
                           back(op(rows_of(lx[0]), s_x, zx, w, b, eps, osc, osh, *RNG, torch.bfloat16))), "the op is not the functional form"

        def new(i):                                     # the op itself, as the functional form and the modules call it
            return back(op(rows_of(lx[i]), s_x, zx, w, b, eps, osc, osh, *RNG, torch.bfloat16))

        def parent(i):
            xd = LevelsTensor(lx[i], s_x, zx, *RNG).dequantize(torch.bfloat16)
            if dim == 1:
                xd = xd.permute(0, 2, 3, 1)
            if kind == "layer":
                y = F.layer_norm(xd, (C,), w16, b16, eps)               # torch's GPU layer_norm wants w and bias in the input's dtype
            else:
                xf = xd.float()
                y = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w).to(torch.bfloat16)
            if dim == 1:
                y = y.permute(0, 3, 1, 2)
            return ops.lsq_levels_per_tensor(y, osc, osh, *RNG, 0).view(torch.uint8)

        def composed(i):
            """the float composition on the float32 dequantized values, float32 w and bias, one rounding to bfloat16: what the
            new route is held to within one level"""
            xd = LevelsTensor(lx[i], s_x, zx, *RNG).dequantize(torch.float32)
            if dim == 1:
                xd = xd.permute(0, 2, 3, 1)
            if kind == "layer":
                y = F.layer_norm(xd, (C,), w, b, eps)
            else:
                y = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps) * w
            if dim == 1:
                y = y.permute(0, 3, 1, 2)
            return ops.lsq_levels_per_tensor(y.to(torch.bfloat16), osc, osh, *RNG, 0).view(torch.uint8)

        def copy(i):
            return dst.copy_(lx[i])

        assert plan["family"] == "packets"
        routes = [new, parent, copy]
        names = []
        with torch.no_grad():
            y = new(0)
            assert torch.equal(y, new(0)), "two launches differ"
            assert dim != 1 or y.is_contiguous(memory_format=CL)
            d = (y.to(torch.int16) - composed(0).to(torch.int16)).abs()
            assert int(d.max()) <= 1, "the new route and the float composition differ by more than one level"
            differ = 100 * (d > 0).float().mean().item()
            d = (y.to(torch.int16) - parent(0).to(torch.int16)).abs()
            pdiffer, pmax = 100 * (d > 0).float().mean().item(), int(d.max())
            inside = ((y > 0) & (y < 255)).float().mean().item()
            assert len(y.unique()) > 32 and 0.25 <= inside and bool((y == 0).any()) and bool((y == 255).any()), \
                "a vacuous output quantizer (%.2f inside)" % inside
            for vname, lib in alts.items():
                rows_ = lx[0].permute(0, 2, 3, 1) if dim == 1 else lx[0]
                out = torch.empty_like(rows_)
                consts = LsqNormW8Consts(s_x.data_ptr(), zx.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), osc.data_ptr(),
                                         osh.data_ptr(), E.LSQ_F32, 0, 255, 0, 255, E.LSQ_BF16, eps)
                geom = LsqNormW8Geom(n_rows, C, 0 if kind == "layer" else 1, 0)

                def alt(i, lib=lib, out=out, consts=consts, geom=geom):
                    rc = lib.lsq_norm_w8(ctypes.addressof(geom), ctypes.addressof(consts), lx[i].data_ptr(), out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
                    assert rc == 0, rc
                    return out
                assert torch.equal(alt(0).reshape(-1), (y.permute(0, 2, 3, 1) if dim == 1 else y).reshape(-1)), "%s: not the default kernel's bytes" % vname
                routes.append(alt)
                names.append(vname)
            del y, d
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
        line = "%-17s %5d %-5s %4d %-4s | %8.1f %6.3f %5.1f %6.3f | %9.1f %6.2f %8.3f %3d | %8.1f %5.1f %6.2f | %-9s | %s" % (
            name, iters, "%dx%d" % (plan["lanes_per_row"], plan["packets_per_lane"]), plan["rows_per_workgroup"], plan["params"][:4], tn,
            spread, 100 * 2 * x_bytes / (tn * 1e-6) / PEAK, differ, tp, tn / tp, pdiffer, pmax, tc, 100 * 2 * x_bytes / (tc * 1e-6) / PEAK, tn / tc, mark,
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
