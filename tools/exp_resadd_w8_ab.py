#!/usr/bin/env python3
"""A/B: the W8A8 layers that close a residual block (liblsq_hip_resadd_w8.so, lsq_conv2d_w8_q8_add_q / lsq_linear_w8_q8_add_q)
against the route of the parent commit on the same inputs, on ResNet-18/50-style block ends at batch 32, on the bottleneck's
last 1 x 1 layer (64 -> 256 at 56 x 56, the largest output) and on a [4096, 4096] linear layer at M = 2048; `pre` off and on.

    new     lsq_*_w8_q8_add_q: uint8 levels in, (the layer's own fake-quantizer,) the residual's uint8 levels added, ReLU and
            the add's quantizer in the epilogue, uint8 levels out: one launch, one byte read and one written per output
    parent  lsq_*_w8_q8 writing a bfloat16 y, (lsq for `pre`,) LevelsTensor.dequantize(bfloat16) of the residual, torch.add,
            torch.relu, lsq_levels_per_tensor: the block's output as floats four times and four to five more launches
    plain   lsq_*_w8_q8_q on the same layer WITHOUT a residual (and without `pre`): new / plain is the price of the residual

Per case the new route is compared BIT FOR BIT with the parent route (which is its definition) on the first input set, and two
launches are compared bit for bit; the quantizers are taken from the data (residual scale sd / 32 of the layer's float result,
`pre` scale sd / 16, output scale sd / 96 of the sum, zero point 0) so that about half of the levels lie strictly inside 0..255.
Then each route is captured as ONE graph of back-to-back calls, one per input set (levels AND residual), over as many sets as
make the input levels alone exceed the 256 MB Infinity Cache by a quarter (at least ITERS calls; the column `calls`), and ROUNDS
rounds alternate the graphs in one process, timed with HIP events.  Reported: the median microseconds per call of each route,
the spread of the new route's rounds ((max - min) / median), new / parent and new / plain.

Expectation from byte counts, marked per line (`HIT` / `MISS`): new / parent < 1.0 in every case.

    python tools/exp_resadd_w8_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

BATCH = 32
# (name, Cin, H = W, Cout, kernel, stride, padding)
CONVS = [("3x3 64@56", 64, 56, 64, 3, 1, 1), ("3x3 128@28", 128, 28, 128, 3, 1, 1), ("3x3 256@14", 256, 14, 256, 3, 1, 1),
         ("3x3 512@7", 512, 7, 512, 3, 1, 1), ("1x1 64>256@56", 64, 56, 256, 1, 1, 0)]
# (name, M, N, K)
LINEARS = [("4096x4096 M=2048", 2048, 4096, 4096)]
CACHE_BYTES = 256 << 20
S_X, ZX = 0.02, 125
RNG = (0, 255, 0, 255)
CL = torch.channels_last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, two convolutions, no linear case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_resadd_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import LevelsTensor, lsq
    ops = torch.ops.torchlsq
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    convs = [CONVS[0], CONVS[3]] if args.quick else CONVS
    linears = [] if args.quick else LINEARS
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x = torch.tensor([S_X], device=dev)
    zx = torch.tensor([ZX], dtype=torch.int32, device=dev)
    lines = ["# exp_resadd_w8_ab: the W8A8 layers that close a residual block (liblsq_hip_resadd_w8.so: the residual's levels, ReLU and "
             "the add's quantizer in the epilogue) vs the parent's route (the float-output op with a bfloat16 y, (lsq,) dequantize, "
             "add, relu, lsq_levels_per_tensor) and vs the same layer without a residual (lsq_*_w8_q8_q); batch %d; %s, %d CUs" % (
                 BATCH, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over as many input sets "
             "(their levels: 1.25 x the 256 MB cache; a residual per set); spread = (max - min) / median of the new route's rounds; "
             "uint8 levels in and out, mid_dtype bfloat16, relu on; bit identity of new and parent checked before any timing" % rounds,
             "%-17s %-3s %5s %-13s %-7s | %9s %6s | %9s %6s | %9s %6s | %s" % (
                 "layer", "pre", "calls", "shape", "res", "new us", "spread", "parent us", "new/p", "plain us", "new/pl", "new/p < 1")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    spreads, misses = [], []
    cases = [("conv",) + c for c in convs] + [("linear",) + c for c in linears]
    for case in cases:
        if case[0] == "conv":
            _, name, Cin, HW, N, k, stride, padding = case
            geo = ([stride, stride], [padding, padding], [1, 1])
            plan = E.resadd_w8_plan_conv(BATCH, Cin, HW, HW, N, k, stride, padding)
            M, K = plan["M"], plan["K"]
            x_shape, w_shape, y_shape = (BATCH, Cin, HW, HW), (N, Cin, k, k), (BATCH, N, HW, HW)
        else:
            _, name, M, N, K = case
            geo = ()
            plan = E.resadd_w8_plan_linear(M, N, K)
            x_shape, w_shape, y_shape = (M, K), (N, K), (M, N)
        assert plan["form"] == "mfma" and plan["store"] == "packets" and plan["res_load"] == "packets"
        x_bytes = M * K if case[0] == "linear" else BATCH * Cin * HW * HW
        nsets = -(-CACHE_BYTES * 5 // 4 // x_bytes)                # the levels of the sets exceed the cache by a quarter ...
        iters = max(args.iters, nsets)                              # ... and one graph walks all of them
        lw = torch.randint(-128, 128, w_shape, dtype=torch.int8, device=dev, generator=gen)
        lx = [torch.randint(0, 256, x_shape, dtype=torch.uint8, device=dev, generator=gen) for _ in range(nsets)]
        rl = [(128 + 32 * torch.randn(y_shape, device=dev, generator=gen)).round().clamp(0, 255).to(torch.uint8) for _ in range(nsets)]
        if case[0] == "conv":
            lw = lw.contiguous(memory_format=CL)
            lx = [v.contiguous(memory_format=CL) for v in lx]
            rl = [v.contiguous(memory_format=CL) for v in rl]
        s_w = torch.rand(N, device=dev, generator=gen) * 0.002 + 0.0001
        zw = torch.randint(-9, 10, (N,), dtype=torch.int32, device=dev, generator=gen)
        bias = torch.randn(N, device=dev, generator=gen)
        float_op = ops.lsq_conv2d_w8_q8 if case[0] == "conv" else ops.lsq_linear_w8_q8
        plain_op = ops.lsq_conv2d_w8_q8_q if case[0] == "conv" else ops.lsq_linear_w8_q8_q
        new_op = ops.lsq_conv2d_w8_q8_add_q if case[0] == "conv" else ops.lsq_linear_w8_q8_add_q
        sd = float_op(lx[0], s_x, zx, lw, s_w, zw, bias, *geo, torch.float32).std()
        rs, rz = (sd / 32).reshape(1), torch.tensor([128], dtype=torch.int32, device=dev)
        res = [LevelsTensor(v, rs, rz, 0, 255) for v in rl]
        psc = (sd / 16).reshape(1)
        psh = -128 * psc
        osc, osh = (sd * 2 ** 0.5 / 96).reshape(1), torch.zeros(1, device=dev)     # the sum of two parts of deviation sd

        for pre_on in (False, True):
            pre = (psc, psh, *RNG) if pre_on else (None, None, *RNG)

            def new(i):
                return new_op(lx[i], s_x, zx, lw, s_w, zw, bias, *geo, osc, osh, *RNG, True, torch.bfloat16, rl[i], rs, rz, *pre)

            def parent(i):
                y = float_op(lx[i], s_x, zx, lw, s_w, zw, bias, *geo, torch.bfloat16)
                if pre_on:
                    y = lsq(y, psc, psh, *RNG)
                t = torch.relu(torch.add(y, res[i].dequantize(torch.bfloat16)))
                return ops.lsq_levels_per_tensor(t, osc, osh, *RNG, 0).view(torch.uint8)

            def plain(i):
                return plain_op(lx[i], s_x, zx, lw, s_w, zw, bias, *geo, osc, osh, *RNG, True, torch.bfloat16)

            # bit identity with the parent's route and repeatability before any timing
            with torch.no_grad():
                y = new(0)
                assert torch.equal(y, new(0)), "two launches differ"
                assert torch.equal(y, parent(0)), "not the bits of the parent's route"
                inside = ((y > 0) & (y < 255)).float().mean().item()
                assert 0.25 <= inside and bool((y == 0).any()) and bool((y == 255).any()), "a vacuous output quantizer (%.2f inside)" % inside
                assert (y != plain(0)).float().mean().item() >= 0.4, "the residual does not show"
                del y

                graphs = []
                for fn in (new, parent, plain):
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
            times = [[], [], []]
            for _ in range(rounds + 1):                     # the first round warms up
                for j, g in enumerate(graphs):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    g.replay()
                    t1.record()
                    t1.synchronize()
                    times[j].append(t0.elapsed_time(t1) * 1e3 / iters)
            tn, tp, tl = (statistics.median(t[1:]) for t in times)
            spread = (max(times[0][1:]) - min(times[0][1:])) / tn
            spreads.append(spread)
            mark = "HIT" if tn / tp < 1.0 else "MISS"
            if mark == "MISS":
                misses.append("%s pre %s" % (name, "on" if pre_on else "off"))
            line = "%-17s %-3s %5d %-13s %-7s | %9.1f %6.3f | %9.1f %6.2f | %9.1f %6.2f | %s" % (
                name, "on" if pre_on else "off", iters, plan["shape"], plan["res_load"], tn, spread, tp, tn / tp, tl, tn / tl, mark)
            print(line, flush=True)
            lines.append(line)
            with open(args.out, "w") as f:                  # kept current: a run that is cut short leaves what it measured
                f.write("\n".join(lines) + "\n")
            del graphs
        del lx, rl, res
        torch.cuda.empty_cache()
    lines.append("# largest spread of the new route's rounds: %.3f" % max(spreads))
    lines.append("# expectation (new / parent < 1.0 in every case): %s" % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
