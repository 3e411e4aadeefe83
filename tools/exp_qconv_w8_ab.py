#!/usr/bin/env python3
"""A/B: the W8A8 conv2d on channels-last 8-bit levels (liblsq_hip_qconv_w8.so, lsq_conv2d_w8_q8 / lsq_conv2d_w8_a8) against the
two routes a user had before it, on ResNet-50's 3 x 3 layers at batch 32.

    new  lsq_conv2d_w8_q8 (uint8 levels in, bfloat16 y) / lsq_conv2d_w8_a8 (bfloat16 x in)      reads x once
    (a)  the route of the parent commit: F.pad with the level zx + F.unfold of the levels + lsq_linear_w8_q8 on the
         [B OH OW, Cin kh kw] matrix (fused form: lsq_levels_per_tensor first)                  writes and re-reads kh kw copies of x
         -- as a user can write it: F.unfold has no byte kernel, so the padded levels are cast to bfloat16 (exact), unfolded,
         transposed and cast back: about 2 x kh kw bytes written per element of x instead of kh kw
    (b)  F.conv2d in bfloat16, channels-last, on the dequantized tensors                        no integer sum, no bit contract

Per case (input form x layer): the new route's first image is compared BIT FOR BIT with the definition -- the exact integer
tensor from a float64 convolution of lx - zx with lw - zw on the device (|I| < 2^53), then the contract's fp32 steps as
individually rounded tensor operations --, two launches are compared bit for bit, and route (a), which forms the same integers,
must give the same bits; then each route is captured as ONE graph of back-to-back calls, one per input set, over as many sets
as make the levels alone exceed the 256 MB Infinity Cache by a quarter (at least ITERS calls; the column `calls`), and ROUNDS
rounds alternate the graphs in one process, timed with HIP events.  Reported: the median microseconds
per call of each route, the spread of the new route's rounds ((max - min) / median), the int8 TOP/s (2 M N K / time), and the
ratios new / (a), new / (b).

Expectation from byte counts, marked per line (`HIT` / `MISS`): new / (a) < 1.0 in every case.  new / (b) is reported without a
claim.

    python tools/exp_qconv_w8_ab.py [--quick] [--form levels|fused] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

BATCH = 32
# (name, Cin, H = W, Cout, kernel, stride, padding)
LAYERS = [("3x3 64@56", 64, 56, 64, 3, 1, 1), ("3x3 128@28", 128, 28, 128, 3, 1, 1), ("3x3 256@14", 256, 14, 256, 3, 1, 1),
          ("3x3 512@7", 512, 7, 512, 3, 1, 1), ("3x3s2 128@56", 128, 56, 128, 3, 2, 1), ("1x1 256>64@56", 256, 56, 64, 1, 1, 0)]
CACHE_BYTES = 256 << 20
S_X, ZX = 0.02, 125                             # the activation quantizer: scale 0.02, shift -2.5, levels 0..255
CL = torch.channels_last


def unfold_levels(lx, k, stride, padding):
    """[B OH OW, Cin k k] uint8: the padding holds the level ZX; F.unfold has no byte kernel, bfloat16 carries 0..255 exactly"""
    cols = F.unfold(F.pad(lx, (padding,) * 4, value=ZX).to(torch.bfloat16), k, 1, 0, stride)
    return cols.transpose(1, 2).reshape(-1, cols.shape[1]).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds, three layers")
    ap.add_argument("--form", choices=["levels", "fused"], help="one input form only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_qconv_w8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    layers = [LAYERS[0], LAYERS[3], LAYERS[5]] if args.quick else LAYERS
    forms = [args.form] if args.form else ["levels", "fused"]
    gen = torch.Generator(device=dev).manual_seed(0)
    s_x = torch.tensor([S_X], device=dev)
    zx = torch.tensor([ZX], dtype=torch.int32, device=dev)
    sc, sh = torch.tensor([S_X], device=dev), torch.tensor([-S_X * ZX], device=dev)
    lines = ["# exp_qconv_w8_ab: the W8A8 conv2d on channels-last levels (liblsq_hip_qconv_w8.so) vs (a) F.pad + F.unfold of the levels + "
             "lsq_linear_w8_q8, (b) bfloat16 channels-last F.conv2d on the dequantized tensors; batch %d; %s, %d CUs"
             % (BATCH, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds of one captured graph per route, `calls` back-to-back calls over as many input sets "
             "(their levels: 1.25 x the 256 MB cache); spread = (max - min) / median of the new route's rounds; levels: uint8 "
             "levels in, bfloat16 y; fused: bfloat16 x in; route (a) includes its casts: F.unfold has no byte kernel, the padded "
             "levels go through bfloat16 and back" % rounds,
             "%-6s %-15s %5s %-13s | %9s %6s %7s | %9s %9s | %6s %6s | %s" % (
                 "form", "layer", "calls", "shape", "new us", "spread", "TOP/s", "(a) us", "(b) us", "new/a", "new/b", "new/a < 1")]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    spreads, misses = [], []
    for form in forms:
        for name, Cin, HW, N, k, stride, padding in layers:
            geo = ([stride, stride], [padding, padding], [1, 1])
            plan = E.qconv_w8_plan(BATCH, Cin, HW, HW, N, k, stride, padding)
            assert plan["form"] == "mfma"
            M, K = plan["M"], plan["K"]
            x_bytes = BATCH * Cin * HW * HW
            nsets = -(-CACHE_BYTES * 5 // 4 // x_bytes)            # the levels of the sets exceed the cache by a quarter ...
            iters = max(args.iters, nsets)                          # ... and one graph walks all of them
            lw = torch.randint(-128, 128, (N, Cin, k, k), dtype=torch.int8, device=dev, generator=gen).contiguous(memory_format=CL)
            s_w = torch.rand(N, device=dev, generator=gen) * 0.02 + 0.001
            zw = torch.randint(-9, 10, (N,), dtype=torch.int32, device=dev, generator=gen)
            wd = ((lw.float() - zw.reshape(-1, 1, 1, 1).float()) * s_w.reshape(-1, 1, 1, 1)).to(torch.bfloat16).contiguous(memory_format=CL)
            w2d = lw.contiguous().reshape(N, -1)                           # [N, (c, i, j)]: F.unfold's order of k
            xf = [(torch.randn(BATCH, Cin, HW, HW, device=dev, generator=gen) * 1.2 + 0.1).to(torch.bfloat16).contiguous(memory_format=CL)
                  for _ in range(nsets)]
            lx = [torch.ops.torchlsq.lsq_levels_per_tensor(x, sc, sh, 0, 255, 0, 255, 0).view(torch.uint8) for x in xf]
            xq = [((v.float() - ZX) * S_X).to(torch.bfloat16) for v in lx]             # x fake-quantized beforehand
            oh = (HW + 2 * padding - k) // stride + 1

            def as_image(y2d):
                return y2d.reshape(BATCH, oh, oh, N).permute(0, 3, 1, 2)

            if form == "levels":
                def new(i):
                    return torch.ops.torchlsq.lsq_conv2d_w8_q8(lx[i], s_x, zx, lw, s_w, zw, None, *geo, torch.bfloat16)

                def unfolded(i):
                    return as_image(torch.ops.torchlsq.lsq_linear_w8_q8(unfold_levels(lx[i], k, stride, padding), s_x, zx, w2d, s_w, zw,
                                                                        None, torch.bfloat16))

                def dense(i):
                    return F.conv2d(xq[i], wd, None, stride, padding)
            else:
                def new(i):
                    return torch.ops.torchlsq.lsq_conv2d_w8_a8(xf[i], sc, sh, 0, 255, 0, 255, lw, s_w, zw, None, *geo)

                def unfolded(i):
                    lv = torch.ops.torchlsq.lsq_levels_per_tensor(xf[i], sc, sh, 0, 255, 0, 255, 0).view(torch.uint8)
                    return as_image(torch.ops.torchlsq.lsq_linear_w8_q8(unfold_levels(lv, k, stride, padding), s_x, zx, w2d, s_w, zw,
                                                                        None, torch.bfloat16))

                def dense(i):
                    return F.conv2d(xf[i], wd, None, stride, padding)

            # the bits of the definition, of route (a) and repeatability before any timing
            y = new(0)
            assert torch.equal(y.view(torch.int16), new(0).view(torch.int16)), "two launches differ"
            I = F.conv2d(lx[0][:1].double() - ZX, lw.double() - zw.reshape(-1, 1, 1, 1).double(), None, stride, padding)   # exact
            want = ((s_w.reshape(1, -1, 1, 1) * I.float()) * s_x).to(torch.bfloat16)
            assert torch.equal(y[:1].contiguous().view(torch.int16), want.contiguous().view(torch.int16)), "not the bits of the definition"
            assert torch.equal(y.contiguous().view(torch.int16), unfolded(0).contiguous().view(torch.int16)), "route (a) has other bits"
            del I, want, y

            graphs = []
            for fn in (new, unfolded, dense):
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
            for _ in range(rounds + 1):                 # the first round warms up
                for j, g in enumerate(graphs):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    g.replay()
                    t1.record()
                    t1.synchronize()
                    times[j].append(t0.elapsed_time(t1) * 1e3 / iters)
            tn, ta, tb = (statistics.median(t[1:]) for t in times)
            spread = (max(times[0][1:]) - min(times[0][1:])) / tn
            spreads.append(spread)
            mark = "HIT" if tn / ta < 1.0 else "MISS"
            if mark == "MISS":
                misses.append("%s %s" % (form, name))
            line = "%-6s %-15s %5d %-13s | %9.1f %6.3f %7.1f | %9.1f %9.1f | %6.2f %6.2f | %s" % (
                form, name, iters, plan["shape"], tn, spread, 2.0 * M * N * K / (tn * 1e-6) / 1e12, ta, tb, tn / ta, tn / tb, mark)
            print(line, flush=True)
            lines.append(line)
            with open(args.out, "w") as f:              # kept current: a run that is cut short leaves what it measured
                f.write("\n".join(lines) + "\n")
            del graphs, xf, lx, xq
            torch.cuda.empty_cache()
    lines.append("# largest spread of the new route's rounds: %.3f" % max(spreads))
    lines.append("# expectation (new / (a) < 1.0 in every case): %s" % ("every case HIT" if not misses else "MISS: " + "; ".join(misses)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
