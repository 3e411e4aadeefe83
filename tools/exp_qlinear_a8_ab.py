#!/usr/bin/env python3
"""A/B: the 8-bit-activation linear op on packed weights (liblsq_hip_qlinear_a8.so, torch.ops.torchlsq.lsq_linear_packed_a8:
floating x in, levels formed in the kernel, integer MFMAs) against the two routes a converted model had before it, on the
same buffers.

    new  lsq_linear_packed_a8(x, scale, shift, range, codes, ...)      one launch: quantize x while staging, integer product
    (a)  lsq(x, scale, shift, ...) then lsq_linear_packed              what a converted model ran: the per-tensor fake-quantize
                                                                       launch, a 16-bit tensor of integer-valued levels, bf16 MFMAs
    (b)  lsq_linear_packed on an x fake-quantized beforehand           the matrix product of (a) alone

Per case (dtype x M x weight shape x G x bits): the new route's result is held to the accuracy bound of
include/lsq_hip_qlinear_a8.h against an int64 / float64 product on the device, compared bit for bit with the levels form on
lsq_levels_per_tensor's bytes and with a second launch; then each route is captured as ONE graph of ITERS back-to-back calls
over weight sets rotated so that the streamed working set exceeds the 256 MB Infinity Cache, and ROUNDS rounds alternate the
three graphs in one process, timed with HIP events.  Reported: the median microseconds per call of each route, the spread of
the new route's rounds ((max - min) / median), the new route's share of the 8 TB/s roofline at
N K bits / 8 + 8 N K / G + (M K + M N) sizeof(x) bytes, the form the plan reports, and the ratios new / (a) and new / (b).

    python tools/exp_qlinear_a8_ab.py [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008)]
GROUPS = [32, 128]
DTYPES = [torch.bfloat16, torch.float16]
BITS = [4, 2]
ROWS = [1, 4, 16]
ROOFLINE = 8.0e12
CACHE_BYTES = 256 << 20
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
QMIN, QMAX, TMIN, TMAX = 0, 127, 0, 255          # the module's default activation range: 7 bits in a quint8


def unpack(codes, bits):
    per = 8 // bits
    c = codes.to(torch.int32)
    return torch.stack([(c >> (j * bits)) & (2 ** bits - 1) for j in range(per)], dim=-1).reshape(codes.shape[0], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds and one weight shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_qlinear_a8_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    from torchlsq.functional import lsq
    a8 = torch.ops.torchlsq.lsq_linear_packed_a8
    q8 = torch.ops.torchlsq.lsq_linear_packed_q8
    op = torch.ops.torchlsq.lsq_linear_packed
    levels = torch.ops.torchlsq.lsq_levels_per_tensor
    dev = torch.device("cuda:0")
    rounds = 3 if args.quick else args.rounds
    shapes = SHAPES[:1] if args.quick else SHAPES
    gen = torch.Generator(device=dev).manual_seed(0)
    sc, sh = torch.tensor([0.03], device=dev), torch.tensor([-1.9], device=dev)        # zero point 63: levels centred in 0..127
    s_x = sc.abs().clamp_min(torch.finfo(torch.float32).eps)
    zx = torch.fmin(torch.full_like(s_x, TMAX), torch.fmax(torch.full_like(s_x, TMIN), -sh * (1.0 / s_x))).round().to(torch.int32)
    lines = ["# exp_qlinear_a8_ab: lsq_linear_packed_a8 (liblsq_hip_qlinear_a8.so, floating x in) vs (a) lsq + lsq_linear_packed and "
             "(b) lsq_linear_packed on an x fake-quantized beforehand; %s, %d CUs" % (
                 torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count),
             "# median of %d alternating rounds x %d back-to-back calls in one captured graph per route, weight sets rotated past "
             "the 256 MB cache; roofline 8 TB/s; spread = (max - min) / median of the new route's rounds" % (rounds, args.iters),
             "%-8s %2s %-12s %4s %4s %-7s | %8s %6s %5s | %8s %8s | %6s %6s" % ("dtype", "M", "weight", "G", "bits", "form", "new us",
                                                                              "spread", "roof", "(a) us", "(b) us", "new/a", "new/b")]
    print("\n".join(lines))
    for dtype in DTYPES:
        for (N, K) in shapes:
            for G in GROUPS:
                for bits in BITS:
                    esize = 2
                    code_bytes = N * K * bits // 8
                    nsets = min(args.iters, -(-CACHE_BYTES * 5 // 4 // code_bytes))
                    codes = [torch.randint(0, 256, (N, K * bits // 8), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nsets)]
                    qs = (torch.rand(N * K // G, device=dev, generator=gen) * 0.05 + 0.01)
                    qz = torch.randint(0, 2 ** bits, (N * K // G,), dtype=torch.int32, device=dev, generator=gen)
                    form = E.qlinear_a8_plan(1, N, K, G, bits)["form"]
                    for M in ROWS:
                        x = (torch.randn(M, K, device=dev, generator=gen) * 1.2).to(dtype)
                        xq = lsq(x, sc, sh, QMIN, QMAX, TMIN, TMAX)
                        # the bound and the bit-identities, before any timing
                        y = a8(x, sc, sh, QMIN, QMAX, TMIN, TMAX, codes[0], qs, qz, None, G, bits)
                        lv = levels(x, sc, sh, QMIN, QMAX, TMIN, TMAX, 0).view(torch.uint8)
                        a = (lv.to(torch.int64) - zx.to(torch.int64)).double().reshape(M, K // G, G)
                        cz = (unpack(codes[0], bits).reshape(N, K // G, G) - qz.reshape(N, K // G, 1)).double()
                        I = torch.einsum("mgk,ngk->mng", a, cz)
                        r = float(s_x) * (I * qs.double().reshape(N, K // G)).sum(-1)
                        S = float(s_x) * (I.abs() * qs.double().reshape(N, K // G)).sum(-1)
                        Eb = (K // G + 8) * 2.0 ** -24 * S
                        bound = Eb + U[dtype] * (r.abs() + Eb) + (2.0 ** -24 if dtype == torch.float16 else 0.0)
                        worst = float(((y.double() - r).abs() / bound).max())
                        assert worst <= 1.0, "new route outside the bound: %.3f" % worst
                        assert torch.equal(y, q8(lv, s_x, zx, codes[0], qs, qz, None, G, bits, dtype)), "fused != levels form"
                        assert torch.equal(y, a8(x, sc, sh, QMIN, QMAX, TMIN, TMAX, codes[0], qs, qz, None, G, bits)), "two launches differ"
                        del a, cz, I, r, S, Eb, bound

                        def run_new():
                            for i in range(args.iters):
                                a8(x, sc, sh, QMIN, QMAX, TMIN, TMAX, codes[i % nsets], qs, qz, None, G, bits)

                        def run_a():
                            for i in range(args.iters):
                                op(lsq(x, sc, sh, QMIN, QMAX, TMIN, TMAX), codes[i % nsets], qs, qz, None, G, bits)

                        def run_b():
                            for i in range(args.iters):
                                op(xq, codes[i % nsets], qs, qz, None, G, bits)

                        graphs = []
                        with torch.no_grad():
                            for fn in (run_new, run_a, run_b):
                                side = torch.cuda.Stream()
                                side.wait_stream(torch.cuda.current_stream())
                                with torch.cuda.stream(side):
                                    fn()
                                torch.cuda.current_stream().wait_stream(side)
                                g = torch.cuda.CUDAGraph()
                                with torch.cuda.graph(g):
                                    fn()
                                graphs.append(g)
                        times = [[], [], []]
                        for _ in range(rounds + 1):                 # the first round warms up
                            for k, g in enumerate(graphs):
                                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                t0.record()
                                g.replay()
                                t1.record()
                                t1.synchronize()
                                times[k].append(t0.elapsed_time(t1) * 1e3 / args.iters)
                        new, ta, tb = (statistics.median(t[1:]) for t in times)
                        spread = (max(times[0][1:]) - min(times[0][1:])) / new
                        algo = N * K * bits / 8.0 + 8.0 * N * K / G + (M * K + M * N) * esize
                        line = "%-8s %2d %-12s %4d %4d %-7s | %8.1f %6.3f %5.2f | %8.1f %8.1f | %6.2f %6.2f" % (
                            str(dtype).replace("torch.", ""), M, "%dx%d" % (N, K), G, bits, form, new, spread,
                            algo / ROOFLINE / (new * 1e-6), ta, tb, new / ta, new / tb)
                        print(line, flush=True)
                        lines.append(line)
                        del graphs
                    del codes
                    torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
