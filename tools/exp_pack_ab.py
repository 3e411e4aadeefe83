#!/usr/bin/env python3
"""A/B: the packed export kernels (liblsq_hip_pack.so) against the routes a user had before them.

    lsq_pack_quantize    vs  lsq_group_forward with levels only (y == NULL): one byte per element, lsq_levels_per_group
    lsq_pack_dequantize  vs  lsq_group_forward: the fake-quantized weight from the fp master weight, lsq_forward_per_group

All four are driven through their C entry points with preallocated outputs, so the host time of the Python layers stays out
of the numbers.  Per case (weight shape x storage x G x bits): warm-up, then ROUNDS rounds that alternate the two routes in
one process; a round is ITERS back-to-back launches on input sets rotated so that the streamed working set exceeds the 256 MB
Infinity Cache (reads come from HBM, as in bench.py), timed with HIP events.  Reported: the median microseconds per launch of
each route, the spread of the new route's rounds ((max - min) / median), the share of the 8 TB/s roofline for the
algorithmic bytes -- per element, E = element bytes: quantize E + bits / 8 + 16 / G (scale, shift, qscale, qzero) against
E + 1 + 8 / G; dequantize E + bits / 8 + 8 / G against 2 E + 8 / G -- and the ratio new / old.  The codes the dequantize
reads are rotated too, over as many sets as exceed the cache on their own, so its reads are as cold as the forward's.
Before timing, the codes are compared with the packing of the old route's levels, and the dequantized values with the old
route's y, bit for bit.

    python tools/exp_pack_ab.py [--quick] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008), (8192, 4096)]
GROUPS = [32, 128]
DTYPES = [torch.float32, torch.bfloat16]
BITS = [4, 2]
RANGE = {4: (-8, 7), 2: (-2, 1)}
ROOFLINE = 8.0e12
CACHE_BYTES = 256 << 20


def algorithmic_bytes(n, G, elem_bytes, bits, op, new):
    """bytes the op has to move: the streams, plus the per-group arrays (fp32 scale / shift in, fp32 + int32 constants out)"""
    if op == "quantize":
        return n * (elem_bytes + (bits / 8.0 + 16.0 / G if new else 1.0 + 8.0 / G))
    return n * (elem_bytes + (bits / 8.0 if new else elem_bytes) + 8.0 / G)


def torch_pack(levels, qmin, bits):
    per = 8 // bits
    c = (levels.reshape(-1, per).to(torch.int32) - qmin)
    out = torch.zeros_like(c[:, 0])
    for j in range(per):
        out |= c[:, j] << (j * bits)
    return out.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_pack_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    rounds = 3 if a.quick else a.rounds
    iters = 10 if a.quick else a.iters

    from torchlsq import extension as E
    from torchlsq._abi import _DTYPE_CODE
    glib, plib = E.group_library(), E.pack_library()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    say("# exp_pack_ab: packed export (liblsq_hip_pack.so) vs lsq_group_forward of liblsq_hip_group.so (quantize: levels only, y == NULL; dequantize: y); %s, %d CUs" %
        (props.name, props.multi_processor_count))
    say("# median of %d alternating rounds x %d back-to-back launches, inputs and code sets rotated past the 256 MB cache; roofline %.0f TB/s; spread = (max - min) / "
        "median of the new route's rounds" % (rounds, iters, ROOFLINE / 1e12))
    say("%-8s %-12s %4s %4s %-10s | %9s %6s %5s | %9s %5s | %7s" %
        ("dtype", "shape", "G", "bits", "op", "new us", "spread", "roof", "old us", "roof", "new/old"))
    worst = {"quantize": 0.0, "dequantize": 0.0}
    for dtype in DTYPES:
        code = _DTYPE_CODE[dtype]
        esz = torch.tensor([], dtype=dtype).element_size()
        for shape in SHAPES:
            n = shape[0] * shape[1]
            sets = max(2, -(-3 * CACHE_BYTES // (2 * n * esz)))
            gen = torch.Generator(device=dev).manual_seed(0)
            xs = [(torch.randn(shape, generator=gen, device=dev) * 0.02).to(dtype) for _ in range(sets)]
            levels = torch.empty(shape, dtype=torch.int8, device=dev)
            y, y2 = torch.empty_like(xs[0]), torch.empty_like(xs[0])
            for G in GROUPS:
                C = n // G
                s = torch.rand(C, generator=gen, device=dev) * 0.004 + 0.001
                b = torch.zeros(C, device=dev)
                qs, qz = torch.empty(C, device=dev), torch.empty(C, dtype=torch.int32, device=dev)
                for bits in BITS:
                    qmin, qmax = RANGE[bits]
                    p = E.LsqParams(qmin, qmax, -128, 127, 1, 1, 0, 0, 1.0, 0)
                    pref = ctypes.byref(p)
                    ex = E.LsqFwdExtras(levels.data_ptr(), 0, 0)
                    exref = ctypes.byref(ex)
                    # the dequantize reads rotate over code sets that exceed the cache on their own, as the forward's x does
                    csets = max(sets, -(-3 * CACHE_BYTES // (2 * (n * bits // 8))))
                    codes = [torch.empty(n * bits // 8, dtype=torch.uint8, device=dev) for _ in range(csets)]

                    def q_new(i):
                        return plib.lsq_pack_quantize(code, xs[i % sets].data_ptr(), n, G, s.data_ptr(), b.data_ptr(), pref, bits,
                                                      codes[i % csets].data_ptr(), qs.data_ptr(), qz.data_ptr(), stream)

                    def q_old(i):
                        return glib.lsq_group_forward(code, xs[i % sets].data_ptr(), None, n, G, s.data_ptr(), b.data_ptr(), pref, exref,
                                                      stream)

                    def d_new(i):
                        return plib.lsq_pack_dequantize(code, codes[i % csets].data_ptr(), n, G, bits, qs.data_ptr(), qz.data_ptr(),
                                                        y.data_ptr(), stream)

                    def d_old(i):
                        return glib.lsq_group_forward(code, xs[i % sets].data_ptr(), y2.data_ptr(), n, G, s.data_ptr(), b.data_ptr(), pref,
                                                      None, stream)

                    for i in range(csets):           # every code set holds real codes (set i: those of input set i % sets)
                        assert q_new(i) == 0
                    for f in (q_old, d_new, d_old):
                        assert f(0) == 0, f.__name__
                    torch.cuda.synchronize()
                    assert torch.equal(codes[0], torch_pack(levels, qmin, bits)), "codes differ (%s %s G=%d %d-bit)" % (dtype, shape, G, bits)
                    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), "y differs (%s %s G=%d %d-bit)" % (dtype, shape, G, bits)
                    for op, new, old in (("quantize", q_new, q_old), ("dequantize", d_new, d_old)):
                        for f in (new, old):
                            for i in range(3):
                                f(i)
                        times = {new: [], old: []}
                        k = 0
                        for _ in range(rounds):
                            for f in (new, old):
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                e0.record()
                                for _ in range(iters):
                                    f(k)
                                    k += 1
                                e1.record()
                                e1.synchronize()
                                times[f].append(e0.elapsed_time(e1) * 1e3 / iters)
                        tn, to = statistics.median(times[new]), statistics.median(times[old])
                        spread = (max(times[new]) - min(times[new])) / tn
                        worst[op] = max(worst[op], tn / to)
                        say("%-8s %-12s %4d %4d %-10s | %9.1f %6.3f %5.2f | %9.1f %5.2f | %7.2f" %
                            (str(dtype).replace("torch.", ""), "%dx%d" % shape, G, bits, op, tn, spread,
                             algorithmic_bytes(n, G, esz, bits, op, True) / (tn * 1e-6) / ROOFLINE, to,
                             algorithmic_bytes(n, G, esz, bits, op, False) / (to * 1e-6) / ROOFLINE, tn / to))
                    del codes
            del xs
            torch.cuda.empty_cache()
    say("# worst new/old: quantize %.2f, dequantize %.2f" % (worst["quantize"], worst["dequantize"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
