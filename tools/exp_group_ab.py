#!/usr/bin/env python3
"""A/B: the group-wise kernels (liblsq_hip_group.so) against the reshape route through the per-channel op.

The reshape route is what a user had before the group ops: lsq(x.reshape(-1, G), s.reshape(-1), b.reshape(-1), axis=0,
is_perchannel=True), i.e. lsq_hip_forward_per_channel / lsq_hip_backward_per_channel on [outer = 1, C = N / G, inner = G]
(the backward with its workspace and finalize launch).  Both are driven through their C entry points with preallocated
outputs, so the host time of the Python layers stays out of the numbers.

Per case (weight shape x storage x G): warm-up, then ROUNDS rounds that alternate the two routes in one process; a round
is ITERS back-to-back launches on input sets rotated so that the streamed working set exceeds the 256 MB Infinity Cache
(reads come from HBM, as in bench.py), timed with HIP events.  Reported: the median microseconds per launch, GElem/s and the
share of the 8 TB/s roofline for the algorithmic bytes -- per fp32 element forward 8 + 8/G, backward 12 + 16/G (16-bit
storage: half the element bytes).  Before timing, both routes' y and dx are compared bit for bit.

    python tools/exp_group_ab.py [--quick] [--out FILE]
Kernel times: the same run under `rocprofv3 --kernel-trace --stats -- python tools/exp_group_ab.py --quick`
(tools/README.md).
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))

import torch  # noqa: E402

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008), (14336, 4096), (8192, 4096)]
GROUPS = [32, 64, 128, 256]
DTYPES = [torch.float32, torch.bfloat16]
ROOFLINE = 8.0e12
CACHE_BYTES = 256 << 20


def algorithmic_bytes(n, G, elem_bytes, direction):
    # fp32: fwd 8 + 8/G, bwd 12 + 16/G per element; the parameters are fp32 for every storage type
    if direction == "fwd":
        return n * (2 * elem_bytes + 8.0 / G)
    return n * (3 * elem_bytes + 16.0 / G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rounds (the rocprofv3 run)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    rounds = 3 if a.quick else a.rounds
    iters = 10 if a.quick else a.iters

    from torchlsq import extension as E
    from torchlsq._abi import _DTYPE_CODE
    lib, glib = E.library(), E.group_library()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    say("# exp_group_ab: group kernels vs the reshape route (per-channel op on [1, N/G, G]); %s, %d CUs" %
        (props.name, props.multi_processor_count))
    say("# median of %d alternating rounds x %d back-to-back launches, rotated inputs; roofline %.0f TB/s" %
        (rounds, iters, ROOFLINE / 1e12))
    say("%-8s %-12s %4s %4s | %9s %7s %5s | %9s %7s %5s | %6s" %
        ("dtype", "shape", "G", "dir", "new us", "GEl/s", "roof", "reshape", "GEl/s", "roof", "new/rs"))
    p = E.LsqParams(-8, 7, -128, 127, 1, 1, 0, 0, 1.0, 0)     # W4 symmetric
    pref = ctypes.byref(p)
    for dtype in DTYPES:
        code = _DTYPE_CODE[dtype]
        esz = torch.tensor([], dtype=dtype).element_size()
        for shape in SHAPES:
            n = shape[0] * shape[1]
            sets = max(2, -(-3 * CACHE_BYTES // (2 * n * esz)))
            gen = torch.Generator(device=dev).manual_seed(0)
            xs = [(torch.randn(shape, generator=gen, device=dev) * 0.02).to(dtype) for _ in range(sets)]
            gs = [torch.randn(shape, generator=gen, device=dev).to(dtype) for _ in range(sets)]
            y, y2 = torch.empty_like(xs[0]), torch.empty_like(xs[0])
            dx, dx2 = torch.empty_like(xs[0]), torch.empty_like(xs[0])
            for G in GROUPS:
                C = n // G
                s = torch.rand(C, generator=gen, device=dev) * 0.004 + 0.001
                b = torch.zeros(C, device=dev)
                ds, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
                wsb = int(lib.lsq_hip_backward_per_channel_workspace(code, 1, C, G))
                ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)

                def fwd_new(i):
                    return glib.lsq_group_forward(code, xs[i].data_ptr(), y.data_ptr(), n, G, s.data_ptr(), b.data_ptr(), pref,
                                                  None, stream)

                def fwd_ref(i):
                    return lib.lsq_hip_forward_per_channel(code, xs[i].data_ptr(), y2.data_ptr(), 1, C, G, s.data_ptr(),
                                                           b.data_ptr(), pref, None, stream)

                def bwd_new(i):
                    return glib.lsq_group_backward(code, gs[i].data_ptr(), xs[i].data_ptr(), dx.data_ptr(), ds.data_ptr(),
                                                   db.data_ptr(), n, G, s.data_ptr(), b.data_ptr(), pref, stream)

                def bwd_ref(i):
                    return lib.lsq_hip_backward_per_channel(code, gs[i].data_ptr(), xs[i].data_ptr(), dx2.data_ptr(),
                                                            ds.data_ptr(), db.data_ptr(), None, 1, C, G, s.data_ptr(),
                                                            b.data_ptr(), pref, None, ws.data_ptr(), ws.numel(), stream)

                for f in (fwd_new, fwd_ref, bwd_new, bwd_ref):
                    assert f(0) == 0, f.__name__
                torch.cuda.synchronize()
                assert torch.equal(y, y2) and torch.equal(dx, dx2), "routes disagree (%s %s G=%d)" % (dtype, shape, G)
                for direction, new, ref in (("fwd", fwd_new, fwd_ref), ("bwd", bwd_new, bwd_ref)):
                    for f in (new, ref):
                        for i in range(3):
                            f(i % sets)
                    times = {new: [], ref: []}
                    k = 0
                    for _ in range(rounds):
                        for f in (new, ref):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(iters):
                                f(k % sets)
                                k += 1
                            e1.record()
                            e1.synchronize()
                            times[f].append(e0.elapsed_time(e1) * 1e3 / iters)
                    tn, tr = statistics.median(times[new]), statistics.median(times[ref])
                    nb = algorithmic_bytes(n, G, esz, direction)
                    say("%-8s %-12s %4d %4s | %9.1f %7.0f %5.2f | %9.1f %7.0f %5.2f | %6.2f" %
                        (str(dtype).replace("torch.", ""), "%dx%d" % shape, G, direction, tn, n / tn / 1e3,
                         nb / (tn * 1e-6) / ROOFLINE, tr, n / tr / 1e3, nb / (tr * 1e-6) / ROOFLINE, tn / tr))
            del xs, gs
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
