#!/usr/bin/env python3
"""Pin what two tests used to ask the reference's own builds at run time, so that they need nothing outside the repository.

Run where the reference's builds exist (oracle/build_ref.py made oracle/_ref/):

    python tests/golden/make_ref_pinned.py

What is written (data only -- the reference's outputs on seeded inputs):
    tests/golden/ref_scalar_digests.json   sha256 of the reference's scalar header (oracle/_ref/liblsq_ref_scalar.so) on the inputs of
                                           tests/test_oracle_pinned.py::test_oracle_bitwise_vs_reference_scalar_header
    tests/golden/soak_reference.json/.npz  the reference's CPU ops (oracle/_ref/libtorchlsq_ref_ops.so) on the first SOAK_CASES cases of
                                           tools/soak_parity.py --seed SOAK_SEED --extreme SOAK_EXTREME: y / dx by sha256, d_scale /
                                           d_shift whole (tools/soak_parity.py --against pinned, tests/test_reference_soak_gpu.py)
No GPU is needed: the inputs are drawn on the host and the reference runs on the CPU.
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

SOAK_SEED, SOAK_EXTREME, SOAK_CASES = 7, 0.15, 24


def scalar_digests():
    import test_oracle_pinned as T
    from helpers import sha
    ref = ctypes.CDLL(T._REF_SCALAR)
    out = {}
    for dtype, key in ((np.float32, "f32"), (np.float64, "f64")):
        want = T.ref_scalar_outputs(ref, dtype)
        got = T.oracle_scalar_outputs(dtype)
        for label in want:          # a drift of the oracle is caught here, not pinned
            assert sha(got[label]) == sha(want[label]), (key, label)
        out[key] = {label: sha(a) for label, a in want.items()}
    with open(os.path.join(HERE, "ref_scalar_digests.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def soak_reference():
    import soak_parity as S
    from helpers import sha
    S.EXTREME[0] = SOAK_EXTREME
    cases, arrays = {}, {}
    for case in range(SOAK_CASES):
        d = S.draw_lsq_case(np.random.default_rng([SOAK_SEED, case]), True)
        ry, rdx, rds, rdb = S.ref_call(d["xs"], d["gsh"], d["scale"], d["shift"], S.ref_args(d))
        cases[str(case)] = {"tag": d["tag"], "y_sha256": sha(ry), "dx_sha256": sha(rdx)}
        arrays["c%d_ds" % case], arrays["c%d_db" % case] = rds, rdb
        print(case, d["tag"], flush=True)
    S.REF[0].stdin.close()
    S.REF[0].wait(timeout=60)
    base = os.path.join(HERE, "soak_reference")
    with open(base + ".json", "w") as f:
        json.dump({"seed": SOAK_SEED, "extreme": SOAK_EXTREME, "cases": cases,
                   "reference": "the reference's CPU ops (oracle/_ref/libtorchlsq_ref_ops.so)"}, f, indent=1)
        f.write("\n")
    np.savez_compressed(base + ".npz", **arrays)


if __name__ == "__main__":
    scalar_digests()
    soak_reference()
