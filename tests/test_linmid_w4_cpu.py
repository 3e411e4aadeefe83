"""liblsq_hip_linmid_w4.so (include/lsq_hip_linmid_w4.h) without a GPU: its plan, and the CPU path at its row counts against the
plain float64-step reference of tests/test_lindec_w4_cpu.py -- the reference the GPU tests hold the kernel to."""
import pytest
import torch

import test_lindec_w4_cpu as C
from torchlsq import extension as E

# (M, N, K, G, bits) of tests/test_linmid_w4_gpu.py: one row in the second sub-tile, one span | full tile, 17 spans, N % 16 != 0 | two
# chunks, four groups per span | span = lcm(3, 4) packets, no PAIR | a group over two steps | crumbs, windows of half a step | windows
# of ONE place of a paired step (64 groups per chunk fill the table).  Each crossed with lindec's variant list.
SHAPES = [(17, 16, 128, 128, 4), (64, 40, 2176, 128, 4), (33, 32, 4224, 32, 4), (48, 16, 768, 96, 4), (40, 16, 512, 256, 4),
          (64, 16, 512, 128, 2), (64, 48, 4096, 64, 4)]
CASES = [s + v for s in SHAPES for v in C.VARIANTS]


@pytest.mark.parametrize("args, want", [
    ((17, 4096, 4096, 128, 4), dict(served=True, subs=2, grid=256, block=512, stages=1, store="packets", res_load="packets")),
    ((33, 4096, 4096, 128, 4), dict(served=True, subs=3, stages=1)),
    ((64, 4096, 4096, 128, 4), dict(served=True, subs=4, grid=256, stages=2)),        # 64 rows of 4096 k are 256 KB
    ((64, 4096, 4096, 128, 2), dict(served=True, subs=4, stages=2)),
    ((64, 40, 2176, 128, 4), dict(served=True, grid=3, store="bytes", res_load="bytes")),
    ((64, 16, 512, 128, 2), dict(served=True, stages=2)),                             # windows of 2 of a step's 4 places
    ((64, 48, 4096, 64, 4), dict(served=True, stages=4)),                             # windows of 1 of a paired step's 2 places
    ((40, 16, 512, 256, 4, True, False, True), dict(served=True, subs=3, store="bytes", res_load="packets")),
    ((16, 4096, 4096, 128, 4), dict(served=False, grid=0, block=0, lds_bytes=0)),
    ((65, 4096, 4096, 128, 4), dict(served=False)),
    ((20, 64, 128, 32, 2), dict(served=False)),
    ((20, 64, 128, 128, 4, False), dict(served=False)),
])
def test_plan(args, want):
    pl = E.linmid_w4_plan(*args)
    assert {k: pl[k] for k in want} == want and pl["lds_bytes"] <= 160 * 1024, pl


@pytest.mark.parametrize("spec", [CASES[0], CASES[8 + 6]], ids=C.ident)
def test_cpu_ops_equal_the_plain_reference(spec):
    c = C.case(*spec)
    for decode in (True, False, None):
        got = C.run(c, decode=decode)
        assert got.dtype == c["want"].dtype and torch.equal(got, c["want"])
