"""CPU: the int8 matrix-core GEMM on packed group-wise weights (include/lsq_hip_qgemm_a8.h, liblsq_hip_qgemm_a8.so), the route
of lsq_linear_packed_q8 / lsq_linear_packed_a8 for more rows than the decode kernel serves, without a GPU.

  * the library exports exactly what its header declares, ABI 1, imports nothing of the six other HIP libraries and reads no
    environment; the decode library still refuses 17 rows;
  * its kernels: the GEMM at 2 bits, at 4 bits with one and with two packets per MFMA, each in 64- and 16-column tiles of 2,
    4 and 8 sub-tiles, and the pre-pass of the fused form per type of x; integer MFMAs, no scratch, no atomics;
  * the plan: served exactly where the decode plan says "mfma", the tile shapes, the grids, the LDS;
  * argument validation, host only: nothing is launched;
  * the kernel's walk over K, replayed on the host: every code packet once, in the order of the contract.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import qlinear_a8_cases as A
from helpers import demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_qgemm_a8.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_qgemm_a8.so")
NAMES = sorted(["lsq_qgemm_a8_abi_version", "lsq_qgemm_a8_last_error", "lsq_qgemm_a8_forward_levels", "lsq_qgemm_a8_forward",
                "lsq_qgemm_a8_plan"])
LSQ_EINVAL = -1
# (N, K, G, bits): 3 spans, 13 empty chains; 3 packets per group, two chunks, the last ragged; a partial span; 2 bits, every
# chain one span; two packets per MFMA, three chunks, chains of several spans
FORMATS = [(67, 384, 128, 4), (33, 4800, 96, 4), (17, 96, 32, 4), (5, 4096, 128, 2), (21, 8320, 64, 4)]


def test_qgemm_a8_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_\w+)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_QGEMM_A8) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear", "lsq_qgemm_forward", "lsq_qgemm_plan"):
        assert other not in und and (other == "getenv" or other not in nm), other
    assert E.qgemm_a8_library().lsq_qgemm_a8_abi_version() == E.QGEMM_A8_ABI_VERSION == 1
    assert re.search(r"#define LSQ_QGEMM_A8_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    # the other libraries' symbol tables know nothing of it
    others = (list(E.C_ABI) + list(E.C_ABI_GROUP) + list(E.C_ABI_PACK) + list(E.C_ABI_CPU) + list(E.C_ABI_QLINEAR) +
              list(E.C_ABI_QLINEAR_A8) + list(E.C_ABI_QGEMM))
    assert not [n for n in others if "qgemm_a8" in n]
    assert E.qgemm_a8_plan is not None and E.qgemm_a8_forward is not None and E.qgemm_a8_forward_levels is not None
    assert E.qgemm_a8_min_rows() > E.QLINEAR_A8_MAX_ROWS == 16
    # the decode library is as it was: 17 rows are refused there
    with pytest.raises(RuntimeError, match="serves 1 to 16"):
        E.qlinear_a8_plan(17, 64, 256, 32, 4)


def test_qgemm_a8_kernels(tmp_path):
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    gemm, levels = set(), set()
    for sym, dm in names.items():
        m = re.match(r"^void lsq::qgemm_a8_kernel<(?:\(int\))?([24]), (?:\(bool\))?(true|false|0|1), (?:\(int\))?([14]), (?:\(int\))?([248])>\(", dm)
        if m:
            gemm.add((int(m.group(1)), m.group(2) in ("true", "1"), int(m.group(3)), int(m.group(4))))
            continue
        m = re.match(r"^void lsq::qgemm_a8_levels_kernel<lsq::io_(bf16|f16|f32)>\(", dm)
        assert m, "neither the GEMM nor its pre-pass: %s" % dm
        levels.add(m.group(1))
    assert gemm == {(b, p, w, s) for b, p in ((2, False), (4, False), (4, True)) for w in (1, 4) for s in (2, 4, 8)}
    assert levels == {"bf16", "f16", "f32"}
    for sym, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0 and not [o for o in ops if o.startswith("scratch_")], "%s uses %d bytes of scratch" % (sym, scratch)
        assert not [o for o in ops if "atomic" in o], sym
        if "levels_kernel" in names[sym]:
            assert "global_store_dwordx4" in ops and not [o for o in ops if o.startswith("v_mfma")], sym
            continue
        mfma = [o for o in ops if o.startswith("v_mfma")]
        assert mfma and all(o == "v_mfma_i32_16x16x64_i8" for o in mfma), sym
        assert "global_load_dwordx4" in ops and "ds_read_b128" in ops, sym
        assert "v_permlane32_swap_b32_e32" in ops and "v_permlane16_swap_b32_e32" in ops, sym


def test_plan_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qgemm_a8_library()
    out = (ctypes.c_int32 * 8)()
    assert lib.lsq_qgemm_a8_plan(17, 64, 250, 32, 4, ctypes.byref(out)) == LSQ_EINVAL
    assert b"multiple of group_size" in lib.lsq_qgemm_a8_last_error()
    assert lib.lsq_qgemm_a8_plan(17, 64, 256, 32, 4, None) == LSQ_EINVAL and b"NULL" in lib.lsq_qgemm_a8_last_error()
    assert lib.lsq_qgemm_a8_plan(0, 64, 256, 32, 4, ctypes.byref(out)) == LSQ_EINVAL
    # the eligibility table of the decode kernel's two forms (tests/test_qlinear_a8_cpu.py): form for form the same
    for G, bits, form in ((32, 4, "mfma"), (128, 4, "mfma"), (96, 4, "mfma"), (128, 2, "mfma"), (64, 2, "mfma"), (1024, 4, "mfma"),
                          (32, 2, "unserved"), (8, 4, "unserved"), (2, 4, "unserved"), (8192, 4, "unserved")):
        K = {96: 4800, 8192: 8192}.get(G, 4096)
        decode = E.qlinear_a8_plan(16, 4096, K, G, bits)["form"]
        assert (decode == "mfma") == (form == "mfma"), (G, bits, decode)
        for M in (1, 17, 32, 33, 64, 65, 2048):
            pl = E.qgemm_a8_plan(M, 4096, K, G, bits)
            assert pl["form"] == form, (G, bits, M, pl)
            if form == "unserved":
                assert not any(v for k, v in pl.items() if k != "form"), pl
                continue
            subs = 2 if M <= 32 else 4 if M <= 64 else 8
            step = 4 * 128 // bits
            assert pl["subs"] == subs and pl["rows_per_tile"] == 16 * subs and pl["k_per_step"] == step
            assert pl["cols_per_tile"] in (16, 64) and pl["block"] == 4 * pl["cols_per_tile"]
            tiles = -(-M // (16 * subs)) * -(-4096 // pl["cols_per_tile"])
            assert pl["grid"] == tiles >= 256, pl
            # x of one step, one byte per element, rows 16 bytes apart, and the 4 byte sums per row
            assert pl["lds_bytes"] == 16 * subs * (step + 16) + 16 * subs * 16 <= 64 * 1024, pl
    for shape in A.SHAPES:          # every decode test shape's form
        M, N, K, G, bits = shape
        assert (E.qgemm_a8_plan(*shape)["form"] == "mfma") == (E.qlinear_a8_plan(*shape)["form"] == "mfma"), shape
    for N, K, G, bits in FORMATS:
        assert E.qgemm_a8_plan(129, N, K, G, bits)["form"] == "mfma"
    # 16-column tiles while 64-column tiles would leave compute units without one (256 are assumed without a device)
    assert E.qgemm_a8_plan(17, 4096, 4096, 128, 4)["cols_per_tile"] == 16 and E.qgemm_a8_plan(17, 4096, 4096, 128, 4)["grid"] == 256
    assert E.qgemm_a8_plan(2048, 4096, 4096, 128, 4)["cols_per_tile"] == 64
    assert E.qgemm_a8_plan(2048, 4096, 4096, 128, 4)["grid"] == 16 * 64
    assert E.qgemm_a8_plan(127 * 128 + 1, 67, 96, 32, 4)["cols_per_tile"] == 64
    assert E.qgemm_a8_plan(127 * 128, 67, 96, 32, 4)["cols_per_tile"] == 16


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qgemm_a8_library()
    ok = 1 << 20

    def lv(ld=E.LSQ_A8_U8, x=ok, M=17, s=ok, z=ok, codes=ok, N=8, K=256, G=32, bits=4, qs=ok, qz=ok, bias=None, bd=E.LSQ_F32, y=ok,
           yd=E.LSQ_BF16):
        return lib.lsq_qgemm_a8_forward_levels(ld, x, M, s, z, codes, N, K, G, bits, qs, qz, bias, bd, y, yd, None)

    def fu(code=E.LSQ_BF16, x=ok, M=17, s=ok, b=ok, r=(0, 255, 0, 255), codes=ok, N=8, K=256, G=32, bits=4, qs=ok, qz=ok, bias=None,
           bd=E.LSQ_F32, y=ok, ws=ok):
        return lib.lsq_qgemm_a8_forward(code, x, M, s, b, r[0], r[1], r[2], r[3], codes, N, K, G, bits, qs, qz, bias, bd, y, ws, None)

    def err():
        return lib.lsq_qgemm_a8_last_error()

    for f in (lv, fu):
        assert f(bits=3) == LSQ_EINVAL and b"bits must be 4 or 2" in err()
        assert f(G=0) == LSQ_EINVAL and b"group_size" in err()
        assert f(K=250) == LSQ_EINVAL and b"multiple of group_size" in err()
        assert f(K=255, G=1) == LSQ_EINVAL and b"one byte" in err()
        assert f(M=0) == LSQ_EINVAL and b"rows of x" in err()
        assert f(M=-3) == LSQ_EINVAL and b"rows of x" in err()
        assert f(M=1 << 62) == LSQ_EINVAL and b"64-bit offsets" in err()
        assert f(M=1 << 40, N=1 << 20) == LSQ_EINVAL and b"31-bit grid" in err()
        assert f(N=-1) == LSQ_EINVAL and b"negative" in err()
        for null in ("x", "codes", "qs", "qz", "y", "s"):
            assert f(**{null: None}) == LSQ_EINVAL and b"NULL" in err(), null
        assert f(qz=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(bias=ok, bd=E.LSQ_F16) == LSQ_EINVAL and b"bias" in err()
        assert f(bias=ok + 2, bd=E.LSQ_F32) == LSQ_EINVAL and b"element-aligned" in err()
        assert f(N=0) == 0                                                 # nothing to do, nothing launched
        # what the decode plan calls generic is not served: LSQ_EINVAL with the reason, nothing launched
        assert f(G=32, bits=2) == LSQ_EINVAL and b"not served" in err() and b"16-byte code packet" in err()
        assert f(K=64, G=8) == LSQ_EINVAL and b"not served" in err() and b"16-byte code packet" in err()
        assert f(K=8192, G=8192) == LSQ_EINVAL and b"not served" in err() and b"4096" in err()
        assert f(codes=ok + 1) == LSQ_EINVAL and b"not served" in err() and b"16-byte aligned" in err()
    assert lv(ld=2) == LSQ_EINVAL and b"level_dtype" in err()
    assert lv(yd=E.LSQ_F64) == LSQ_EINVAL and b"float64" in err()
    assert lv(yd=9) == LSQ_EINVAL and b"dtype" in err()
    assert lv(z=None) == LSQ_EINVAL and b"NULL" in err()
    assert lv(s=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
    assert fu(code=E.LSQ_F64) == LSQ_EINVAL and b"float64" in err()
    assert fu(x=ok + 1) == LSQ_EINVAL and b"element-aligned" in err()
    assert fu(b=None) == LSQ_EINVAL and b"NULL" in err()
    assert fu(ws=None) == LSQ_EINVAL and b"levels_ws" in err()
    assert fu(ws=ok + 8) == LSQ_EINVAL and b"levels_ws" in err()
    for r in ((-1, 255, 0, 255), (0, 256, 0, 256), (-128, 127, 0, 255), (5, 4, 0, 255), (-129, 127, -129, 127)):
        assert fu(r=r) == LSQ_EINVAL and b"0..255 or within -128..127" in err(), r


# ------------------------------------------------------------------------------------------------
# the walk over K
# ------------------------------------------------------------------------------------------------
def _cut(K, G, bits):
    """(packet elements, packets per group, packets per span, spans per chunk, packets) as plan_a8 / plan_g8 cut K"""
    be = 128 // bits
    ppg = G // be
    span_p = ppg if ppg % 4 == 0 else ppg * 2 if ppg % 2 == 0 else ppg * 4
    return be, ppg, span_p, 4096 // (span_p * be), K // be


def kernel_walk(K, G, bits):
    """[(chain, first packet, packets)] of the load steps in the order the kernel takes them: G8Walk / g8_settle / g8_advance
    of csrc/qgemm_a8/lsq_qgemm_a8.hip, statement for statement"""
    be, ppg, span_p, chunk_spans, n_packets = _cut(K, G, bits)
    chunk_p = chunk_spans * span_p
    n_chunks = -(-n_packets // chunk_p)
    steps_per_span = span_p // 4
    w, c, span, l = 0, 0, 0, 0
    out = []
    while True:
        # g8_settle
        p0 = None
        while True:
            if w >= 16:
                break
            if c >= n_chunks:
                w, c, l = w + 1, 0, 0
                span = w
                continue
            if span < chunk_spans:
                p = c * chunk_p + span * span_p + l * 4
                if p < n_packets:
                    p0 = p
                    break
            c, span, l = c + 1, w, 0
        if p0 is None:
            return out
        out.append((w, p0, min(4, n_packets - p0)))
        # g8_advance
        l += 1
        if l == steps_per_span:
            l, span = 0, span + 16
    return out


def contract_order(K, G, bits):
    """[(chain, group)] as include/lsq_hip_qgemm_a8.h orders one output's sum: chains 0..15, for a chain the chunks ascending,
    in a chunk the spans s = w mod 16 ascending, in a span the groups ascending"""
    be, ppg, span_p, chunk_spans, n_packets = _cut(K, G, bits)
    groups_per_span = span_p // ppg
    spans = -(-n_packets // span_p)
    out = []
    for w in range(16):
        for c in range(-(-spans // chunk_spans)):
            for s in range(w, chunk_spans, 16):
                for g in range(groups_per_span):
                    group = (c * chunk_spans + s) * groups_per_span + g
                    if c * chunk_spans + s < spans and group < K // G:
                        out.append((w, group))
    return out


@pytest.mark.parametrize("fmt", FORMATS + [(8, 4096, 32, 4), (8, 1024, 1024, 4), (8, 11008, 128, 4), (8, 128, 64, 2)],
                         ids=lambda v: "x".join(map(str, v)))
def test_the_walk_over_k_takes_every_packet_once_in_the_contract_order(fmt):
    from torchlsq import extension as E
    _, K, G, bits = fmt
    be, ppg, span_p, chunk_spans, n_packets = _cut(K, G, bits)
    # the cut is the decode plan's: its chunk is chunk_spans whole spans
    assert E.qlinear_a8_plan(1, 16, K, G, bits)["chunk"] == chunk_spans * span_p * be
    steps = kernel_walk(K, G, bits)
    packets = [(w, p) for w, p0, n in steps for p in range(p0, p0 + n)]
    assert sorted(p for _, p in packets) == list(range(n_packets))             # every packet exactly once
    # the groups complete in the order of the contract, each from ppg consecutive packets of one chain
    groups = []
    for i in range(0, len(packets), ppg):
        run = packets[i:i + ppg]
        assert len({w for w, _ in run}) == 1 and [p for _, p in run] == list(range(run[0][1], run[0][1] + ppg)), run
        assert run[0][1] % ppg == 0
        groups.append((run[0][0], run[0][1] // ppg))
    assert groups == contract_order(K, G, bits)
    assert [w for w, _ in groups] == sorted(w for w, _ in groups)              # chain by chain
    # ... which is the decode kernel's: span s of a chunk belongs to wave s % 16
    for w, g in groups:
        span = g * ppg // span_p
        assert (span % chunk_spans) % 16 == w
