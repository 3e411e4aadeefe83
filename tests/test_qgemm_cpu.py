"""CPU: the matrix-core GEMM on packed group-wise weights (include/lsq_hip_qgemm.h, liblsq_hip_qgemm.so), the route of
torchlsq.functional.lsq_linear_packed for more than 16 rows of bfloat16 / float16 x, without a GPU.

  * the library exports exactly what its header declares, ABI 1, imports nothing of the five other HIP libraries and reads
    no environment;
  * its kernels: one family per (16-bit dtype x bits), no scratch, no atomics, 16-byte code loads, mfma_f32_16x16x32;
  * argument validation and the launch plan, host only: what is served, what is not and why, the grids, the LDS.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from helpers import demangle, gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip_qgemm.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_qgemm.so")
NAMES = sorted(["lsq_qgemm_abi_version", "lsq_qgemm_last_error", "lsq_qgemm_forward", "lsq_qgemm_plan"])
LSQ_EINVAL = -1


def test_qgemm_library_exports_what_its_header_declares():
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_\w+)\s*\(", text)))
    assert declared == NAMES and sorted(E.C_ABI_QGEMM) == NAMES
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    assert exported == NAMES
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    for other in ("getenv", "lsq_hip_", "lsq_group_", "lsq_pack_", "lsq_qlinear"):
        assert other not in und and (other == "getenv" or other not in nm), other
    assert E.qgemm_library().lsq_qgemm_abi_version() == E.QGEMM_ABI_VERSION == 1
    assert re.search(r"#define LSQ_QGEMM_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == "1"
    # the other libraries' symbol tables know nothing of it
    others = list(E.C_ABI) + list(E.C_ABI_GROUP) + list(E.C_ABI_PACK) + list(E.C_ABI_CPU) + list(E.C_ABI_QLINEAR) + list(E.C_ABI_QLINEAR_A8)
    assert not [n for n in others if "qgemm" in n]
    assert E.qgemm_plan is not None and E.qgemm_forward is not None


def test_qgemm_kernels(tmp_path):
    """one kernel family per (16-bit dtype x bits) -- the tile shapes of each are its members --, none for float32; no
    scratch, no atomics, the code stream in 16-byte packets, x from LDS in 16-byte reads, mfma_f32_16x16x32"""
    every = gfx950_kernels(LIB, str(tmp_path))
    names = demangle(sorted(every))
    families = {}
    for sym, dm in names.items():
        m = re.match(r"^void lsq::qgemm_kernel<lsq::io_(bf16|f16), (?:\(int\))?([24]), (?:\(int\))?([14]), (?:\(int\))?([248])>\(", dm)
        assert m, "not a GEMM kernel: %s" % dm
        families.setdefault((m.group(1), int(m.group(2))), set()).add((int(m.group(3)), int(m.group(4))))
    assert sorted(families) == [("bf16", 2), ("bf16", 4), ("f16", 2), ("f16", 4)]
    # each family: 64- and 16-column tiles, each computing 8, 4 or 2 sub-tiles of 16 rows
    assert all(members == {(w, s) for w in (1, 4) for s in (2, 4, 8)} for members in families.values()), families
    for name, (body, scratch) in every.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0 and not [o for o in ops if o.startswith("scratch_")], "%s uses %d bytes of scratch" % (name, scratch)
        assert not [o for o in ops if "atomic" in o], name
        assert "global_load_dwordx4" in ops and "ds_read_b128" in ops, name
        mfma = [o for o in ops if o.startswith("v_mfma")]
        assert mfma and all(o.startswith("v_mfma_f32_16x16x32") for o in mfma), name
        assert "v_permlane32_swap_b32_e32" in ops and "v_permlane16_swap_b32_e32" in ops, name


def test_argument_validation_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qgemm_library()
    ok = 1 << 20

    def fwd(code=E.LSQ_BF16, x=ok, M=17, codes=ok, N=8, K=256, G=32, bits=4, qs=ok, qz=ok, bias=None, bd=E.LSQ_F32, y=ok):
        return lib.lsq_qgemm_forward(code, x, M, codes, N, K, G, bits, qs, qz, bias, bd, y, None)

    def err():
        return lib.lsq_qgemm_last_error()

    assert fwd(bits=3) == LSQ_EINVAL and b"bits must be 4 or 2" in err()
    assert fwd(bits=8) == LSQ_EINVAL and b"bits" in err()
    assert fwd(G=0) == LSQ_EINVAL and b"group_size" in err()
    assert fwd(K=250) == LSQ_EINVAL and b"multiple of group_size" in err()
    assert fwd(K=255, G=1) == LSQ_EINVAL and b"one byte" in err()                 # G % (8 / bits) != 0
    assert fwd(K=258, G=2, bits=2) == LSQ_EINVAL and b"one byte" in err()
    assert fwd(M=0) == LSQ_EINVAL and b"rows of x" in err()
    assert fwd(M=-3) == LSQ_EINVAL and b"rows of x" in err()
    assert fwd(M=1 << 62) == LSQ_EINVAL and b"64-bit offsets" in err()
    assert fwd(M=1 << 40, N=1 << 20) == LSQ_EINVAL and b"31-bit grid" in err()
    assert fwd(N=-1) == LSQ_EINVAL and b"negative" in err()
    assert fwd(code=7) == LSQ_EINVAL and b"dtype" in err()
    assert fwd(code=E.LSQ_F64) == LSQ_EINVAL and b"float64" in err()
    for null in ("x", "codes", "qs", "qz", "y"):
        assert fwd(**{null: None}) == LSQ_EINVAL and b"NULL" in err(), null
    assert fwd(x=ok + 1) == LSQ_EINVAL and b"element-aligned" in err()
    assert fwd(qz=ok + 2) == LSQ_EINVAL and b"element-aligned" in err()
    assert fwd(bias=ok, bd=E.LSQ_F16) == LSQ_EINVAL and b"bias" in err()           # neither float32 nor x's type
    assert fwd(bias=ok + 2, bd=E.LSQ_F32) == LSQ_EINVAL and b"element-aligned" in err()
    assert fwd(N=0) == 0                                                           # nothing to do, nothing launched
    # formats that are not served: LSQ_EINVAL with the reason, nothing launched
    assert fwd(code=E.LSQ_F32) == LSQ_EINVAL and b"not served" in err() and b"float32" in err()
    assert fwd(G=32, bits=2) == LSQ_EINVAL and b"not served" in err() and b"16-byte code packet" in err()
    assert fwd(code=E.LSQ_F16, K=64, G=8) == LSQ_EINVAL and b"not served" in err() and b"16-byte code packet" in err()
    assert fwd(codes=ok + 1) == LSQ_EINVAL and b"not served" in err() and b"16-byte aligned" in err()


def test_plan_without_a_gpu():
    from torchlsq import extension as E
    lib = E.qgemm_library()
    out = (ctypes.c_int32 * 8)()
    assert lib.lsq_qgemm_plan(E.LSQ_BF16, 17, 64, 250, 32, 4, ctypes.byref(out)) == LSQ_EINVAL
    assert b"multiple of group_size" in lib.lsq_qgemm_last_error()
    assert lib.lsq_qgemm_plan(E.LSQ_BF16, 17, 64, 256, 32, 4, None) == LSQ_EINVAL and b"NULL" in lib.lsq_qgemm_last_error()
    assert lib.lsq_qgemm_plan(E.LSQ_BF16, 0, 64, 256, 32, 4, ctypes.byref(out)) == LSQ_EINVAL
    for dtype, G, bits, form in ((torch.bfloat16, 32, 4, "mfma"), (torch.float16, 96, 4, "mfma"), (torch.bfloat16, 128, 2, "mfma"),
                                 (torch.float16, 128, 4, "mfma"), (torch.float32, 128, 4, "unserved"), (torch.float32, 32, 4, "unserved"),
                                 (torch.float32, 128, 2, "unserved"), (torch.bfloat16, 32, 2, "unserved"), (torch.float16, 8, 4, "unserved")):
        for M in (1, 17, 64, 65, 2048):
            K = 4800 if G == 96 else 4096
            pl = E.qgemm_plan(dtype, M, 4096, K, G, bits)
            assert pl["form"] == form, (dtype, G, bits, M, pl)
            if form == "unserved":
                assert not any(v for k, v in pl.items() if k != "form"), pl
                continue
            step = 4 * 128 // bits
            assert pl["rows_per_tile"] == 128 and pl["k_per_step"] == step and pl["block"] == 4 * pl["cols_per_tile"]
            assert pl["cols_per_tile"] in (16, 64)
            tiles = -(-M // 128) * -(-4096 // pl["cols_per_tile"])
            # one workgroup per tile, and at least one tile for each of the 256 compute units at a Llama-size N
            assert pl["grid"] == tiles >= 256, pl
            subs = 2 if M <= 32 else 4 if M <= 64 else 8
            assert pl["lds_bytes"] == subs * 16 * (2 * step + 16) <= 160 * 1024, pl
    # 16-column tiles while 64-column tiles would leave compute units without one (256 are assumed without a device)
    assert E.qgemm_plan(torch.bfloat16, 17, 4096, 4096, 128, 4)["cols_per_tile"] == 16
    assert E.qgemm_plan(torch.bfloat16, 17, 4096, 4096, 128, 4)["grid"] == 256
    assert E.qgemm_plan(torch.bfloat16, 2048, 4096, 4096, 128, 4)["cols_per_tile"] == 64
    assert E.qgemm_plan(torch.bfloat16, 2048, 4096, 4096, 128, 4)["grid"] == 16 * 64
    assert E.qgemm_plan(torch.bfloat16, 17, 17, 96, 32, 4)["grid"] == 2
    assert E.qgemm_plan(torch.bfloat16, 127 * 128 + 1, 67, 96, 32, 4)["cols_per_tile"] == 64
    assert E.qgemm_plan(torch.bfloat16, 127 * 128, 67, 96, 32, 4)["cols_per_tile"] == 16
    # the decode library is as it was: 17 rows are refused there
    with pytest.raises(RuntimeError, match="serves 1 to 16"):
        E.qlinear_plan(torch.bfloat16, 17, 64, 256, 32, 4)
