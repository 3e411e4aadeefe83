"""CPU: design rules checked on the gfx950 machine code that actually ships in liblsq_hip.so.

The device code objects are pulled out of the library's .hip_fatbin section and disassembled with the ROCm LLVM
tools (no GPU needed):
  * no v_fma_mix* -- hipcc likes to select "fp16 -> fp32, multiply, -> fp16" as a mixed-precision FMA with a +0
    addend, which loses the sign of a zero product (IO::to_elem in csrc/lsq_math.hpp prevents it);
  * no scratch (register spills / runtime-indexed private arrays) in any kernel;
  * FMA contraction is off: v_fma_f32 / v_fmac_f32 only inside the IEEE division expansion (and the explicit fp64
    fma of the statistics kernels);
  * the streaming kernels move 16-byte packets.
"""
import os
import re

import pytest

from helpers import gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip.so")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel symbol: (disassembly text, metadata dict)} for every gfx950 kernel in the library."""
    out = gfx950_kernels(LIB, str(tmp_path_factory.mktemp("devcode")))
    assert len(out) > 100, "expected the whole kernel table, found %d kernels" % len(out)
    return out


def _ops(body):
    return re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)


def test_no_mixed_precision_fma_and_no_scratch(kernels):
    for name, (body, scratch) in kernels.items():
        ops = _ops(body)
        assert not [o for o in ops if o.startswith("v_fma_mix") or o.startswith("v_mad_mix")], name
        assert scratch == 0 and not [o for o in ops if o.startswith("scratch_")], "%s uses %d bytes of scratch" % (name, scratch)


def test_fp_contraction_is_off(kernels):
    """x*inv_s + zp must round twice, like the reference's x86-64 build: the only fp32/fp64 FMAs allowed in the
    fake-quantize kernels are those of the correctly rounded division expansion (v_div_fmas / v_div_fixup around them)."""
    checked = 0
    for name, (body, _) in kernels.items():
        if not re.search(r"(fwd|bwd)_(pt|pc|seg|mask)_", name):      # the fake-quantize kernels proper
            continue
        ops = _ops(body)
        n_fma = sum(1 for o in ops if re.fullmatch(r"v_(fma|fmac|mad|mac)_f(32|64)(_e32|_e64)?", o))
        n_div = sum(1 for o in ops if o.startswith("v_div_fmas_f"))
        assert n_fma <= 5 * n_div, "%s: %d FMAs for %d divisions (5 per division expected)" % (name, n_fma, n_div)
        checked += 1
    assert checked > 100


def test_streaming_kernels_move_16_byte_packets(kernels):
    picked = [n for n in kernels if re.search(r"(fwd_pt_kernel|bwd_pt_kernel|fwd_pc_kernel|bwd_pc_kernel|fwd_seg_kernel|bwd_seg_kernel)"
                                              r"INS_(6io_f32|7io_bf16|6io_f16|6io_f64)ELi(4|8|2)", n)]
    assert len(picked) > 20
    rings = 0
    for name in picked:
        ops = _ops(kernels[name][0])
        # 16-byte packets in: ordinary loads, or the LDS-DMA ring's global -> LDS copies read back with ds_read_b128
        if "global_load_lds_dwordx4" in ops:
            rings += 1
            assert "ds_read_b128" in ops and "global_store_dwordx4" in ops, name
        else:
            assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops, name
    assert rings > 10       # the window-mode per-channel kernels ship with their LDS-DMA variants
