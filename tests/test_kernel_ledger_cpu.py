"""No GPU: the bookkeeping of a kernel ledger -- which per-channel kernel instantiations the library ships, by name.  The
tools build records the kernels it launches (tools/lsq_tools.py: launched_reset / launched), so a GPU sweep can say which of
the shipped instantiations its oracle-checked cases ran; this file pins what that comparison stands on.  Every
per-channel kernel symbol of the built liblsq_hip.so reads as coordinates (helpers.per_channel_kernels: family, storage type,
V, CPL, modes, the other template arguments, workgroup size), no two symbols share coordinates, the exemption file names
only kernels that exist, and the tools build -- whose launches the ledger records -- contains every per-channel kernel of
the production build under the same symbol."""
import json
import os

import pytest

from helpers import PC_FAMILIES, demangle, gfx950_kernels, parse_pc_kernel, pc_coordinates, per_channel_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROD_LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip.so")
TOOLS_LIB = os.path.join(ROOT, "tools", "_tune", "liblsq_hip_tools.so")
EXEMPT = os.path.join(ROOT, "tests", "golden", "kernel_ledger_exempt.json")


@pytest.fixture(scope="module")
def shipped(tmp_path_factory):
    return per_channel_kernels(PROD_LIB, str(tmp_path_factory.mktemp("prod")))


def test_every_per_channel_kernel_parses(shipped, tmp_path):
    # (per_channel_kernels raises on a per-channel name it cannot read; here: nothing per-channel slipped past its filter)
    every = demangle(sorted(gfx950_kernels(PROD_LIB, str(tmp_path))))
    named = {s for s, d in every.items() if any(f in d for f in PC_FAMILIES)}
    assert named == set(shipped)
    by_family = {}
    for r in shipped.values():
        by_family.setdefault(r["family"], []).append(r)
    assert set(by_family) == {f[:-len("_kernel")] for f in PC_FAMILIES}, sorted(by_family)
    for r in shipped.values():
        if r["family"].startswith("finalize"):
            assert r["storage"] in ("float", "double") and r["V"] is None
        else:
            assert r["storage"] in ("f32", "f64", "bf16", "f16")
            assert r["V"] in (1, {"f32": 4, "f64": 2, "bf16": 8, "f16": 8}[r["storage"]]), pc_coordinates(r)
            assert r["CPL"] in (1, 2, r["V"]) and r["block"] in (256, 512, 768, 1024), pc_coordinates(r)
            assert not (r["modes"].get("EVAL") and r["modes"].get("SYM")), pc_coordinates(r)      # (with_bwd_modes)


def test_a_name_that_does_not_parse_is_an_error():
    for bad in ("void lsq::bwd_pc_kernel<lsq::io_f32, 4, 1, false>(void const*)",                  # too few arguments
                "void lsq::fwd_seg_kernel<lsq::io_f8, 4, false, false, 4, true, true, 1>(void const*)",   # unknown storage
                "void lsq::fwd_seg_kernel<lsq::io_f32, 4, 0, false, 4, true, true, 1>(void const*)",      # a number for a flag
                "void lsq::other_kernel<float>(int)"):
        with pytest.raises(ValueError):
            parse_pc_kernel("_Zbad", bad)


def test_both_demanglers_spellings_read_alike():
    plain = "void lsq::bwd_pc_kernel<lsq::io_bf16, 8, 2, true, false, false, 1, true, true, false, true, 4, 768>(void const*)"
    cast = ("void lsq::bwd_pc_kernel<lsq::io_bf16, (int)8, (int)2, (bool)1, (bool)0, (bool)0, (int)1, (bool)1, (bool)1, (bool)0, "
            "(bool)1, (int)4, (int)768>(void const*)")
    a, b = parse_pc_kernel("_Zk", plain), parse_pc_kernel("_Zk", cast)
    assert a == b and a["modes"] == {"SYM": True, "INIT": False, "EVAL": False} and (a["V"], a["CPL"], a["block"]) == (8, 2, 768)
    assert a["rest"] == {"UNROLL": 1, "NTL": True, "NTS": True, "PIPE": False, "WW": True, "DMA": 4}
    with pytest.raises(ValueError):
        parse_pc_kernel("_Zk", plain.replace("true, false, false, 1", "(bool)2, false, false, 1"))


def test_parsed_records_are_unique(shipped):
    seen = {}
    for sym, r in shipped.items():
        key = (r["family"], r["storage"], r["V"], r["CPL"], tuple(sorted(r["modes"].items())), tuple(sorted(r["rest"].items())), r["block"])
        assert key not in seen, "%s and %s both read as %s" % (sym, seen[key], pc_coordinates(r))
        seen[key] = sym


def test_exemptions_name_shipped_kernels(shipped):
    with open(EXEMPT) as f:
        doc = json.load(f)
    symbols = [e["symbol"] for e in doc["exempt"]]
    assert len(symbols) == len(set(symbols))
    for e in doc["exempt"]:
        assert e["symbol"] in shipped, "exempt, but not in liblsq_hip.so: %s" % e["symbol"]
        assert e["kernel"] == pc_coordinates(shipped[e["symbol"]]), e
        assert len(e["condition"]) > 20 and ("lsq_pc_plan.hpp" in e["condition"] or "lsq_pc_geom.hpp" in e["condition"]), e


def test_tools_build_contains_the_production_kernels(shipped, tmp_path):
    assert os.path.isfile(TOOLS_LIB), "the tools build is missing: make -C lsqfakequantize-pytorch_amd/csrc tools"
    tools = per_channel_kernels(TOOLS_LIB, str(tmp_path))
    missing = sorted(pc_coordinates(shipped[s]) for s in shipped if s not in tools)
    assert not missing, "per-channel kernels of liblsq_hip.so that the tools build does not have:\n  " + "\n  ".join(missing)
