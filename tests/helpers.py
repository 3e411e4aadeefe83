"""Shared helpers of the tests: bitwise and reduction comparisons, and the gfx950 kernels of a built library."""
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

TOL = 1e-6   # north_star: dequantized output and gradients within 1e-6 relative of the reference CPU path


def bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_bits_equal(got, want, what):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want).reshape(got.shape)
    if got.tobytes() != want.tobytes():
        gi = got.view(np.uint8).reshape(got.size, -1)
        wi = want.view(np.uint8).reshape(want.size, -1)
        bad = np.nonzero((gi != wi).any(axis=1))[0]
        raise AssertionError("%s: %d of %d elements differ bitwise; first at %d: got %r want %r" %
                             (what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


def assert_reduction_close(got, want, abs_terms, what, tol=TOL):
    """|got - want| <= tol * sum|terms| (== tol * |want| when the terms do not cancel); NaN == NaN."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    want = np.asarray(want, dtype=np.float64).reshape(-1)
    scale = np.maximum(np.asarray(abs_terms, dtype=np.float64).reshape(-1), 1e-300)
    ok = (np.abs(got - want) <= tol * scale) | (got == want) | (np.isnan(got) & np.isnan(want))
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        raise AssertionError("%s: element %d got %.12g want %.12g (|diff| %.3g, allowed %.3g)" %
                             (what, i, got[i], want[i], abs(got[i] - want[i]), tol * scale[i]))


def same_stored(got, want, dtype, what):
    """a result of the GPU (a tensor) against the oracle's (an array), bit for bit.  16-bit storage: the oracle's fp32 result
    rounded to the storage type; rounding does not say which of the storage type's NaNs an fp32 NaN becomes (the payload cannot
    be kept), so where the oracle has a NaN the result must be a NaN, and every other element must have the rounded value's
    bits."""
    import torch
    if dtype in (torch.float32, torch.float64):
        return assert_bits_equal(got.cpu().numpy(), want, what)
    want = torch.from_numpy(np.ascontiguousarray(want)).reshape(got.shape)
    nan = torch.isnan(want)
    got = got.cpu()
    assert torch.equal(torch.isnan(got), nan), what + ": NaNs are not where the oracle's are"
    assert_bits_equal(got.masked_fill(nan, 0).view(torch.int16).numpy(), want.to(dtype).masked_fill(nan, 0).view(torch.int16).numpy(), what)


def check_sums(got, wide, abs_terms, what):
    """d_scale / d_shift (a tensor) against the oracle's fp64 sums: the oracle's NaN / +-inf pattern exactly -- which shows that a
    non-finite term stayed with its own channel or group -- and assert_reduction_close on the finite ones"""
    got, wide = got.cpu().numpy().astype(np.float64).reshape(-1), np.asarray(wide, dtype=np.float64).reshape(-1)
    bad = ~np.isfinite(wide)
    assert (np.isfinite(got) == ~bad).all(), "%s: non-finite channels got %r want %r" % (what, got, wide)
    assert (np.isnan(got) == np.isnan(wide)).all(), "%s: NaN channels got %r want %r" % (what, got, wide)
    inf = np.isinf(wide)
    assert (got[inf] == wide[inf]).all(), "%s: inf signs got %r want %r" % (what, got, wide)
    assert_reduction_close(got[~bad], wide[~bad], np.asarray(abs_terms).reshape(-1)[~bad], what + " (finite channels)")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


LLVM = "/opt/rocm/lib/llvm/bin"


def gfx950_kernels(lib, tmp, missing_tool="skip"):
    """{kernel symbol: (disassembly text, private segment bytes)} for every gfx950 kernel of the shared library `lib`: its
    code objects are pulled out of the .hip_fatbin section, unbundled and disassembled with the ROCm LLVM tools (no GPU
    needed) in the directory `tmp`.  Skips the calling test when the tools are missing (missing_tool="error": raises)."""
    for tool in ("clang-offload-bundler", "llvm-objdump", "llvm-readelf"):
        if not os.path.isfile(os.path.join(LLVM, tool)):
            if missing_tool == "error":
                raise RuntimeError("ROCm LLVM tool %s not found in %s" % (tool, LLVM))
            pytest.skip("ROCm LLVM tool %s not found" % tool)
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    assert starts, "no offload bundle in %s" % os.path.basename(lib)
    out = {}
    for i, s in enumerate(starts):
        part = os.path.join(tmp, "bundle%d.bin" % i)
        with open(part, "wb") as f:
            f.write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        co = os.path.join(tmp, "dev%d.co" % i)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        meta = {m.group(1): int(m.group(2)) for m in
                re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", notes, re.S)}
        for m in re.finditer(r"^[0-9a-f]+ <(\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", asm, re.S | re.M):
            if m.group(1) in meta:
                out[m.group(1)] = (m.group(2), meta[m.group(1)])
    return out


def demangle(names):
    """{mangled: demangled} with llvm-cxxfilt of the ROCm LLVM directory (binutils' c++filt where that LLVM ships without
    it: parse_pc_kernel reads both demanglers' spellings of a template argument); an error when there is neither"""
    names = list(names)
    tool = os.path.join(LLVM, "llvm-cxxfilt")
    if not os.path.isfile(tool):
        tool = shutil.which("c++filt")
    if not tool:
        raise RuntimeError("no demangler: neither %s/llvm-cxxfilt nor c++filt" % LLVM)
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    if len(out) != len(names):
        raise RuntimeError("%s answered %d lines for %d names" % (tool, len(out), len(names)))
    return dict(zip(names, out))


# the per-channel kernels (csrc/lsq_pc_fwd.hpp, lsq_pc_bwd.hpp, lsq_pc_seg.hpp, lsq_pc_finalize.hpp) and their template
# parameters after the storage type, in declaration order
PC_FAMILIES = {
    "fwd_pc_kernel": ("V", "CPL", "INIT", "LEVELS", "UNROLL", "NTL", "NTS", "DMA"),
    "fwd_seg_kernel": ("V", "INIT", "LEVELS", "UNROLL", "NTL", "NTS", "WALK"),
    "bwd_pc_kernel": ("V", "CPL", "SYM", "INIT", "EVAL", "UNROLL", "NTL", "NTS", "PIPE", "WW", "DMA", "BLOCK"),
    "bwd_seg_kernel": ("V", "SYM", "INIT", "EVAL", "UNROLL", "NTL", "NTS", "WALK"),
    "finalize_pc_kernel": (), "finalize_ww_kernel": (), "finalize_seg_kernel": (),
}
_PC_MODES = ("SYM", "INIT", "EVAL", "LEVELS")
_PC_STORAGE = {"lsq::io_f32": "f32", "lsq::io_f64": "f64", "lsq::io_bf16": "bf16", "lsq::io_f16": "f16", "float": "float", "double": "double"}


def parse_pc_kernel(symbol, demangled):
    """One per-channel kernel symbol as its coordinates: family, storage type (the finalizes: their arithmetic type), V, CPL
    (segment kernels: one channel per workgroup, CPL 1), the mode flags, the remaining template arguments and the workgroup
    size.  A name that does not read as one of PC_FAMILIES' instantiations is an error."""
    m = re.match(r"^void lsq::(\w+)<([^<>]*)>\(", demangled)
    if not m or m.group(1) not in PC_FAMILIES:
        raise ValueError("not a per-channel kernel instantiation: %s (%s)" % (demangled, symbol))
    family, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    names = PC_FAMILIES[family]
    if len(args) != 1 + len(names) or args[0] not in _PC_STORAGE:
        raise ValueError("%s: template arguments %r do not fit <storage, %s>" % (family, args, ", ".join(names)))
    vals = {}
    for name, a in zip(names, args[1:]):
        # (older binutils demanglers write a cast in front of a literal: (bool)1, (int)4)
        cast = re.fullmatch(r"\((bool|int)\)(-?\d+)", a)
        if cast:
            a = cast.group(2) if cast.group(1) == "int" else {"0": "false", "1": "true"}.get(cast.group(2), a)
        if a in ("true", "false"):
            vals[name] = a == "true"
        elif re.fullmatch(r"-?\d+", a):
            vals[name] = int(a)
        else:
            raise ValueError("%s: template argument %s = %r is neither a number nor a flag" % (family, name, a))
    for name in names:
        flag = name in _PC_MODES or name in ("NTL", "NTS", "PIPE", "WW")
        if isinstance(vals[name], bool) != flag:
            raise ValueError("%s: template argument %s = %r has the wrong kind" % (family, name, vals[name]))
    rec = {"symbol": symbol, "family": family[:-len("_kernel")], "storage": _PC_STORAGE[args[0]],
           "V": vals.pop("V", None), "CPL": vals.pop("CPL", 1 if names else None),
           "modes": {k: vals.pop(k) for k in _PC_MODES if k in vals},
           "block": vals.pop("BLOCK", 256)}
    rec["rest"] = vals
    return rec


def pc_coordinates(rec):
    """a record of parse_pc_kernel on one line"""
    modes = "".join(" " + k.lower() for k, v in sorted(rec["modes"].items()) if v) or " plain"
    rest = " ".join("%s=%s" % (k, int(v) if isinstance(v, bool) else v) for k, v in sorted(rec["rest"].items()))
    if rec["V"] is None:
        return "%s<%s>" % (rec["family"], rec["storage"])
    return "%s %s V=%d CPL=%d%s | %s | block %d" % (rec["family"], rec["storage"], rec["V"], rec["CPL"], modes, rest, rec["block"])


def per_channel_kernels(lib, tmp=None):
    """{kernel symbol: record of parse_pc_kernel} for the per-channel kernels -- forward / backward window and segment kernels
    and the three finalizes -- among the gfx950 kernels of the built library `lib` (gfx950_kernels: no GPU needed)."""
    own = tmp is None
    if own:
        tmp = tempfile.mkdtemp(prefix="lsq_pc_kernels_")
    try:
        symbols = sorted(gfx950_kernels(lib, tmp, missing_tool="error"))      # (a ledger that skips says nothing)
    finally:
        if own:
            shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for sym, dm in demangle(symbols).items():
        m = re.match(r"^(?:void )?lsq::(\w+)", dm)
        if m and m.group(1) in PC_FAMILIES:
            out[sym] = parse_pc_kernel(sym, dm)
    return out
