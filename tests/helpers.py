"""Shared helpers of the tests: bitwise and reduction comparisons, and the gfx950 kernels of a built library."""
import hashlib
import os
import re
import subprocess

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


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


LLVM = "/opt/rocm/lib/llvm/bin"


def gfx950_kernels(lib, tmp):
    """{kernel symbol: (disassembly text, private segment bytes)} for every gfx950 kernel of the shared library `lib`: its
    code objects are pulled out of the .hip_fatbin section, unbundled and disassembled with the ROCm LLVM tools (no GPU
    needed) in the directory `tmp`.  Skips the calling test when the tools are missing."""
    for tool in ("clang-offload-bundler", "llvm-objdump", "llvm-readelf"):
        if not os.path.isfile(os.path.join(LLVM, tool)):
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
