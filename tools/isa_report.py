#!/usr/bin/env python3
"""Compile the kernel translation units to gfx950 assembly and report, per kernel: VGPR/SGPR
counts, scratch bytes, LDS bytes, and a few instruction counts that encode the design rules
(no fp contraction outside the IEEE division sequence, 16-byte global accesses, no scratch).

usage: python tools/isa_report.py [substring-filter]
       python tools/isa_report.py --diff OLD.so NEW.so [substring-filter]

--diff compares two BUILT libraries kernel by kernel (tests/helpers.gfx950_kernels: no GPU needed): the set of kernel
symbols; per kernel the VGPR / SGPR / LDS / scratch figures of the code-object notes and the instruction stream without
the address column and the branch-target annotations.  Every differing kernel is printed with its hunks, and each hunk
says whether it lies inside a LOOP (between a backward branch and its target).  Exit status 0: no kernel differs,
1: differences in straight-line code only (same symbols, same figures, same instruction counts, loops identical),
2: anything else.
"""
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "csrc")
FLAGS = ["-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
         "--cuda-device-only", "-S"]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), text=True,
                         capture_output=True).stdout.splitlines()
    return dict(zip(names, out))


def _kernels_of(lib, tmp):
    """{symbol: (instructions, loop flags, figures)} of every gfx950 kernel in the shared library `lib`"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    for tool in ("clang-offload-bundler", "llvm-objdump", "llvm-readelf"):      # (helpers would skip a test: say it here)
        if not os.path.isfile(os.path.join(helpers.LLVM, tool)):
            sys.exit("isa_report.py --diff: ROCm LLVM tool %s not found in %s" % (tool, helpers.LLVM))
    os.makedirs(tmp)
    kernels = helpers.gfx950_kernels(lib, tmp)
    figures = {}
    for co in sorted(f for f in os.listdir(tmp) if f.endswith(".co")):
        notes = subprocess.run([os.path.join(helpers.LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, co)],
                               capture_output=True, text=True, check=True).stdout
        # a kernel's record lists its keys in alphabetical order; `.symbol` (NAME.kd) is the kernel's own, no argument has one
        for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+)"
                             r".*?\.symbol:\s+(\S+?)\.kd.*?\.vgpr_count:\s+(\d+)", notes, re.S):
            figures[m.group(4)] = (int(m.group(5)), int(m.group(3)), int(m.group(1)), int(m.group(2)))
    out = {}
    for name, (text, _) in kernels.items():
        ins, addr = [], []
        for m in re.finditer(r"^\s+(\S[^\n]*?)\s*// ([0-9A-Fa-f]+):", text, re.M):
            ins.append(re.sub(r"\s+", " ", m.group(1)))
            addr.append(int(m.group(2), 16))
        in_loop = [False] * len(ins)
        for i, t in enumerate(ins):       # a backward branch closes a loop: [target, branch]
            m = re.fullmatch(r"s_c?branch\w* (\d+)", t)
            if m and int(m.group(1)) >= 0x8000:
                target = addr[i] + 4 + 4 * (int(m.group(1)) - 0x10000)
                for k in range(i, -1, -1):
                    if addr[k] < target:
                        break
                    in_loop[k] = True
        out[name] = (ins, in_loop, figures[name])
    return out


def diff_main(old, new, filt):
    tmp = tempfile.mkdtemp(prefix="lsq_isa_diff_")
    try:
        a, b = _kernels_of(old, os.path.join(tmp, "old")), _kernels_of(new, os.path.join(tmp, "new"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    dm = demangle(sorted(set(a) | set(b)))
    short = lambda n: re.sub(r"\(.*", "", dm[n]).replace("lsq::", "").replace("void ", "")
    worst = 0
    for n in sorted(set(a) ^ set(b), key=short):
        if filt not in short(n):
            continue
        print("%s only: %s" % ("OLD" if n in a else "NEW", short(n)))
        worst = 2
    same = differing = 0
    for n in sorted(set(a) & set(b), key=short):
        if filt not in short(n):
            continue
        (ia, la, fa), (ib, lb, fb) = a[n], b[n]
        if ia == ib and fa == fb:
            same += 1
            continue
        differing += 1
        level = 1 if fa == fb and len(ia) == len(ib) else 2
        print("DIFFERS %s\n  vgpr/sgpr/lds/scratch %s -> %s, instructions %d -> %d" % (short(n), fa, fb, len(ia), len(ib)))
        for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, ia, ib, autojunk=False).get_opcodes():
            if tag == "equal":
                continue
            loop = any(la[i1:i2]) or any(lb[j1:j2])
            if loop:
                level = 2
            print("  @@ old %d-%d, new %d-%d: %s" % (i1, i2, j1, j2, "INSIDE A LOOP" if loop else "straight-line code"))
            for t in ia[i1:i2]:
                print("    - " + t)
            for t in ib[j1:j2]:
                print("    + " + t)
        worst = max(worst, level)
    print("%d kernels compared: %d identical, %d differ%s" % (same + differing, same, differing,
          "" if not differing else " (straight-line code only)" if worst == 1 else " (beyond straight-line code: see above)"))
    return worst


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--diff":
        if len(sys.argv) < 4:
            sys.exit(__doc__)
        sys.exit(diff_main(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else ""))
    filt = sys.argv[1] if len(sys.argv) > 1 else ""
    extra = [a for a in sys.argv[2:]]
    tmp = tempfile.mkdtemp(prefix="lsq_isa_")
    rows = []
    for src in ("lsq_per_tensor.hip", "lsq_per_channel.hip", "lsq_observe.hip"):
        asm = os.path.join(tmp, src + ".s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + extra + [os.path.join(CSRC, src), "-o", asm],
                       check=True, stderr=subprocess.DEVNULL)
        text = open(asm).read()
        # kernel bodies
        bodies = {}
        for m in re.finditer(r"^(_ZN3lsq\w+):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M):
            bodies[m.group(1)] = m.group(2)
        meta = {}
        for m in re.finditer(r"\.group_segment_fixed_size: (\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size: (\d+).*?"
                             r"\.sgpr_count:\s+(\d+).*?\.vgpr_count:\s+(\d+)", text, re.S):
            meta[m.group(2)] = (int(m.group(1)), int(m.group(3)), int(m.group(4)), int(m.group(5)))
        for name, body in bodies.items():
            ins = re.findall(r"^\s+([a-z_0-9]+)", body, re.M)
            cnt = lambda pat: sum(1 for i in ins if re.fullmatch(pat, i))
            lds, scratch, sgpr, vgpr = meta.get(name, (-1, -1, -1, -1))
            rows.append((name, vgpr, sgpr, scratch, lds, cnt(r"v_(fma|fmac|mad)_f(32|64).*"), cnt(r"v_div_fmas_f(32|64)"),
                         cnt(r"global_load_dwordx4"), cnt(r"global_store_dwordx4"),
                         cnt(r"global_load_(dword|ushort|short_d16.*|dwordx2|ubyte)"), cnt(r"ds_add_f64|ds_add_rtn_f64"),
                         cnt(r"v_rndne_f(32|64).*"), len(ins)))
    dm = demangle([r[0] for r in rows])
    print("%-5s %-5s %-7s %-5s %-4s %-4s %-5s %-5s %-5s %-6s %-5s %-6s  kernel" %
          ("vgpr", "sgpr", "scratch", "lds", "fma", "div", "ld16", "st16", "ldsm", "ldsadd", "rndne", "instr"))
    for r in sorted(rows, key=lambda r: dm[r[0]]):
        short = re.sub(r"\(.*", "", dm[r[0]]).replace("lsq::", "").replace("void ", "")
        if filt in short:
            print("%-5d %-5d %-7d %-5d %-4d %-4d %-5d %-5d %-5d %-6d %-5d %-6d  %s" % (r[1:] + (short,)))


if __name__ == "__main__":
    main()
