#!/usr/bin/env python3
"""Are two builds' device code the same?  Compares two sets of `hipcc --save-temps` device assembly files
(*-hip-amdgcn-amd-amdhsa-gfx950.s) function by function, whatever file a function is in and whatever order the compiler
emitted them in: the instructions of every function (labels renumbered per function, since their numbers carry the
function's index in the file), every kernel descriptor (.amdhsa_kernel block: registers, scratch, LDS) and every
kernel's metadata entry.

Functions are matched by demangled name with the `(anonymous namespace)::` and `mrx::` qualifiers removed, and mangled
names inside a function's text (.type, .size, .globl, the descriptor's symbol, calls) are rewritten the same way: code
that moved to another unit or into the namespace compares equal when its instructions are.

usage: python tools/compare_device_asm.py parent1.s,parent2.s,... change1.s,change2.s,...    exit status 0 = identical"""
import os
import re
import shutil
import subprocess
import sys

# ROCm's demangler where it is installed, else the one of binutils
CXXFILT = next(p for p in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")) if p and os.path.exists(p))
MANGLED = re.compile(r"_Z\w+")


def demangler(paths):
    """mangled token -> demangled name without the qualifiers, for every mangled token of the files (one filter run)."""
    tokens = sorted({t for p in paths for t in MANGLED.findall(open(p).read())})
    if not tokens:
        return {}
    out = subprocess.run([CXXFILT], input="\n".join(tokens) + "\n", capture_output=True, text=True, check=True).stdout
    names = out.split("\n")[:len(tokens)]
    return {t: n.replace("(anonymous namespace)::", "").replace("mrx::", "") for t, n in zip(tokens, names)}


def functions(paths):
    """name -> sorted normalised texts of the functions of that name (one per file that has it); the same for the
    kernel descriptors and the metadata entries."""
    names = demangler(paths)
    plain = lambda text: MANGLED.sub(lambda m: names.get(m.group(0), m.group(0)), text)
    out, desc, meta = {}, {}, {}
    for path in paths:
        cur, in_meta = None, False
        for line in open(path):
            m = re.match(r"\s*\.section\s+\.text\.(\S+?),", line)
            if m:
                cur = []
                out.setdefault(plain(m.group(1)), []).append(cur)
                continue
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                cur = []
                desc.setdefault(plain(m.group(1)), []).append(cur)
                continue
            if re.match(r"\s*\.(section|text)\b", line):   # (another section: the function's text is over)
                cur = None
                continue
            if re.match(r"\s*\.amdgpu_metadata", line):
                in_meta, cur = True, None
                continue
            if re.match(r"\s*\.end_amdgpu_metadata", line):
                in_meta, cur = False, None
                continue
            if in_meta:
                if not line.startswith(" "):   # (a top-level key: the kernels' list begins or is over)
                    cur = None
                if line.startswith("  - ."):
                    cur = []
                    meta[len(meta)] = cur
                if cur is not None:
                    cur.append(plain(line))
                continue
            if cur is not None:
                line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line)   # (the compilation unit's id: a hash of the source)
                line = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", plain(line))
                line = re.sub(r"\bBB\d+_", "BB_", line)   # (loop comments name blocks without the .L)
                line = re.sub(r"[ \t]+;", " ;", line)   # (a comment's column moves with the label's length)
                cur.append(re.sub(r" ; %(?!bb\.).*$", "", line))   # (an IR value's name: numbered per unit)
    by_symbol = {}
    for entry in meta.values():
        sym = [m.group(1) for m in (re.match(r"\s+\.symbol:\s+(.+)", ln) for ln in entry) if m]
        by_symbol.setdefault(sym[0] if sym else "".join(entry[:2]), []).append(entry)
    return [{k: sorted("".join(t) for t in v) for k, v in d.items()} for d in (out, desc, by_symbol)]


def main():
    a, b = functions(sys.argv[1].split(",")), functions(sys.argv[2].split(","))
    bad = 0
    for what, x, y in zip(("functions", "kernel descriptors", "metadata entries"), a, b):
        if sorted(x) != sorted(y):
            print("the set of %s differs: only left %s, only right %s" % (what, sorted(set(x) - set(y))[:5], sorted(set(y) - set(x))[:5]))
            bad += 1
        diff = [k for k in x if k in y and x[k] != y[k]]
        print("%-18s %5d left, %5d right, %d differ" % (what, sum(map(len, x.values())), sum(map(len, y.values())), len(diff)))
        for k in diff[:5]:
            print("   differs:", k)
        bad += len(diff)
    print("device code identical" if not bad else "DEVICE CODE DIFFERS")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
