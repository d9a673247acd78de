#!/usr/bin/env python3
"""Are two builds' device code the same?  Compares two `hipcc --save-temps` device assembly files
(*-hip-amdgcn-amd-amdhsa-gfx950.s) function by function, whatever order the compiler emitted the functions in: the
instructions of every function (labels renumbered per function, since their numbers carry the function's index in the
file), every kernel descriptor (.amdhsa_kernel block: registers, scratch, LDS) and every kernel's metadata entry.

usage: python tools/compare_device_asm.py parent.s change.s     exit status 0 = identical"""
import re
import sys


def functions(path):
    """name -> normalised text of the function's section, its descriptor and its metadata entry."""
    out, cur, name = {}, None, None
    meta, in_meta = {}, False
    desc = {}
    for line in open(path):
        m = re.match(r"\s*\.section\s+\.text\.(\S+?),", line)
        if m:
            name, cur = m.group(1), []
            out[name] = cur
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name, cur = m.group(1), []
            desc[name] = cur
            continue
        if re.match(r"\s*\.amdgpu_metadata", line):
            in_meta, cur = True, None
            continue
        if in_meta:
            if line.startswith("  - ."):
                cur = []
                meta[len(meta)] = cur
            if cur is not None:
                cur.append(line)
            continue
        if cur is not None:
            line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line)   # (the compilation unit's id: a hash of the source)
            cur.append(re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", line))
    by_symbol = {}
    for entry in meta.values():
        sym = [m.group(1) for m in (re.match(r"\s+\.symbol:\s+(\S+)", ln) for ln in entry) if m]
        by_symbol[sym[0] if sym else "".join(entry[:2])] = entry
    return out, desc, by_symbol


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for what, x, y in zip(("functions", "kernel descriptors", "metadata entries"), a, b):
        if sorted(x) != sorted(y):
            print("the set of %s differs: only left %s, only right %s" % (what, sorted(set(x) - set(y))[:5], sorted(set(y) - set(x))[:5]))
            bad += 1
        diff = [k for k in x if k in y and x[k] != y[k]]
        print("%-18s %5d left, %5d right, %d differ" % (what, len(x), len(y), len(diff)))
        for k in diff[:5]:
            print("   differs:", k)
        bad += len(diff)
    print("device code identical" if not bad else "DEVICE CODE DIFFERS")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
