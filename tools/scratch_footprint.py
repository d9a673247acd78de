"""What the scratch arena holds after each call of tests/scratch_matrix.py: for every case, mrx_release_scratch(), the
call three times (the arena settles within two calls of a batch shape), then mrx_debug_scratch_bytes() -- once at the
matrix's own sizes and once with four times as many texts.  Prints one markdown table row per case.

    python tools/scratch_footprint.py [--check] > table.md      (run on the GPU; --check also compares the results)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import mojo_regex_amd as M  # noqa: E402
import scratch_matrix as SM  # noqa: E402


def footprint(case, check):
    lib = M.load_library()
    torch.cuda.synchronize()
    lib.mrx_release_scratch()
    with SM.switched(case.switch):
        for _ in range(3):
            case.run(check)
    torch.cuda.synchronize()
    return int(lib.mrx_debug_scratch_bytes())


def main():
    check = "--check" in sys.argv[1:]
    small, big = SM.cases(1), SM.cases(4)
    print("| call | bytes, n x 1 | bytes, n x 4 |")
    print("|---|---:|---:|")
    for a, b in zip(small, big):
        print("| %s | %d | %d |" % (a.name.replace("|", "\\|"), footprint(a, check), footprint(b, False)), flush=True)


if __name__ == "__main__":
    main()
