#!/usr/bin/env python3
"""Host time per call of count and findall on a stepper plan: 64 texts of 16 bytes, where the kernels take microseconds
and the call's cost is the host's route decision and launches.  Warm-up, then `reps` rounds of `calls` back-to-back calls
each closed by one synchronisation; prints the median microseconds per call as one JSON line.
MRX_LIB=<path> times another build of the library (profiles/step_route.md)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mojo_regex_amd as M  # noqa: E402


def per_call_us(fn, calls=2000, reps=9):
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e6)
    return round(statistics.median(out), 3), round(min(out), 3), round(max(out), 3)


def main():
    lib = M.load_library()
    rng = np.random.default_rng(3)
    al = np.frombuffer(b"0123456789. ab", dtype=np.uint8)
    texts = [bytes(rng.choice(al, size=16).tolist()) for _ in range(64)]
    batch = M.DeviceBatch.from_texts(texts)
    row = {"lib": os.environ.get("MRX_LIB", "in-tree"), "texts": 64, "bytes": 16}
    for pat in (b"\\d+(\\.\\d+)?", b"\\d{3}-\\d{4}"):
        rx = M.CompiledRegex(pat)
        prefix = torch.empty(batch.n + 1, dtype=torch.int64, device="cuda")
        spans = torch.empty((1024, 2), dtype=torch.int32, device="cuda")
        for op, fn in (("count", lambda: rx.count(batch)), ("findall", lambda: rx._dev_findall(batch, out=(prefix, spans)))):
            med, lo, hi = per_call_us(fn)
            row["%s %s" % (op, pat.decode())] = {"kernel": lib.mrx_last_kernel_name().decode(), "us_median": med, "us_min": lo, "us_max": hi}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
