#!/usr/bin/env python3
"""Pattern-set k-sweep (profiles/set_scan.md): one set call against the k single-pattern calls it replaces.

  python tools/bench_set.py [--reps R] [--out FILE.jsonl]

Batch: make_c2_batch(2**20, 1024) at a fixed pitch and its to_ragged CSR form.  Members, deterministically: the five
configs' patterns, then streamable patterns of tests/pattern_gen.py.  For count, search and matches: the set call's ms
(shared pass forced, mrx_debug_set_route(1), and under the route rule) and GB/s of input, beside the sum of the k
single-pattern calls (count / search)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import mojo_regex_amd as M  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch, to_ragged  # noqa: E402
from pattern_gen import patterns as gen_patterns  # noqa: E402

CONFIG = [b"hello", b"[a-z]+\\d+", b"\\d+", b"(\\d{3})(\\d{3})(\\d{4})", b"(x|y|foo|bar)+"]


def members(kmax):
    out = list(CONFIG)
    for p in gen_patterns(20261015, 2000):
        if len(out) >= kmax:
            break
        p = p.encode()
        try:
            d = M.CompiledRegex(p).describe()
        except M.MrxError:
            continue
        if "device.streamable=yes" in d and "findall_only=1" not in d and p not in out:
            out.append(p)
    return out[:kmax]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="1,2,4,8,16,32,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = M.load_library()
    arr = make_c2_batch(1 << 20, 1024)
    flat = arr.reshape(-1)
    data, off = to_ragged(arr)
    layouts = {"pitch": (M.DeviceBatch.strided(flat, 1024, length=1024), flat.numel()),
               "ragged": (M.DeviceBatch(data, off), data.numel())}
    ks = [int(x) for x in args.ks.split(",")]
    pats = members(max(ks))
    rows = []
    for k in ks:
        ps = pats[:k]
        s = M.compile_set(ps)
        rxs = [M.CompiledRegex(p) for p in ps]
        shared = sum(1 for ln in s.describe().splitlines() if " count=shared" in ln)
        for lay, (batch, nbytes) in layouts.items():
            for op in ("count", "search", "matches"):
                setfn = getattr(s, op)
                lib.mrx_debug_set_route(1)
                ms_shared = timed(lambda: setfn(batch), args.reps)
                lib.mrx_debug_set_route(2)
                ms_own = timed(lambda: setfn(batch), args.reps)
                lib.mrx_debug_set_route(0)
                ms_rule = timed(lambda: setfn(batch), args.reps)
                kern = lib.mrx_last_kernel_name().decode()
                if op == "count":
                    loop = lambda: [rx.count(batch) for rx in rxs]  # noqa: E731
                else:
                    loop = lambda: [rx._dev_spans(rx._lib.mrx_search_dev, rx._lib.mrx_search_strided_dev, batch)  # noqa: E731
                                    for rx in rxs]
                ms_loop = timed(loop, max(1, args.reps // 2))
                r = {"k": k, "layout": lay, "op": op, "shared_members": shared, "ms_shared": round(ms_shared, 4),
                     "ms_own_route": round(ms_own, 4), "ms_rule": round(ms_rule, 4), "rule_kernel": kern,
                     "ms_single_loop": round(ms_loop, 4), "gbs_shared": round(nbytes / ms_shared / 1e6, 1),
                     "gbs_single_loop": round(nbytes / ms_loop / 1e6, 1)}
                rows.append(r)
                print(json.dumps(r), flush=True)
        del s
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
