#!/usr/bin/env python3
"""Pattern-set findall (profiles/set_findall.md): one PatternSet.findall call against the calls it replaces.

  python tools/bench_set_findall.py [--reps R] [--ks 1,2,4,8,16,64] [--layouts pitch,ragged] [--no-sparse] [--out F]

Batch: make_c2_batch(2**20, 1024) at a fixed pitch and its to_ragged CSR form.  Members as in tools/bench_set.py (the
five configs' patterns, then streamable patterns of tests/pattern_gen.py).  Per k: the set call's ms beside the sum of
the k single findall calls and beside the sum of the k (count + findall) calls, each as a caller makes them (every
call reads its total back).  One sparse rule set: 64 members of which four match (the other 60 begin with a byte the
batch never holds)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import mojo_regex_amd as M  # noqa: E402
from bench_set import members, timed  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch, to_ragged  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="1,2,4,8,16,64")
    ap.add_argument("--layouts", default="pitch,ragged")
    ap.add_argument("--no-sparse", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    arr = make_c2_batch(1 << 20, 1024)
    flat = arr.reshape(-1)
    data, off = to_ragged(arr)
    nd = int(off[-1])
    layouts = {"pitch": (M.DeviceBatch.strided(flat, 1024, length=1024), flat.numel()),
               "ragged": (M.DeviceBatch.csr_known(data, off, nd, 1024), nd)}
    layouts = {k: v for k, v in layouts.items() if k in args.layouts.split(",")}
    ks = [int(x) for x in args.ks.split(",")]
    pats = members(max(ks))
    cases = [("k%d" % k, pats[:k]) for k in ks]
    if not args.no_sparse:
        cases.append(("sparse64", pats[:4] + [b"\x01(?:" + p + b")" for p in members(64)[4:]]))
    rows = []
    for name, ps in cases:
        s = M.compile_set(ps)
        rxs = [M.CompiledRegex(p) for p in ps]
        for lay, (batch, nbytes) in layouts.items():
            prefix, _, _ = s.findall(batch)
            total = int(prefix[-1])
            matching = int((s.count(batch).sum(0) > 0).sum())
            del prefix
            ms_set = timed(lambda: s.findall(batch), args.reps)
            ms_findall = timed(lambda: [rx._dev_findall(batch) for rx in rxs], max(1, args.reps // 2))
            ms_both = timed(lambda: [(rx.count(batch), rx._dev_findall(batch)) for rx in rxs], max(1, args.reps // 2))
            r = {"set": name, "k": len(ps), "layout": lay, "members_matching": matching, "hits": total,
                 "ms_set_findall": round(ms_set, 3), "ms_sum_findall": round(ms_findall, 3),
                 "ms_sum_count_findall": round(ms_both, 3), "gbs_set": round(nbytes / ms_set / 1e6, 1),
                 "set_vs_findall_loop": round(ms_findall / ms_set, 3)}
            rows.append(r)
            print(json.dumps(r), flush=True)
        del s
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
