#!/usr/bin/env python3
"""Pattern-set sub (profiles/set_sub.md): one PatternSet.sub call beside the set findall of the same set and the k
single sub calls.

  python tools/bench_set_sub.py [--reps R] [--ks 1,2,4,8,16,64] [--layouts pitch,ragged] [--no-sparse] [--out F]

Batch: make_c2_batch(2**20, 1024) at a fixed pitch and its to_ragged CSR form.  Members as in tools/bench_set.py; the
sparse set as in tools/bench_set_findall.py.  Member j's replacement is "<j>".  The k single sub calls are a cost
comparison only: their semantics differ (each call sees the previous call's output)."""
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
    ap.add_argument("--no-singles", action="store_true", help="skip the k single sub calls")
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
        reps = [b"<%d>" % j for j in range(len(ps))]
        rxs = [M.CompiledRegex(p) for p in ps]
        for lay, (batch, nbytes) in layouts.items():
            out_off, out, nsub = s.subn(reps, batch)
            out_bytes, nrep = int(out.numel()), int(nsub.sum())
            del out_off, out, nsub
            prefix, _, _ = s.findall(batch)
            hits = int(prefix[-1])
            del prefix
            ms_sub = timed(lambda: s.sub(reps, batch), args.reps)
            ms_fa = timed(lambda: s.findall(batch), args.reps)
            r = {"set": name, "k": len(ps), "layout": lay, "hits": hits, "replacements": nrep,
                 "out_bytes": out_bytes, "ms_set_sub": round(ms_sub, 3), "ms_set_findall": round(ms_fa, 3),
                 "ms_sub_over_findall": round(ms_sub - ms_fa, 3)}
            if not args.no_singles:
                r["ms_sum_single_sub"] = round(timed(lambda: [rx.sub_dev(reps[j], batch) for j, rx in enumerate(rxs)],
                                                     max(1, args.reps // 2)), 3)
            rows.append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
        del s
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
