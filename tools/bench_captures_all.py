#!/usr/bin/env python3
"""captures_all against sub with the template \\1 on the same batch (profiles/captures_all.md).

  python tools/bench_captures_all.py [--n N] [--len L] [--reps R] [--out FILE.jsonl]

One pattern per route: '(\\d{3})(\\d{3})(\\d{4})' on phone-like texts (k_capall_fixed), '(\\w+) (\\w+)' on words
(k_capall_chain), '(a|ab)(c|bcd)(d*)' (k_capall_count / k_capall_emit).  Texts: N rows of L bytes at a fixed pitch.
The two calls alternate in one process, R times each; ms per call and GB/s of input, from HIP events."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mojo_regex_amd as M  # noqa: E402


def batch(kind, n, L, rng):
    if kind == "phone":
        al = np.frombuffer(b"Call  or today. -", np.uint8)
        arr = rng.choice(al, size=(n, L)).astype(np.uint8)
        digits = rng.integers(0x30, 0x3A, size=(n, L), dtype=np.uint8)
        for s in range(0, L - 10, 37):   # a 10-digit number every 37 bytes
            arr[:, s:s + 10] = digits[:, s:s + 10]
    elif kind == "words":
        words = [b"hello", b"world", b"foo", b"bar", b"baz", b"qux", b"regex", b"gpu"]
        row = b" ".join(words[i % len(words)] for i in range(L))[:L]
        base = np.frombuffer(row * 2, np.uint8)
        shifts = rng.integers(0, L, size=n)
        arr = np.stack([base[s:s + L] for s in shifts[:min(n, 4096)]])
        arr = np.resize(arr, (n, L))
    else:
        arr = rng.choice(np.frombuffer(b"abcd abcd acd x", np.uint8), size=(n, L)).astype(np.uint8)
    return torch.from_numpy(arr.reshape(-1)).cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="one of phone, words, alt")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(20261015)
    lib = M.load_library()
    cases = [("phone", b"(\\d{3})(\\d{3})(\\d{4})"), ("words", b"(\\w+) (\\w+)"), ("alt", b"(a|ab)(c|bcd)(d*)")]
    rows = []
    for kind, pat in cases:
        if args.only and kind != args.only:
            continue
        d = batch(kind, args.n, args.len, rng)
        b = M.DeviceBatch.strided(d, args.len, length=args.len)
        rx = M.compile_regex(pat)
        prefix, groups = rx.captures_all(b)   # warm-up; sizes the buffers
        kernel = lib.mrx_last_kernel_name().decode()
        total = int(prefix[-1])
        cap = total + 64
        _, sub_out = rx.sub_dev(b"\\1", b)
        sub_cap = int(sub_out.numel()) + 64
        torch.cuda.synchronize()
        t_cap, t_sub = [], []
        for _ in range(args.reps):   # alternating, same process
            t_cap.append(timed(lambda: rx._captures_all_dev(b, 0, match_cap=cap)))
            t_sub.append(timed(lambda: rx.sub_dev(b"\\1", b, out_cap=sub_cap)))
        gb = args.n * args.len / 1e9
        r = {"pattern": pat.decode(), "texts": kind, "n": args.n, "len": args.len, "route": kernel, "matches": total,
             "captures_all_ms": round(float(np.median(t_cap)), 3), "sub_ms": round(float(np.median(t_sub)), 3),
             "captures_all_GBps": round(gb / (np.median(t_cap) / 1e3), 1), "sub_GBps": round(gb / (np.median(t_sub) / 1e3), 1)}
        rows.append(r)
        print(json.dumps(r), flush=True)
        del d, b, prefix, groups, sub_out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
