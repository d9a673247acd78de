#!/usr/bin/env python3
"""Keywords on one GPU (profiles/keywords.md).  Entries: m seeded lower-case words of 4 to 12 bytes, m = 16, 256, 10^4 and
10^5.  Batches: the headline batch (2^20 texts of 1 KiB at a fixed pitch), its ragged CSR cut (the same rows cut to
U[64, 1024] bytes and packed) and the same GiB read as 64 texts of 16 MiB.
  (1) per m and batch: `count` (k_kw_count, the scan, k_kw_text) and `findall` with a capacity that fits (the same, one
      synchronisation for the total, k_kw_emit), the hits, and the automaton (states, classes, table bytes);
  (2) `count` on the headline batch with the LDS tier on and off;
  (3) a sweep of the piece size P, `count`, m = 10^4, on the headline batch and on the 64 long texts;
  (4) the build (Keywords(entries) from host entries: trie, failure links, dense table, three uploads, one
      synchronisation), host clock around a call that ends synchronised;
  (5) beside them, in the same run: `PatternSet.count` on the same entries at k = 16 and 256 (the only route the API had;
      every member's own call) and a plain device copy of the input.
Times are medians of device-event timings after warm-up, with the fastest and slowest call.  Before anything is timed
the hits of k = 16 are compared with the set's counts (they agree unless an entry overlaps itself in a text).

  python tools/bench_keywords.py [--out TABLE.md] [--small] [--skip-set]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch  # noqa: E402

SIZES = (16, 256, 10**4, 10**5)


def timed(fn, warmup=2, reps=5):
    """(median, fastest, slowest) of `reps` device-event timings in ms."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def words(m):
    rng = np.random.default_rng(20261020)
    out, seen = [], set()
    while len(out) < m:
        w = bytes(rng.integers(97, 123, size=int(rng.integers(4, 13))).tolist())
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def ragged_of(data, n, L, lo, hi, seed):
    """The same rows cut to lengths U[lo, hi] and packed: a CSR batch with known bounds."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lens = torch.randint(lo, hi + 1, (n,), device="cuda", generator=g)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), lens, output_size=total)
    src = row * L + (torch.arange(total, device="cuda") - off[:-1][row])
    return M.DeviceBatch.csr_known(data[src], off, total, hi)


def fmt(t):
    return "%.2f (%.2f - %.2f)" % t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--skip-set", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_keywords.py measures on a GPU"
    lib = M.load_library()
    k = 64 if args.small else 1
    n, L = (1 << 20) // k, 1024
    data = make_c2_batch(n).reshape(-1)
    long_len = (16 << 20) // k
    batches = [("%d x 1 KiB, fixed pitch" % n, M.DeviceBatch.strided(data, L, length=L)),
               ("%d ragged texts of 64..1024 bytes, CSR" % n, ragged_of(data, n, L, 64, 1024, 7)),
               ("%d x %d KiB, fixed pitch" % (data.numel() // long_len, long_len >> 10), M.DeviceBatch.strided(data, long_len, length=long_len))]
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    sets, builds = {}, {}
    for m in SIZES:
        ws = words(m)
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kw = M.Keywords(ws)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        sets[m], builds[m] = (ws, kw), statistics.median(ts)

    dst = torch.empty_like(data)
    copy = timed(lambda: dst.copy_(data))
    del dst
    say("Input: %.1f MiB.  A plain device copy of it: %s ms.\n" % (data.numel() / 2**20, fmt(copy)))

    say("### (1) count and findall, ms: median (fastest - slowest)\n")
    say("| m | batch | MiB | hits | count | GiB/s (count) | findall | count / copy |")
    say("|---|---|---|---|---|---|---|---|")
    for m in SIZES:
        ws, kw = sets[m]
        for title, batch in batches:
            mib = batch.data.numel() / 2**20
            hits = int(kw.count(batch).sum())
            cap = max(hits, 1)
            prefix, ents, spans = kw.findall(batch, span_cap=cap)
            assert int(prefix[-1]) == hits == ents.numel()
            del prefix, ents, spans
            c = timed(lambda: kw.count(batch))
            f = timed(lambda: kw.findall(batch, span_cap=cap))
            say("| %d | %s | %.0f | %d | %s | %.1f | %s | %.1fx |" % (m, title, mib, hits, fmt(c), mib / 1024 / (c[0] / 1e3), fmt(f),
                                                                 c[0] / copy[0]))
    say("\nAutomata: " + "; ".join("m=%d: %s" % (m, sets[m][1].describe().split(": ")[1]) for m in SIZES) + "\n")

    say("### (2) the LDS tier: count on the headline batch, ms\n")
    say("| m | rows of the shallowest states in LDS | every row from global memory |")
    say("|---|---|---|")
    head = batches[0][1]
    for m in SIZES:
        kw = sets[m][1]
        row = []
        for lds in (1, 0):
            lib.mrx_debug_kw_tier(lds)
            row.append(fmt(timed(lambda: kw.count(head))))
        lib.mrx_debug_kw_tier(1)
        say("| %d | %s |" % (m, " | ".join(row)))

    say("\n### (3) the piece size: count with m = 10^4, ms\n")
    sizes = (64, 128, 256, 512, 1024, 4096, 16384)
    say("| batch | " + " | ".join("P = %d" % p for p in sizes) + " | the rule |")
    say("|---|" + "---|" * (len(sizes) + 1))
    kw = sets[10**4][1]
    for title, batch in (batches[0], batches[2]):
        row = []
        for p in sizes + (0,):
            lib.mrx_debug_kw_piece(p)
            row.append(fmt(timed(lambda: kw.count(batch))))
        lib.mrx_debug_kw_piece(0)
        say("| %s | %s |" % (title, " | ".join(row)))

    say("\n### (4) the build, ms (host clock, median of 3)\n")
    say("| m | build |")
    say("|---|---|")
    for m in SIZES:
        say("| %d | %.1f |" % (m, builds[m]))

    if not args.skip_set:
        say("\n### (5) PatternSet.count on the same entries, headline batch, ms\n")
        say("| k | PatternSet.count | Keywords.count | set / keywords | hits agree |")
        say("|---|---|---|---|---|")
        for m in (16, 256):
            ws, kw = sets[m]
            ps = M.compile_set(ws)
            theirs = ps.count(head)
            agree = bool(torch.equal(theirs.to(torch.int64).sum(dim=1), kw.count(head)))
            del theirs
            s = timed(lambda: ps.count(head), warmup=1, reps=3)
            c = timed(lambda: kw.count(head))
            say("| %d | %s | %s | %.1fx | %s |" % (m, fmt(s), fmt(c), s[0] / c[0], "yes" if agree else "NO"))
            del ps
            torch.cuda.empty_cache()

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
