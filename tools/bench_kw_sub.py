#!/usr/bin/env python3
"""Keywords.sub and Keywords.leftmost on one GPU (profiles/kw_sub.md).  Entries and batches are those of
tools/bench_keywords.py (m seeded lower-case words of 4 to 12 bytes, m = 16, 256, 10^4 and 10^5; the headline batch of
2^20 texts of 1 KiB, its ragged CSR cut, the same GiB as 64 texts of 16 MiB), and beside them the GiB as log lines of 99
bytes at a fixed pitch and HEADLESS texts of 1 and 16 MiB (`aaaa...` with the entries `a` .. `aaaa`: no candidate behind the
first is a head, so one lane walks the whole selection).  Every fourth word is planted into the batch at a seeded
position of every 1 KiB, so that there is something to replace.
  (1) per m and batch, the routes taking turns call by call: `sub` with one 8-byte replacement, `sub` with a replacement
      per entry (0 to 12 bytes), `leftmost`, `Keywords.findall` on the same input (what the hits cost before), and with
      k = 16 and 256 `PatternSet.sub` (the route that sub replaces where it applies: not timed on the 16 MiB texts, which
      it selects with one wavefront each; it resolves equal starts by member order, not by length); beside them a plain device copy of the input;
  (2) the first leftmost / sub call on a fresh handle (the reversed build and its upload) per m, host clock;
  (3) --profile-row: only `sub`, m = 10^4, on the headline batch, five calls, for a kernel trace of its own.
Times are medians of 7 device-event timings after warm-up, with the fastest and slowest call.

  python tools/bench_kw_sub.py [--out TABLE.md] [--small] [--skip-set] [--profile-row]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch  # noqa: E402
from bench_keywords import SIZES, fmt, ragged_of, words  # noqa: E402


def timed_turns(fns, warmup=2, reps=7):
    """{name: (median, fastest, slowest)} in ms of device-event timings; the routes take turns, call by call."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[name].append(a.elapsed_time(b))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in ts.items()}


def plant(data, ws, every=1024, seed=11):
    """One of `ws` written into every `every` bytes of data at a seeded position (in place)."""
    rng = np.random.default_rng(seed)
    n = data.numel() // every
    pick = rng.integers(0, len(ws), size=n)
    at = rng.integers(0, every - 16, size=n) + np.arange(n) * every
    host = data.cpu().numpy()
    for j in np.unique(pick):
        w = np.frombuffer(ws[int(j)], np.uint8)
        pos = at[pick == j]
        host[pos[:, None] + np.arange(len(w))[None, :]] = w
    data.copy_(torch.from_numpy(host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--skip-set", action="store_true")
    ap.add_argument("--profile-row", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kw_sub.py measures on a GPU"
    k = 64 if args.small else 1
    n, L = (1 << 20) // k, 1024
    data = make_c2_batch(n).reshape(-1)
    all_words = {m: words(m) for m in SIZES}
    plant(data, all_words[16][::4] + all_words[256][::4] + all_words[10**4][::4] + all_words[10**5][::4])
    long_len = (16 << 20) // k
    nl = data.numel() // 99
    batches = [("%d x 1 KiB, fixed pitch" % n, M.DeviceBatch.strided(data, L, length=L)),
               ("%d ragged texts of 64..1024 bytes, CSR" % n, ragged_of(data, n, L, 64, 1024, 7)),
               ("%d x %d KiB, fixed pitch" % (data.numel() // long_len, long_len >> 10),
                M.DeviceBatch.strided(data, long_len, length=long_len)),
               ("%d lines of 99 bytes, fixed pitch" % nl, M.DeviceBatch.strided(data[:nl * 99], 99, length=99))]
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    if args.profile_row:
        kw = M.Keywords(all_words[10**4])
        for _ in range(5):
            kw.sub(b"[REDACT]", batches[0][1])
        torch.cuda.synchronize()
        print("profile row done")
        return

    dst = torch.empty_like(data)
    copy = timed_turns({"copy": lambda: dst.copy_(data)})["copy"]
    del dst
    say("Input: %.1f MiB.  A plain device copy of it: %s ms.\n" % (data.numel() / 2**20, fmt(copy)))

    say("### (1) sub, leftmost and findall, ms: median of 7 (fastest - slowest), the routes taking turns\n")
    say("| m | batch | matches | sub, one replacement | sub, per entry | leftmost | findall | PatternSet.sub | sub / copy | "
        "PatternSet.sub / sub |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    first_call = {}
    for m in SIZES:
        ws = all_words[m]
        per = [w.upper()[:j % 13] for j, w in enumerate(ws)]
        kw = M.Keywords(ws)
        tiny = M.DeviceBatch.from_texts([b"warm"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kw.leftmost(tiny)
        torch.cuda.synchronize()
        first_call[m] = (time.perf_counter() - t0) * 1e3
        per_dev = kw._repl_batch(per, "cuda")
        one_dev = kw._repl_batch(b"[REDACT]", "cuda")
        ps = M.compile_set(ws) if m <= 256 and not args.skip_set else None
        for title, batch in batches:
            prefix, ents, spans = kw.leftmost(batch)
            matches = int(prefix[-1])
            hits = int(kw.count(batch).sum())
            out = kw.sub(one_dev, batch)
            cap, ocap = max(matches, 1), int(out.data.numel()) + matches * 8 + 64
            del prefix, ents, spans, out
            fns = {"sub1": lambda: kw.sub(one_dev, batch, out_cap=ocap),
                   "subm": lambda: kw.sub(per_dev, batch, out_cap=ocap),
                   "left": lambda: kw.leftmost(batch, span_cap=cap),
                   "find": lambda: kw.findall(batch, span_cap=max(hits, 1))}
            with_set = ps is not None and batch.stride != long_len   # (a wavefront per text: not on the 16 MiB texts)
            if with_set:
                need = int(ps.sub(b"[REDACT]", batch)[1].numel())
                fns["set"] = lambda: ps.sub(b"[REDACT]", batch, out_cap=need + 64)
            t = timed_turns(fns, warmup=1 if with_set else 2)
            slower = with_set and t["sub1"][0] > t["set"][0]
            cells = ["%d" % m, title, "%d" % matches, fmt(t["sub1"]), fmt(t["subm"]), fmt(t["left"]), fmt(t["find"]),
                     fmt(t["set"]) if with_set else "-", "%.1fx" % (t["sub1"][0] / copy[0]),
                     "%.1fx" % (t["set"][0] / t["sub1"][0]) if with_set else "-"]
            if slower:   # slower than the route it replaces
                cells = ["**%s**" % c for c in cells]
            say("| " + " | ".join(cells) + " |")
        del ps
        torch.cuda.empty_cache()

    say("\n### (2) the first leftmost / sub call on a fresh handle (the reversed build and its upload), ms, host clock\n")
    say("| m | first call |")
    say("|---|---|")
    for m in SIZES:
        say("| %d | %.1f |" % (m, first_call[m]))

    say("\n### The headless text: `a` repeated, entries `a` .. `aaaa`, ms (the larger one: a single call each, no warm-up)\n")
    say("| text | matches | sub, one replacement | leftmost | findall | a copy of the text |")
    say("|---|---|---|---|---|---|")
    kw = M.Keywords([b"a", b"aa", b"aaa", b"aaaa"])
    one_dev = kw._repl_batch(b"[REDACT]", "cuda")
    for size, warm, reps in ((long_len // 16, 1, 3), (long_len, 0, 1)):
        head = M.DeviceBatch.from_texts([b"a" * size])
        matches, hits = (size + 3) // 4, 4 * size - 6
        dst = torch.empty_like(head.data)
        t = timed_turns({"sub1": lambda: kw.sub(one_dev, head, out_cap=matches * 8 + 64),
                         "left": lambda: kw.leftmost(head, span_cap=matches),
                         "find": lambda: kw.findall(head, span_cap=hits),
                         "copy": lambda: dst.copy_(head.data)}, warmup=warm, reps=reps)
        say("| **1 x %d KiB** | **%d** | **%s** | **%s** | %s | %s |" % (size >> 10, matches, fmt(t["sub1"]), fmt(t["left"]),
                                                                     fmt(t["find"]), fmt(t["copy"])))
        del head, dst

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
