#!/usr/bin/env python3
"""The sorted index on one GPU (profiles/sorted.md).  Per row:
  (b) SortedIndex(entries), the whole build (sort's rounds, the packed copy, the aids), median of 3 host-clock timings;
  (e) / (p) / (l) a search in mode EQUAL / PREFIX / LONGEST of all probes into caller tensors (search_async), each in the
      three forms that mrx_debug_sorted_aids chooses: the plain binary search over the entries' bytes, with the key
      array, and with the fence posts in LDS above it;
  (d) Dictionary.lookup on the same entries and probes: the cost of the equality-only question;
  (t) where every text has exactly 8 bytes: torch.searchsorted of the probes' big-endian words (sign bit flipped) in the
      sorted words of the entries; its answer must equal (e)'s lower bound (checked);
  (h) what a user has today: the probes copied to the host and bisect.bisect_left on the sorted entries -- the copy,
      building the bytes objects and the searches, timed with the host clock on the first --host-probes probes (default
      2^21, an eighth) and reported per million probes;
  (c) a plain device copy of the probed bytes, for scale.
(e), (p), (l), (d), (t) and (c) are medians of 7 device-event timings after warm-up, the routes taking turns in one
process.  Before anything is timed the three forms must agree with each other in every mode, and SortedIndex.index with
Dictionary.lookup.

  python tools/bench_sorted.py [--out TABLE.md] [--small] [--row NAME]
"""
import argparse
import bisect
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402
from bench_distinct import CASES  # noqa: E402

MODES = ("equal", "prefix", "longest")
AIDS = ((0, "bytes"), (1, "keys"), (3, "keys + fence"))


def turns(fns, warmup=2, reps=7):
    """Median ms of every function, by device events, the functions taking turns."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return [statistics.median(t) for t in ts]


def words_of(n, mult=0x1E3779B97F4A7C15):
    """n different texts of 8 bytes (an odd multiplier is a bijection of 64 bits)."""
    keys = torch.arange(n, dtype=torch.int64, device="cuda") * mult
    return M.DeviceBatch.strided(keys.view(torch.uint8), 8, length=8)


def first_rows(batch, m):
    return M.DeviceBatch.strided(batch.data[:m * batch.stride], batch.stride, length=batch.length)


def row_zipf(k):
    title, probes, _ = CASES["zipf"](k)
    return title + ", index: the words that occur", probes.distinct()[0], probes


def row_equal(k):
    _, words, _ = CASES["zipf"](k * 16)
    title, probes, _ = CASES["equal"](k)
    index = words.distinct()[0]
    return title + ", index: %d lower-case words" % index.n, index, probes


def row_unique(k):
    probes = words_of((1 << 24) // k)
    return "%d distinct probes of 8 bytes, index: the first half of them" % probes.n, first_rows(probes, probes.n // 2), probes


def row_headline(k):
    title, probes, _ = CASES["headline"](k)
    return title + ", index: their distinct values", probes.distinct()[0], probes


def row_sweep(m):
    def make(k):
        probes = words_of((1 << 22) // k)
        return "size sweep: %d entries of 8 bytes, %d probes" % (m // k, probes.n), first_rows(words_of((1 << 24) // k), m // k), probes
    return make


def row_urls(k):
    m, n = 1000000 // k, (1 << 22) // k
    head = torch.tensor(list(b"https://www.example-shop.com/catalog/it/"), dtype=torch.uint8, device="cuda")
    assert head.numel() == 40

    def rows(count, mult):
        ids = (torch.arange(count, dtype=torch.int64, device="cuda") * mult) % (2 * m)
        digits = torch.stack([(ids // 10 ** p) % 10 + 48 for p in range(7, -1, -1)], 1).to(torch.uint8)
        return M.DeviceBatch.strided(torch.cat([head.expand(count, 40), digits], 1).reshape(-1).contiguous(), 48, length=48)
    return "URL-like: %d entries of 48 bytes behind 40 shared ones, %d probes" % (m, n), rows(m, 7919), rows(n, 104729)


ROWS = {"zipf": row_zipf, "equal": row_equal, "unique": row_unique, "headline": row_headline, "urls": row_urls}
for _m in (100, 10000, 1000000, 10000000):
    ROWS["sweep%d" % _m] = row_sweep(_m)


def be_words(batch):
    """Texts of exactly 8 bytes as int64 whose signed order is the bytes' unsigned one."""
    rows = batch.data.view(batch.n, batch.stride)[:, :8]
    return rows.flip(1).contiguous().view(torch.int64).view(-1) ^ (-1 << 63)


def host_bisect(entries_sorted, probes, m):
    """Seconds for the first m probes: copy to the host, bytes objects, bisect_left."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if probes.offsets is None:
        raw = probes.data[:m * probes.stride].cpu().numpy().tobytes()
        texts = [raw[i * probes.stride:i * probes.stride + probes.length] for i in range(m)]
    else:
        off = probes.offsets[:m + 1].cpu().numpy()
        raw = probes.data[:int(off[-1])].cpu().numpy().tobytes()
        texts = [raw[off[i]:off[i + 1]] for i in range(m)]
    out = [bisect.bisect_left(entries_sorted, t) for t in texts]
    return time.perf_counter() - t0, out


def host_list(batch):
    if batch.offsets is None:
        raw = batch.data.cpu().numpy().tobytes()
        return [raw[i * batch.stride:i * batch.stride + batch.length] for i in range(batch.n)]
    off, raw = batch.offsets.cpu().numpy(), batch.data.cpu().numpy().tobytes()
    return [raw[off[i]:off[i + 1]] for i in range(batch.n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--row", choices=list(ROWS), action="append")
    ap.add_argument("--host-probes", type=int, default=1 << 21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sorted.py measures on a GPU"
    lib = M.load_library()
    k = 64 if args.small else 1
    forms = " / ".join(name for _, name in AIDS)
    lines = ["| row | probes | entries | distinct | MiB probed | (b) build ms | (e) EQUAL ms: %s | (p) PREFIX ms: %s | (l) LONGEST ms: %s | "
             "M probes/s, best (e) | (d) Dictionary.lookup ms | best (e)/(d) | (t) torch.searchsorted on 8-byte words ms | "
             "(h) host bisect, s per million probes (probes timed) | (c) copy ms |" % (forms, forms, forms),
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in args.row or list(ROWS):
        title, entries, probes = ROWS[name](k)
        n = probes.n
        builds = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix = M.SortedIndex(entries)
            torch.cuda.synchronize()
            builds.append((time.perf_counter() - t0) * 1e3)
        d = M.Dictionary(entries)
        lo = torch.empty(n, dtype=torch.int64, device="cuda")
        hi = torch.empty(n, dtype=torch.int64, device="cuda")
        index = torch.empty(n, dtype=torch.int64, device="cuda")
        answers = {}
        for aids, _ in AIDS:   # the forms agree before anything is timed
            lib.mrx_debug_sorted_aids(aids)
            for mode in MODES:
                ix.search_async(probes, mode, lo, hi)
                got = (lo.clone(), hi.clone())
                if mode in answers:
                    assert torch.equal(got[0], answers[mode][0]) and torch.equal(got[1], answers[mode][1]), (name, aids, mode)
                answers[mode] = got
        lib.mrx_debug_sorted_aids(-1)
        assert torch.equal(ix.index(probes), d.lookup(probes)), name
        assert bool((answers["prefix"][0] == answers["equal"][0]).all()) and bool((answers["prefix"][1] >= answers["equal"][1]).all())

        def search(aids, mode):
            def run():
                lib.mrx_debug_sorted_aids(aids)
                ix.search_async(probes, mode, lo, hi)
            return run
        fns = [search(aids, mode) for mode in MODES for aids, _ in AIDS]
        fns.append(lambda: d.lookup_async(probes, index))
        dst = torch.empty_like(probes.data)
        fns.append(lambda: dst.copy_(probes.data))
        eight = probes.offsets is None and entries.offsets is None and probes.length == 8 and entries.length == 8
        if eight:
            sorted_words = torch.sort(be_words(entries)).values
            probe_words = be_words(probes)
            assert torch.equal(torch.searchsorted(sorted_words, probe_words), answers["equal"][0]), name
            fns.append(lambda: torch.searchsorted(sorted_words, probe_words))
        ms = turns(fns)
        lib.mrx_debug_sorted_aids(-1)
        per_mode = [ms[3 * q:3 * q + 3] for q in range(3)]
        look, copy = ms[9], ms[10]
        t_txt = "%.3f" % ms[11] if eight else "not applicable"
        m = min(n, args.host_probes // k)
        srt = sorted(host_list(entries)) if entries.n <= 2000000 else None
        if srt is not None:
            secs, out = host_bisect(srt, probes, m)
            assert out == answers["equal"][0][:m].tolist(), name
            h_txt = "%.2f (%d)" % (secs / m * 1e6, m)
        else:
            h_txt = "not timed: %d entries as bytes objects" % entries.n
        best = min(per_mode[0])
        cells = [" / ".join("%.3f" % t for t in row) for row in per_mode]
        lines.append("| %s | %d | %d | %d | %.1f | %.1f | %s | %s | %s | %.0f | %.3f | %.2fx | %s | %s | %.3f |" % (
            title, n, len(ix), ix.distinct_count, int(probes.data.numel()) / 2**20, statistics.median(builds), cells[0], cells[1],
            cells[2], n / best / 1e3, look, best / look, t_txt, h_txt, copy))
        print(lines[-1], flush=True)
        del ix, d, lo, hi, index, dst, answers, entries, probes
        torch.cuda.empty_cache()
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
