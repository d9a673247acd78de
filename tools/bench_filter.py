#!/usr/bin/env python3
"""filter on one GPU (profiles/filter.md): per batch shape and kept fraction
  (a) search alone -- the floor, the predicate is part of the call;
  (b) filter, with each form of the gather (mrx_debug_filter_form);
  (c) what the public API offered before: search, then a torch mask, a cumulative sum and a gather (row-mask indexing
      for a fixed pitch, a per-byte index gather for CSR);
  (d) a plain device copy of as many bytes as were kept;
and a set of 7 and of 64 members against its own matches call.  Times are medians of device-event timings after
warm-up, and (b) is timed a second time with its fastest and slowest call; every filter result is compared with (c)'s
bytes before it is timed.

  python tools/bench_filter.py [--out profiles/filter.md] [--small]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402

NEEDLE = b"hello"
ALPHABET = b"abcxyz0189 -"


def timed(fn, warmup=3, reps=10, spread=False):
    """Median of `reps` device-event timings in ms; with spread, (median, fastest, slowest)."""
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
    return (statistics.median(ts), min(ts), max(ts)) if spread else statistics.median(ts)


def make_pitch(n, L, frac, seed):
    """n rows of L bytes without the needle; it is planted at the start of about frac of them."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    al = torch.tensor(list(ALPHABET), dtype=torch.uint8, device="cuda")
    data = al[torch.randint(0, len(ALPHABET), (n, L), device="cuda", generator=g)]
    rows = torch.nonzero(torch.rand(n, device="cuda", generator=g) < frac).flatten()
    data[rows, :len(NEEDLE)] = torch.tensor(list(NEEDLE), dtype=torch.uint8, device="cuda")
    return data.reshape(-1)


def ragged_of(data, n, L, lo, hi, seed):
    """The same rows cut to lengths U[lo, hi] and packed: a CSR batch (the needle stays at each text's start)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lens = torch.randint(lo, hi + 1, (n,), device="cuda", generator=g)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), lens, output_size=total)
    src = row * L + (torch.arange(total, device="cuda") - off[:-1][row])
    packed = data[src]
    return M.DeviceBatch.csr_known(packed, off, total, hi)


def torch_filter(rx, batch):
    """(c): search, mask, cumulative sum, gather."""
    s, _ = rx.search(batch)
    mask = s >= 0
    if batch.offsets is None:
        rows = batch.data.view(batch.n, batch.stride)[mask]
        return rows.reshape(-1)
    off = batch.offsets
    lens = (off[1:] - off[:-1]) * mask
    out_off = torch.zeros(batch.n + 1, dtype=torch.int64, device=off.device)
    out_off[1:] = torch.cumsum(lens, 0)
    idx = torch.nonzero(mask).flatten()
    total = int(out_off[-1])
    shift = (off[:-1] - out_off[:-1])[idx]
    src = torch.repeat_interleave(shift, lens[idx], output_size=total) + torch.arange(total, device=off.device)
    return batch.data[src]


def cell(lib, rx, batch, name, frac, lines, forms=(0, 1, 16)):
    want = torch_filter(rx, batch)
    res = {}
    for form in forms:
        lib.mrx_debug_filter_form(form)
        kb, _ = rx.filter(batch)
        assert torch.equal(kb.data, want), (name, frac, form)
        res[form] = timed(lambda: rx.filter(batch))
    lib.mrx_debug_filter_form(0)
    _, b_lo, b_hi = timed(lambda: rx.filter(batch), spread=True)   # the rule's form once more: the spread of (b)
    kept_bytes = int(want.numel())
    del want
    a = timed(lambda: rx.search(batch))
    c = timed(lambda: torch_filter(rx, batch), warmup=2, reps=5)
    dst = torch.empty(max(kept_bytes, 1), dtype=torch.uint8, device="cuda")
    d = timed(lambda: dst[:kept_bytes].copy_(batch.data[:kept_bytes]))
    b = res[0]
    gbs = kept_bytes / max(b - a, 1e-6) / 1e6
    lines.append("| %s | %d%% | %.1f | %.3f | %.3f | %.3f - %.3f | %s | %.3f | %.1fx | %.3f | %.3f | %.0f |" % (
        name, round(frac * 100), kept_bytes / 2**20, a, b, b_lo, b_hi,
        " / ".join("%.3f" % res[f] for f in forms if f), c, c / b, b - a, d, gbs))
    print(lines[-1], flush=True)


def set_cell(lib, pats, batch, name, lines):
    s = M.compile_set(pats)
    for mode in ("any", "all"):
        m = timed(lambda: s.matches(batch), reps=5)
        f = timed(lambda: s.filter(batch, mode=mode), reps=5)
        kb, _ = s.filter(batch, mode=mode)
        lines.append("| %s | %d | %s | %d | %.3f | %.3f | %.3f |" % (name, len(pats), mode, kb.n, m, f, f - m))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "filter.md"))
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_filter.py measures on a GPU"
    lib = M.load_library()
    rx = M.compile_regex(NEEDLE)
    k = 64 if args.small else 1
    lines = ["| shape | kept | kept MiB | (a) search ms | (b) filter ms | (b) again: fastest - slowest of 10 | (b) block form / text form ms | (c) torch ms | (c)/(b) "
             "| (b)-(a) ms | (d) copy ms | gather GB/s |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    n1, n3, n4 = (1 << 20) // k, (1 << 22) // k, max(256 // k, 8)
    head50 = None
    for frac in (0.01, 0.5, 0.99):
        data = make_pitch(n1, 1024, frac, 1)
        b = M.DeviceBatch.strided(data, 1024, length=1024)
        cell(lib, rx, b, "%d x 1 KiB, fixed pitch" % n1, frac, lines)
        cell(lib, rx, ragged_of(data, n1, 1024, 64, 1024, 2), "%d ragged CSR, U[64, 1024]" % n1, frac, lines)
        if frac == 0.5:
            head50 = b
        else:
            del data, b
        data = make_pitch(n3, 64, frac, 3)
        cell(lib, rx, M.DeviceBatch.strided(data, 64, length=64), "%d x 64 B, fixed pitch" % n3, frac, lines)
        del data
        data = make_pitch(n4, 4 << 20, frac, 4)
        cell(lib, rx, M.DeviceBatch.strided(data, 4 << 20, length=4 << 20), "%d x 4 MiB, fixed pitch" % n4, frac, lines)
        del data
        torch.cuda.empty_cache()
    sets = ["", "| batch | k | mode | kept | matches ms | filter ms | filter - matches ms |", "|---|---|---|---|---|---|---|"]
    # h, e, l and o are not in the alphabet: every member hits exactly the rows that hold the needle, so any and all
    # both keep about half the texts (a member that hits every text, or none, would decide the fraction by itself)
    words = [NEEDLE, b"^hel", b"llo", b"ello", b"h[a-z]+o", b"l+", b"he"]
    set_cell(lib, words, head50, "%d x 1 KiB, 50%% hold the needle" % n1, sets)
    set_cell(lib, words + [b"hel|w%02dq" % j for j in range(57)], head50, "%d x 1 KiB, 50%% hold the needle" % n1, sets)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + sets) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
