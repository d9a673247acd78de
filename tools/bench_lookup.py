#!/usr/bin/env python3
"""Dictionaries on one GPU (profiles/lookup.md): per case
  (a) the build (Dictionary(entries): distinct's first three kernels, a fix-up, the packed copy, two synchronisations and
      three hipMallocs), timed with the host clock around a call that ends synchronised;
  (b) the lookup, one kernel (Dictionary.lookup_async into a tensor of the caller), with its fastest and slowest call;
  (c) the filter (Dictionary.filter: the lookup, a flags kernel, filter's scans, scatter and gather, one read-back);
  (d) the route the API offered before: the entries concatenated in front of the batch, distinct over the whole, and
      first[group_of[m + i]] < m read as "text i is an entry" -- the concatenation, the distinct call and the three
      torch operations that derive the index, all timed;
  (e) a plain device copy of the probed bytes, for scale.
Cases: distinct's -- the extract pieces of the headline batch ([a-z]+\\d+ on 2^20 x 1 KiB), a Zipf-distributed vocabulary
of about 10^5 words over 2^24 pieces, 2^24 equal pieces, 2^24 distinct pieces -- each against a dictionary of every
other one of its own values (the measured hit rate is in the table); and a sweep over the dictionary's size and the hit
rate: 2^24 probes of 8 bytes drawn uniformly from m / rate keys of which the first m are the entries, m from 10^2 to 10^7
and the rate about 1 %, 50 % and 99 %.
(b) to (e) are medians of device-event timings after warm-up.  Every lookup result is checked before it is timed: it
equals route (d)'s result element for element, the filter keeps exactly the texts with an index, and in the sweep the
index of a hit is the key itself.

  python tools/bench_lookup.py [--out TABLE.md] [--small] [--case NAME] [--only-lookup]

--only-lookup runs five lookups per case and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mojo_regex_amd as M  # noqa: E402
from bench_distinct import case_equal, case_headline, case_unique, case_zipf, timed  # noqa: E402

ODD = 0x1E3779B97F4A7C15   # (odd: a bijection of 64 bits)


def as_csr(batch):
    """(data, offsets) of a batch whose rows are whole (a CSR batch as it is)."""
    return batch.data, batch.csr_offsets()


def csr_take(batch, picks):
    """The CSR batch of texts picks[0], picks[1], ... of a CSR batch, built on the device."""
    data, off = as_csr(batch)
    lens = (off[1:] - off[:-1])[picks]
    new_off = torch.zeros(picks.numel() + 1, dtype=torch.int64, device="cuda")
    new_off[1:] = torch.cumsum(lens, 0)
    total = int(new_off[-1])
    row = torch.repeat_interleave(torch.arange(picks.numel(), device="cuda"), lens, output_size=total)
    src = off[:-1][picks][row] + (torch.arange(total, device="cuda") - new_off[:-1][row])
    return M.DeviceBatch.csr_known(data[src], new_off, total, int(lens.max()) if picks.numel() else 0)


def own_values(make):
    """A case of bench_distinct.py against every other one of its own values (and one text that is no value)."""
    def case(k):
        title, batch, _ = make(k)
        values = batch.distinct()[0]
        entries = csr_take(values, torch.arange(0, values.n, 2, device="cuda"))
        return title + ", every other value", entries, batch, None
    return case


def sweep(m, rate):
    def case(k):
        n, mm = (1 << 24) // k, max(m // k, 2)
        g = torch.Generator(device="cuda").manual_seed(m * 100 + int(rate * 100))
        universe = max(int(mm / rate), mm + 1)
        picks = torch.randint(0, universe, (n,), dtype=torch.int64, device="cuda", generator=g)
        probes = M.DeviceBatch.strided((picks * ODD).view(torch.uint8), 8, length=8)
        entries = M.DeviceBatch.strided((torch.arange(mm, dtype=torch.int64, device="cuda") * ODD).view(torch.uint8), 8, length=8)
        return "%d keys of 8 bytes, uniform over %d" % (n, universe), entries, probes, torch.where(picks < mm, picks, -1)
    return case


CASES = {"headline": own_values(case_headline), "zipf": own_values(case_zipf), "equal": own_values(case_equal),
         "unique": own_values(case_unique)}
for _m in (100, 10**4, 10**6, 10**7):
    for _r in (0.01, 0.5, 0.99):
        CASES["m%d_hit%d" % (_m, round(_r * 100))] = sweep(_m, _r)


def old_route(entries, batch):
    """What the API offered before dictionaries: int64[n], the index of every text in `entries` or -1."""
    edata, eoff = as_csr(entries)
    data, off = as_csr(batch)
    m = entries.n
    both = M.DeviceBatch(torch.cat([edata, data]), torch.cat([eoff, off[1:] + eoff[-1]]))   # (both begin at offset 0)
    _, _, group_of, first = both.distinct()
    f = first[group_of[m:]]
    return torch.where(f < m, f, torch.full_like(f, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--case", choices=list(CASES), action="append")
    ap.add_argument("--only-lookup", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lookup.py measures on a GPU"
    k = 64 if args.small else 1
    lines = ["| case | probes | entries | different | hit rate | MiB probed | (a) build ms | (b) lookup ms | (b) fastest - slowest of 10 | "
             "M texts/s | (c) filter ms | (d) concatenate + distinct ms | (d)/(b) | (d)/(c) | (e) copy ms | (b)/(e) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in args.case or list(CASES):
        title, entries, batch, known = CASES[name](k)
        d = M.Dictionary(entries)
        index = torch.empty(batch.n, dtype=torch.int64, device="cuda")
        d.lookup_async(batch, index)
        torch.cuda.synchronize()
        if args.only_lookup:
            for _ in range(5):
                d.lookup_async(batch, index)
            torch.cuda.synchronize()
            print("%s: %d probes, %d entries, 5 lookups" % (title, batch.n, len(d)), flush=True)
            continue
        # the checks, before anything is timed
        route = old_route(entries, batch)
        assert torch.equal(index, route), "the lookup and the concatenate-then-distinct route differ"
        if known is not None:
            assert torch.equal(index, known)
        kept, kept_idx = d.filter(batch)
        assert torch.equal(kept_idx, torch.nonzero(index >= 0).reshape(-1)) and kept.n == kept_idx.numel()
        hits = int((index >= 0).sum())
        del route, kept, kept_idx
        builds = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tmp = M.Dictionary(entries)
            torch.cuda.synchronize()
            builds.append((time.perf_counter() - t0) * 1e3)
            del tmp
        a = statistics.median(builds[1:])
        b, b_lo, b_hi = timed(lambda: d.lookup_async(batch, index))
        c = timed(lambda: d.filter(batch))[0]
        r = timed(lambda: old_route(entries, batch), warmup=1, reps=3)[0]
        dst = torch.empty_like(batch.data)
        e = timed(lambda: dst.copy_(batch.data))[0]
        del dst
        lines.append("| %s | %d | %d | %d | %.1f %% | %.1f | %.3f | %.3f | %.3f - %.3f | %.0f | %.3f | %.3f | %.1fx | %.1fx | %.3f | %.1fx |" % (
            title, batch.n, len(d), d.distinct_count, 100.0 * hits / max(batch.n, 1), batch.data.numel() / 2**20, a, b, b_lo, b_hi,
            batch.n / b / 1e3, c, r, r / b, r / c, e, b / e))
        print(lines[-1], flush=True)
        del d, entries, batch, index, known
        torch.cuda.empty_cache()
    if not args.only_lookup:
        print("\n".join(lines))
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
            print("wrote", args.out)


if __name__ == "__main__":
    main()
