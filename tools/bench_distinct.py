#!/usr/bin/env python3
"""distinct on one GPU (profiles/distinct.md): per case
  (a) distinct, the whole call (DeviceBatch.distinct: five kernels of its own, two scans, filter's gather, one
      read-back of the totals), with its fastest and slowest call;
  (b) the pieces copied to the host and counted with collections.Counter -- the copy, and building and counting the
      bytes objects, timed with the host clock around work that ends in a synchronise.  It is measured on the first
      --host-pieces pieces of a case (default 2^21) and reported per million pieces: the whole of 2^24 pieces takes
      the better part of a minute;
  (c) torch.unique(dim=0, return_counts=True) on the pieces padded to 32-byte rows on the device, the padding
      included, where no piece is longer than 32 bytes;
  (d) a plain device copy of the input's bytes, for scale.
Cases: the extract pieces of the headline batch ([a-z]+\\d+ on 2^20 x 1 KiB); a Zipf-distributed vocabulary of about
10^5 words over 2^24 pieces; 2^24 equal pieces; 2^24 distinct pieces; 2^16 texts of 4 KiB of which half are duplicates.
(a), (c) and (d) are medians of device-event timings after warm-up.  Every distinct result is checked before it is
timed: the counts add up to n, first increases, distinct of the values finds them all distinct, and where the case knows
its answer (the vocabulary picks, the 8-byte pieces as int64) the number of groups and the sorted counts are compared
with torch's.

  python tools/bench_distinct.py [--out TABLE.md] [--small] [--case NAME] [--only-distinct]

--only-distinct runs five calls of (a) per case and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the kernel rows.
"""
import argparse
import collections
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch  # noqa: E402


def timed(fn, warmup=3, reps=10):
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


def csr_of_picks(vocab, picks):
    """The CSR batch whose text i is vocab[picks[i]], built on the device."""
    vdata, voff = M.pack_texts(vocab)
    vdata, voff = torch.from_numpy(vdata).cuda(), torch.from_numpy(voff).cuda()
    vlen = voff[1:] - voff[:-1]
    lens = vlen[picks]
    off = torch.zeros(picks.numel() + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    row = torch.repeat_interleave(torch.arange(picks.numel(), device="cuda"), lens, output_size=total)
    src = voff[:-1][picks][row] + (torch.arange(total, device="cuda") - off[:-1][row])
    return M.DeviceBatch.csr_known(vdata[src], off, total, int(vlen.max()))


def case_headline(k):
    n = (1 << 20) // k
    rx = M.compile_regex(b"[a-z]+\\d+")
    pieces = rx.extract(M.DeviceBatch.strided(make_c2_batch(n).reshape(-1), 1024, length=1024))[0]
    pieces = M.DeviceBatch.csr_known(pieces.data.clone(), pieces.offsets.clone(), pieces._end_offset, pieces._max_len)
    return "extract pieces of %d x 1 KiB, [a-z]+\\d+" % n, pieces, None


def case_zipf(k):
    n, v = (1 << 24) // k, 100000 // k
    rng = np.random.default_rng(20260302)
    vocab = list(dict.fromkeys(bytes(rng.integers(97, 123, size=int(rng.integers(2, 13))).tolist()) for _ in range(2 * v)))[:v]
    picks = torch.from_numpy(np.minimum(rng.zipf(1.2, size=n) - 1, len(vocab) - 1)).cuda()
    return "Zipf(1.2) over %d words, %d pieces" % (len(vocab), n), csr_of_picks(vocab, picks), picks


def case_equal(k):
    n = (1 << 24) // k
    data = torch.tensor(list(b"error503"), dtype=torch.uint8, device="cuda").repeat(n)
    return "%d equal pieces of 8 bytes" % n, M.DeviceBatch.strided(data, 8, length=8), torch.zeros(n, dtype=torch.int64, device="cuda")


def case_unique(k):
    n = (1 << 24) // k
    keys = torch.arange(n, dtype=torch.int64, device="cuda") * 0x1E3779B97F4A7C15   # (odd: a bijection of 64 bits)
    return "%d distinct pieces of 8 bytes" % n, M.DeviceBatch.strided(keys.view(torch.uint8), 8, length=8), keys


def case_4k(k):
    n = (1 << 16) // k
    g = torch.Generator(device="cuda").manual_seed(7)
    half = torch.randint(0, 256, (n // 2, 4096), dtype=torch.uint8, device="cuda", generator=g)
    perm = torch.randperm(n // 2, device="cuda", generator=g)
    data = torch.cat([half, half[perm]]).reshape(-1)
    picks = torch.cat([torch.arange(n // 2, device="cuda"), perm])
    return "%d texts of 4 KiB, half of them duplicates" % n, M.DeviceBatch.strided(data, 4096, length=4096), picks


CASES = {"headline": case_headline, "zipf": case_zipf, "equal": case_equal, "unique": case_unique, "4k": case_4k}


def check(batch, res, picks):
    values, counts, group_of, first = res
    assert int(counts.sum()) == batch.n and bool((first[1:] > first[:-1]).all())
    assert int(group_of.max()) == values.n - 1 and bool((group_of[first] == torch.arange(values.n, device="cuda")).all())
    again = values.distinct()
    assert again[0].n == values.n and bool((again[1] == 1).all()), "the values are not distinct"
    if picks is not None:   # the case knows which texts are equal
        _, inv, cnt = torch.unique(picks, return_inverse=True, return_counts=True)
        assert values.n == cnt.numel()
        assert torch.equal(torch.sort(counts).values, torch.sort(cnt).values)
        assert torch.equal(counts[group_of], cnt[inv])   # every text's group has the size of its pick's


def padded_rows(batch):
    """The pieces as rows of 32 bytes, zero padded, with the length in a 33rd byte (so that "a" and "a\\0" differ)."""
    n = batch.n
    if batch.offsets is None:
        rows = torch.zeros((n, 33), dtype=torch.uint8, device="cuda")
        rows[:, :batch.length] = batch.data.view(n, batch.stride)[:, :batch.length]
        rows[:, 32] = batch.length
        return rows
    off = batch.offsets
    lens = off[1:] - off[:-1]
    total = int(batch.data.numel())
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), lens, output_size=total)
    col = torch.arange(total, device="cuda") - off[:-1][row]
    rows = torch.zeros((n, 33), dtype=torch.uint8, device="cuda")
    rows[row, col] = batch.data
    rows[:, 32] = lens.to(torch.uint8)
    return rows


def host_counter(batch, m):
    """Seconds for the first m pieces: copy to the host, bytes objects, collections.Counter."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if batch.offsets is None:
        raw = batch.data[:m * batch.stride].cpu().numpy().tobytes()
        c = collections.Counter(raw[i * batch.stride:i * batch.stride + batch.length] for i in range(m))
    else:
        off = batch.offsets[:m + 1].cpu().numpy()
        raw = batch.data[:int(off[-1])].cpu().numpy().tobytes()
        c = collections.Counter(raw[off[i]:off[i + 1]] for i in range(m))
    return time.perf_counter() - t0, len(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--case", choices=list(CASES), action="append")
    ap.add_argument("--only-distinct", action="store_true")
    ap.add_argument("--host-pieces", type=int, default=1 << 21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_distinct.py measures on a GPU"
    k = 64 if args.small else 1
    lines = ["| case | texts | groups | MiB in | MiB values | (a) distinct ms | (a) fastest - slowest of 10 | M texts/s | (b) host Counter, s per "
             "million pieces (pieces timed) | (c) torch.unique on 32-byte rows ms | (c)/(a) | (d) copy ms | (a)/(d) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in args.case or list(CASES):
        title, batch, picks = CASES[name](k)
        res = batch.distinct()
        check(batch, res, picks)
        u, vbytes, nbytes = res[0].n, int(res[0].data.numel()), int(batch.data.numel())
        del res
        if args.only_distinct:
            for _ in range(5):
                batch.distinct()
            torch.cuda.synchronize()
            print("%s: %d texts, %d groups, 5 calls" % (title, batch.n, u), flush=True)
            continue
        a, a_lo, a_hi = timed(lambda: batch.distinct())
        m = min(batch.n, args.host_pieces // k)
        secs, _ = host_counter(batch, m)
        longest = batch.length if batch.offsets is None else int((batch.offsets[1:] - batch.offsets[:-1]).max())
        if longest <= 32:
            def torch_route():
                return torch.unique(padded_rows(batch), dim=0, return_counts=True)
            assert torch_route()[0].shape[0] == u
            c = timed(torch_route, warmup=1, reps=3)[0]
            c_txt, ratio = "%.1f" % c, "%.1fx" % (c / a)
        else:
            c_txt, ratio = "not applicable: pieces of up to %d bytes" % longest, ""
        dst = torch.empty_like(batch.data)
        d = timed(lambda: dst.copy_(batch.data))[0]
        del dst
        lines.append("| %s | %d | %d | %.1f | %.1f | %.3f | %.3f - %.3f | %.0f | %.2f (%d) | %s | %s | %.3f | %.1fx |" % (
            title, batch.n, u, nbytes / 2**20, vbytes / 2**20, a, a_lo, a_hi, batch.n / a / 1e3, secs / m * 1e6, m, c_txt,
            ratio, d, a / d))
        print(lines[-1], flush=True)
        del batch, picks
        torch.cuda.empty_cache()
    if not args.only_distinct:
        print("\n".join(lines))
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
            print("wrote", args.out)


if __name__ == "__main__":
    main()
