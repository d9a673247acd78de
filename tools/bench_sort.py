#!/usr/bin/env python3
"""sort and take on one GPU (profiles/sort.md), on the cases of tools/bench_distinct.py: per case
  (s) DeviceBatch.argsort(), the whole call (its kernels, the scans, the allocation of the order and one read-back of a
      word per refinement round), with its fastest and slowest call and the number of rounds;
  (r) argsort(rank=True): the same with the dense ranks and the distinct count;
  (t) DeviceBatch.take(order): the texts moved into that order;
  (v) the value_counts(sort="value") path: argsort and take of the case's distinct values;
  (a) what a user has today: the pieces copied to the host and sorted() -- the copy, building the bytes objects and
      the sort, timed with the host clock.  It is measured on the first --host-pieces pieces of a case (default 2^21, an
      eighth) and reported per million pieces;
  (b) where no piece is longer than 32 bytes: the rows padded to 32 bytes on the device, read as four big-endian int64
      columns (the sign bit flipped, so that the signed comparison is the unsigned one) and ordered by four stable
      torch.sort passes from the last column to the first, the padding included.  Where all pieces have one length its
      order must equal argsort's (checked);
  (f) take of every text in its place (an identity index) against filter with every text kept, on the same bytes;
  (d) a plain device copy of the input's bytes, for scale.
(s), (r), (t), (v), (b), (f) and (d) are medians of 10 device-event timings after warm-up.  Every order is checked before
it is timed: it is a permutation, neighbours in it do not decrease (compared on the device through their ranks and, on
a sample, bytewise on the host), equal texts keep index order, and the rank agrees with distinct's groups.

  python tools/bench_sort.py [--out TABLE.md] [--small] [--case NAME] [--only-sort]

--only-sort runs five calls of (s) per case and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the kernel rows.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402
from bench_distinct import CASES, timed  # noqa: E402

SORT_CASES = ("headline", "zipf", "equal", "unique")


def host_texts(batch, idx):
    """The texts at the indices idx (a list) as bytes objects."""
    if batch.offsets is None:
        rows = batch.data.view(batch.n, batch.stride)[torch.tensor(idx, device="cuda")].cpu().numpy()
        return [rows[j, :batch.length].tobytes() for j in range(len(idx))]
    off = batch.offsets.cpu().numpy()
    raw = batch.data.cpu().numpy()
    return [raw[off[i]:off[i + 1]].tobytes() for i in idx]


def check(batch, order, rank, u):
    n = batch.n
    assert bool((torch.sort(order).values == torch.arange(n, device="cuda")).all()), "not a permutation"
    along = rank[order]
    assert bool((along[1:] >= along[:-1]).all()) and int(along[0]) == 0 and int(along[-1]) == u - 1
    same = along[1:] == along[:-1]
    assert bool((order[1:][same] > order[:-1][same]).all()), "equal texts left their index order"
    values, _, group_of, first = batch.distinct()
    assert values.n == u
    assert bool((rank[first][group_of] == rank).all()), "texts of one distinct group have different ranks"
    assert int(torch.unique(rank[first]).numel()) == u, "two distinct groups share a rank"
    step = max(1, n // 4096)
    at = list(range(0, n - 1, step))
    left, right = host_texts(batch, order[at].tolist()), host_texts(batch, order[[p + 1 for p in at]].tolist())
    assert all(a <= b for a, b in zip(left, right)), "neighbours in the order decrease"


def host_sorted(batch, m):
    """Seconds for the first m pieces: copy to the host, bytes objects, sorted()."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if batch.offsets is None:
        raw = batch.data[:m * batch.stride].cpu().numpy().tobytes()
        out = sorted(raw[i * batch.stride:i * batch.stride + batch.length] for i in range(m))
    else:
        off = batch.offsets[:m + 1].cpu().numpy()
        raw = batch.data[:int(off[-1])].cpu().numpy().tobytes()
        out = sorted(raw[off[i]:off[i + 1]] for i in range(m))
    return time.perf_counter() - t0, len(out)


def padded_columns(batch):
    """The pieces as rows of 32 bytes, zero padded, read as four big-endian int64 columns with the sign bit flipped."""
    n = batch.n
    rows = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    if batch.offsets is None:
        rows[:, :batch.length] = batch.data.view(n, batch.stride)[:, :batch.length]
    else:
        off = batch.offsets
        lens = off[1:] - off[:-1]
        total = int(batch.data.numel())
        row = torch.repeat_interleave(torch.arange(n, device="cuda"), lens, output_size=total)
        rows[row, torch.arange(total, device="cuda") - off[:-1][row]] = batch.data
    cols = rows.view(n, 4, 8).flip(2).contiguous().view(torch.int64).view(n, 4)   # (the device is little-endian)
    return cols ^ (-1 << 63)


def torch_route(batch):
    cols = padded_columns(batch)
    order = torch.arange(batch.n, device="cuda")
    for c in (3, 2, 1, 0):
        order = order[torch.sort(cols[order, c], stable=True).indices]
    return order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--case", choices=list(SORT_CASES), action="append")
    ap.add_argument("--only-sort", action="store_true")
    ap.add_argument("--host-pieces", type=int, default=1 << 21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sort.py measures on a GPU"
    lib = M.load_library()
    k = 64 if args.small else 1
    lines = ["| case | texts | distinct | MiB in | rounds | (s) argsort ms | (s) fastest - slowest of 10 | M texts/s | (r) with rank ms | "
             "(t) take(order) ms | (v) sort of the distinct values ms (rounds) | (a) host sorted(), s per million pieces (pieces timed) "
             "| (b) four torch.sort passes on 32-byte rows ms | (b)/(s) | (f) take in place ms / filter keeping all ms | (d) copy ms | (s)/(d) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in args.case or list(SORT_CASES):
        title, batch, _ = CASES[name](k)
        order, rank, u = batch.argsort(rank=True)
        rounds = lib.mrx_debug_sort_rounds()
        check(batch, order, rank, u)
        nbytes = int(batch.data.numel())
        del rank
        if args.only_sort:
            for _ in range(5):
                batch.argsort()
            torch.cuda.synchronize()
            print("%s: %d texts, %d distinct, %d rounds, 5 calls" % (title, batch.n, u, rounds), flush=True)
            continue
        s, s_lo, s_hi = timed(lambda: batch.argsort())
        r = timed(lambda: batch.argsort(rank=True))[0]
        t = timed(lambda: batch.take(order))[0]
        values = batch.distinct()[0]
        v = timed(lambda: values.take(values.argsort()))[0]
        v_rounds = lib.mrx_debug_sort_rounds()
        del values
        m = min(batch.n, args.host_pieces // k)
        secs, _ = host_sorted(batch, m)
        lens = None if batch.offsets is None else batch.offsets[1:] - batch.offsets[:-1]
        longest = batch.length if lens is None else int(lens.max())
        if longest <= 32:
            if lens is None or int(lens.min()) == longest:   # one length: no "a" against "a\0", the orders must agree
                assert torch.equal(torch_route(batch), order), "the torch route gives another order"
            b = timed(lambda: torch_route(batch), warmup=1, reps=3)[0]
            b_txt, ratio = "%.1f" % b, "%.1fx" % (b / s)
        else:
            b_txt, ratio = "not applicable: pieces of up to %d bytes" % longest, ""
        ident = torch.arange(batch.n, dtype=torch.int64, device="cuda")
        f_take = timed(lambda: batch.take(ident))[0]
        if name == "unique":   # arbitrary bytes: no pattern keeps them all; a dictionary without entries, inverted, does
            keep_all = M.Dictionary([])
            assert keep_all.filter(batch, invert=True)[0].n == batch.n
            f_filter, how = timed(lambda: keep_all.filter(batch, invert=True))[0], "empty dictionary, inverted"
        else:
            rx = M.compile_regex(b"[a-z]")
            assert rx.filter(batch)[0].n == batch.n
            f_filter, how = timed(lambda: rx.filter(batch))[0], "[a-z]"
        del ident
        dst = torch.empty_like(batch.data)
        d = timed(lambda: dst.copy_(batch.data))[0]
        del dst
        lines.append("| %s | %d | %d | %.1f | %d | %.3f | %.3f - %.3f | %.0f | %.3f | %.3f | %.3f (%d) | %.2f (%d) | %s | %s | "
                     "%.3f / %.3f (%s) | %.3f | %.1fx |" % (
                         title, batch.n, u, nbytes / 2**20, rounds, s, s_lo, s_hi, batch.n / s / 1e3, r, t, v, v_rounds,
                         secs / m * 1e6, m, b_txt, ratio, f_take, f_filter, how, d, s / d))
        print(lines[-1], flush=True)
        del batch, order
        torch.cuda.empty_cache()
    if not args.only_sort:
        print("\n".join(lines))
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
            print("wrote", args.out)


if __name__ == "__main__":
    main()
