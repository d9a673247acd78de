#!/usr/bin/env python3
"""extract on one GPU (profiles/extract.md): per case
  (a) the spans alone -- findall (split_dev for the split case): the floor, it is part of the call;
  (b) extract / split_batch;
  (c) what the public API offered before: (a), then a gather built from torch ops -- repeat_interleave for the owners,
      a cumulative sum for the output CSR, a ranged index for the bytes;
  (d) a plain device copy of as many bytes as the pieces hold.
Cases: the headline batch ([a-z]+\\d+ on 2^20 x 1 KiB, fixed pitch), the same rows cut to a ragged CSR batch of
64..1024-byte texts, and split_batch of "," on a few 4 MiB texts.  Times are medians of device-event timings after
warm-up, (b) with its fastest and slowest call; every result is compared with (c)'s before it is timed.

  python tools/bench_extract.py [--out TABLE.md] [--small] [--only-extract]

The table is printed; --out also writes it to a file (profiles/extract.md is a write-up around a copy of it: do not
point --out at it).
"""
import argparse
import os
import statistics
import sys

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


def ragged_of(data, n, L, lo, hi, seed):
    """The rows cut to lengths U[lo, hi] and packed: a CSR batch with known bounds."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lens = torch.randint(lo, hi + 1, (n,), device="cuda", generator=g)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), lens, output_size=total)
    src = row * L + (torch.arange(total, device="cuda") - off[:-1][row])
    return M.DeviceBatch.csr_known(data[src], off, total, hi)


def text_starts(batch):
    if batch.offsets is not None:
        return batch.offsets[:-1]
    return torch.arange(batch.n, device=batch.data.device, dtype=torch.int64) * batch.stride


def torch_gather(batch, prefix, spans):
    """(c) behind the spans: (owner, out_offsets, bytes) from torch ops."""
    m = spans.shape[0]
    dev = batch.data.device
    owner = torch.repeat_interleave(torch.arange(batch.n, device=dev), prefix[1:] - prefix[:-1], output_size=m)
    s = spans[:, 0].to(torch.int64)
    lens = spans[:, 1].to(torch.int64) - s
    out_off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    out_off[1:] = torch.cumsum(lens, 0)
    total = int(out_off[-1])
    shift = text_starts(batch)[owner] + s - out_off[:-1]
    src = torch.repeat_interleave(shift, lens, output_size=total) + torch.arange(total, device=dev)
    return owner, out_off, batch.data[src]


def cell(name, batch, spans_fn, extract_fn, lines):
    """spans_fn() -> (prefix, spans[m, 2]); extract_fn() -> (pieces, prefix, owner)."""
    prefix, spans = spans_fn()
    owner, out_off, want = torch_gather(batch, prefix, spans)
    pieces, _, got_owner = extract_fn()
    assert torch.equal(pieces.data, want) and torch.equal(pieces.offsets, out_off) and torch.equal(got_owner, owner), name
    m, nbytes = int(spans.shape[0]), int(want.numel())
    del owner, out_off, want, pieces, got_owner
    a, _, _ = timed(spans_fn)
    b, b_lo, b_hi = timed(extract_fn)
    c, _, _ = timed(lambda: torch_gather(batch, *spans_fn()), warmup=2, reps=5)
    dst = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    d, _, _ = timed(lambda: dst[:nbytes].copy_(batch.data[:nbytes]))
    lines.append("| %s | %d | %.1f | %.1f | %.3f | %.3f | %.3f - %.3f | %.3f | %.2fx | %.3f | %.3f |" % (
        name, m, nbytes / 2**20, nbytes / max(m, 1), a, b, b_lo, b_hi, c, c / b, b - a, d))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--only-extract", action="store_true",
                    help="run extract of the headline batch a few times and stop (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_extract.py measures on a GPU"
    k = 64 if args.small else 1
    n, L = (1 << 20) // k, 1024
    rx = M.compile_regex(b"[a-z]+\\d+")
    data = make_c2_batch(n, L).reshape(-1)
    head = M.DeviceBatch.strided(data, L, length=L)
    if args.only_extract:
        for _ in range(5):
            pieces, _, _ = rx.extract(head)
        torch.cuda.synchronize()
        print("pieces %d bytes %d" % (pieces.n, pieces.data.numel()))
        return
    lines = ["| case | pieces | MiB out | bytes a piece | (a) spans ms | (b) extract ms | (b) fastest - slowest of 10 | (c) torch ms "
             "| (c)/(b) | (b)-(a) ms | (d) copy ms |", "|---|---|---|---|---|---|---|---|---|---|---|"]

    def spans_of(batch):
        p, s, t = rx._dev_findall(batch)
        return p, s[:t]

    cell("%d x 1 KiB, fixed pitch, [a-z]+\\d+" % n, head, lambda: spans_of(head), lambda: rx.extract(head), lines)
    rag = ragged_of(data, n, L, 64, 1024, 2)
    cell("%d ragged CSR, U[64, 1024], [a-z]+\\d+" % n, rag, lambda: spans_of(rag), lambda: rx.extract(rag), lines)
    del rag, head, data
    torch.cuda.empty_cache()
    # a few 4 MiB texts of comma separated fields of 1..2000 bytes
    comma = M.compile_regex(b",")
    nt, big = 8, (4 << 20) // k
    g = torch.Generator(device="cuda").manual_seed(7)
    body = torch.randint(97, 123, (nt * big,), device="cuda", generator=g, dtype=torch.uint8)
    cuts = torch.randint(0, nt * big, (nt * big // 1000,), device="cuda", generator=g)
    body[cuts] = ord(",")
    texts = M.DeviceBatch.strided(body, big, length=big)

    def split_spans():
        p, s, t = comma.split_dev(texts)
        return p, s[:t]

    cell("%d x %d KiB, split on ','" % (nt, big >> 10), texts, split_spans, lambda: comma.split_batch(texts), lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
