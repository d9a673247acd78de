#!/usr/bin/env python3
"""Quoted fields on one GPU (profiles/fields_quoted.md).  Inputs, all generated on the device from a seed, the first and
the last as tools/bench_fields.py makes them:
  csv          256 MiB of letters with b"," every U[5, 15] bytes and a newline every U[80, 120], cut by from_lines;
               no quote byte in it
  csv, quoted  the same bytes with every third cell of 5 bytes or more set in quotes and a comma put inside it
  log, quoted  1 GiB shaped as csv with a space for the comma, about 10^7 lines of 8 to 12 fields, every fifth cell (two
               a line) in quotes with a space inside; timed in whitespace mode and with delim=b" "
  headline     the headline batch, 2^20 rows of 1 KiB, in whitespace mode as it is
Per input, columns [1, 4, 10] with counts and [2] without; the routes take turns in one process, each the median
(fastest - slowest) of 7 device-event timings after 2 warm-up calls:
  quoted      DeviceBatch.fields_async(quote=b'"') on the caller's tensors, with the quoted bytes
  no bytes    the same without them (quoted=None)
  plain       DeviceBatch.fields_async on the same bytes: other answers where there are quotes, the same reads
  copy        a plain device copy of the input's bytes
and, on the host, csv.reader over an eighth of the rows (wall clock, once, the bytes already on the host).
Before anything is timed, quoted fields is compared with plain fields on the input without quotes.

  python tools/bench_fields_quoted.py [--out TABLE.md] [--small] [--plain-only]

--plain-only times plain fields alone and prints one line per row: with MRX_LIB set to a build of another commit this
is the A/B that shows whether plain fields got slower.
"""
import argparse
import csv
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch  # noqa: E402
from bench_fields import field_buffer, fmt, timed_alternating  # noqa: E402

REQUESTS = (([1, 4, 10], True), ([2], False))
Q = b'"'


def quote_cells(data, sep, every):
    """Sets every `every`-th cell of 5 bytes or more in quotes, in place, and puts a separator inside it."""
    at = torch.nonzero((data == sep) | (data == 10)).reshape(-1)
    a, b = at[:-1][::every], at[1:][::every]
    ok = b - a >= 6
    a, b = a[ok], b[ok]
    data[a + 1] = Q[0]
    data[b - 1] = Q[0]
    data[a + 3] = sep
    return int(a.numel())


def host_reader_ms(batch, delim):
    """csv.reader over an eighth of the batch's rows, in ms (wall clock; the rows are str lines already)."""
    n = max(batch.n // 8, 1)
    if batch.offsets is not None:
        off = batch.offsets[:n + 1].cpu().numpy()
        raw = batch.data[:int(off[-1])].cpu().numpy().tobytes()
        lines = [raw[off[i]:off[i + 1]].decode("latin-1") for i in range(n)]
    else:
        raw = batch.data[:n * batch.stride].cpu().numpy().tobytes()
        lines = [raw[i * batch.stride:i * batch.stride + batch.length].decode("latin-1") for i in range(n)]
    t0 = time.perf_counter()
    cells = sum(len(r) for r in csv.reader(lines, delimiter=(delim or b" ").decode()))
    return (time.perf_counter() - t0) * 1e3, n, cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fields_quoted.py measures on a GPU"
    k = 64 if args.small else 1
    out_lines = []

    def say(line):
        out_lines.append(line)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(out_lines) + "\n")

    csv_data = field_buffer((1 << 28) // k, 44, 2)
    plain_csv = M.DeviceBatch.from_lines(csv_data)
    quoted_data = csv_data.clone()
    n_csv = quote_cells(quoted_data, 44, 3)
    quoted_csv = M.DeviceBatch.from_lines(quoted_data)
    log_data = field_buffer((1 << 30) // k, 32, 1)
    n_log = quote_cells(log_data, 32, 5)
    log = M.DeviceBatch.from_lines(log_data)
    c2 = make_c2_batch((1 << 20) // k)
    inputs = [
        ("csv: %d lines, no quote in them, delim b\",\"" % plain_csv.n, plain_csv, b","),
        ("csv, %d cells quoted, delim b\",\"" % n_csv, quoted_csv, b","),
        ("log: %d lines, %d cells quoted, whitespace" % (log.n, n_log), log, None),
        ("log, delim b\" \"", log, b" "),
        ("headline batch: %d rows of 1 KiB, whitespace" % c2.shape[0], M.DeviceBatch.strided(c2.reshape(-1), 1024, length=1024), None),
    ]

    if args.plain_only:
        for title, batch, delim in inputs:
            for cols, counts in REQUESTS:
                out = (torch.empty(batch.n + 1, dtype=torch.int64, device="cuda"),
                       torch.empty((batch.n, len(cols), 2), dtype=torch.int32, device="cuda"),
                       torch.empty(batch.n, dtype=torch.int32, device="cuda") if counts else None)
                t = timed_alternating([lambda: batch.fields_async(out, cols, delim)])[0]
                say("plain | %s | %s | %s | %s" % (title, cols, "yes" if counts else "no", fmt(t)))
                del out
        return

    # without a quote byte in the input, quoted fields gives plain fields' rows
    for cols, counts in REQUESTS:
        _, rows, nf = plain_csv.fields(cols, b",", counts=counts)
        _, qrows, qnf, quoted = plain_csv.fields(cols, b",", counts=counts, quote=Q)
        assert torch.equal(rows, qrows) and not bool(quoted.any()) and (not counts or torch.equal(nf, qnf)), cols
        del rows, nf, qrows, qnf, quoted
    torch.cuda.empty_cache()

    say("Times in ms: median (fastest - slowest) of 7 calls after 2 warm-up calls, the routes of a row taking turns; the "
        "slower of quoted and plain in bold.  csv.reader: wall clock of one pass over an eighth of the rows on the host, "
        "and that time taken times eight.\n")
    say("| input | MiB | columns | counts | quoted | quoted, no bytes | plain fields | copy | quoted / plain | quoted / copy | "
        "GiB/s | csv.reader, 1/8 of the rows | x 8 / quoted |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for title, batch, delim in inputs:
        mib = batch.data.numel() / 2**20
        dst = torch.empty_like(batch.data)
        host_ms, host_n, host_cells = host_reader_ms(batch, delim)
        for cols, counts in REQUESTS:
            out = (torch.empty(batch.n + 1, dtype=torch.int64, device="cuda"),
                   torch.empty((batch.n, len(cols), 2), dtype=torch.int32, device="cuda"),
                   torch.empty(batch.n, dtype=torch.int32, device="cuda") if counts else None)
            qb = torch.empty((batch.n, len(cols)), dtype=torch.uint8, device="cuda")
            tq, tn, tp, tc = timed_alternating([
                lambda: batch.fields_async(out + (qb,), cols, delim, quote=Q),
                lambda: batch.fields_async(out + (None,), cols, delim, quote=Q),
                lambda: batch.fields_async(out, cols, delim),
                lambda: dst.copy_(batch.data)])
            bold = lambda t, other: ("**%s**" if t[0] > other[0] else "%s") % fmt(t)   # noqa: E731
            say("| %s | %.0f | %s | %s | %s | %s | %s | %s | %.2fx | %.2fx | %.0f | %.0f ms (%d rows, %d cells) | %.0fx |" % (
                title, mib, cols, "yes" if counts else "no", bold(tq, tp), fmt(tn), bold(tp, tq), fmt(tc), tq[0] / tp[0],
                tq[0] / tc[0], mib / 1024 / (tq[0] / 1e3), host_ms, host_n, host_cells, 8 * host_ms / tq[0]))
            del out, qb
        del dst
        torch.cuda.empty_cache()
    if args.out:
        print("wrote", args.out)


if __name__ == "__main__":
    main()
