#!/usr/bin/env python3
"""Fields on one GPU (profiles/fields.md).  Inputs, all generated on the device from a seed:
  log     a buffer of 1 GiB of letters with a space every U[5, 15] bytes and a newline every U[80, 120], cut by
          DeviceBatch.from_lines into about 10^7 lines of 8 to 12 fields (a CSR batch with known bounds); timed in
          whitespace mode and with delim=b" "
  ragged  2^20 rows of the headline batch cut to U[64, 1024] bytes and packed, one byte in ten a space
  rows64  2^24 rows of 64 bytes at a fixed pitch, spaces as in log
  c2      the headline batch, 2^20 rows of 1 KiB, in whitespace mode as it is
  csv     256 MiB shaped as log with b"," in the place of the space, delim=b","
Per input, columns [1], [1, 4, 10] and [-1], with and without counts; the routes take turns in one process, each the
median (fastest - slowest) of 7 device-event timings after 2 warm-up calls:
  fields    DeviceBatch.fields_async on the caller's tensors
  split     compile_regex(delim).split_dev with a capacity that fits, plus the index arithmetic in torch that picks the
            columns out of its ranges (delimiter mode, with counts: the route gives them anyway)
  captures  captures_all(count=1) of the equivalent (\\S+) \\S+ ... pattern (whitespace mode, positive columns)
  copy      a plain device copy of the input's bytes
Then G, the lanes that share a text, swept over the inputs.  Before anything is timed, fields is compared with the split
route on the csv input.

  python tools/bench_fields.py [--out TABLE.md] [--small]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch  # noqa: E402

COLUMNS = ([1], [1, 4, 10], [-1])


def timed_alternating(fns, warmup=2, reps=7):
    """Per function (median, fastest, slowest) in ms of `reps` device-event timings, the functions taking turns."""
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
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def fmt(t):
    return "%.3f (%.3f - %.3f)" % t


def field_buffer(nbytes, sep, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    data = torch.randint(97, 123, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
    for byte, lo, hi in ((sep, 5, 15), (10, 80, 120)):
        at = torch.cumsum(torch.randint(lo, hi + 1, (2 * nbytes // (lo + hi) + 1024,), device="cuda", generator=g), 0) - 1
        data[at[at < nbytes - 1]] = byte
        del at
    data[-1] = 10
    return data


def ragged_with_spaces(n, seed):
    """The headline batch's rows cut to U[64, 1024] bytes and packed, one byte in ten a space."""
    L = 1024
    data = make_c2_batch(n).reshape(-1).clone()
    g = torch.Generator(device="cuda").manual_seed(seed)
    data[torch.rand(data.numel(), device="cuda", generator=g) < 0.1] = 32
    lens = torch.randint(64, L + 1, (n,), device="cuda", generator=g)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), lens, output_size=total)
    src = row * L + (torch.arange(total, device="cuda") - off[:-1][row])
    return M.DeviceBatch.csr_known(data[src], off, total, L)


def split_route(rx, batch, cols, cap):
    """rows and nf as fields gives them, from split_dev's ranges and index arithmetic in torch."""
    pprefix, ranges, total = rx.split_dev(batch, piece_cap=cap)
    c = torch.tensor(cols, dtype=torch.int64, device="cuda")
    idx = torch.where(c > 0, pprefix[:-1, None] + c - 1, pprefix[1:, None] + c)
    ok = (idx < pprefix[1:, None]) & (idx >= pprefix[:-1, None])
    rows = torch.where(ok[..., None], ranges[idx.clamp(0, max(int(total) - 1, 0))], -1)
    return rows, (pprefix[1:] - pprefix[:-1]).to(torch.int32)


def capture_pattern(cols):
    """(\\S+) \\S+ ... with a group at every requested column: the first fields of a text, single spaces between them."""
    return b" ".join(b"(\\S+)" if k + 1 in cols else b"\\S+" for k in range(max(cols)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fields.py measures on a GPU"
    lib = M.load_library()
    k = 64 if args.small else 1
    out_lines = []

    def say(line):
        out_lines.append(line)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(out_lines) + "\n")

    log = M.DeviceBatch.from_lines(field_buffer((1 << 30) // k, 32, 1))
    csv = M.DeviceBatch.from_lines(field_buffer((1 << 28) // k, 44, 2))
    rows64 = field_buffer((1 << 30) // k, 32, 3)
    c2 = make_c2_batch((1 << 20) // k)
    inputs = [
        ("log: %d lines of 8 to 12 fields, whitespace" % log.n, log, None, True),
        ("log, delim b\" \"", log, b" ", False),
        ("ragged CSR: %d texts of U[64, 1024], whitespace" % ((1 << 20) // k), ragged_with_spaces((1 << 20) // k, 4), None, False),
        ("%d rows of 64 bytes, whitespace" % (rows64.numel() // 64), M.DeviceBatch.strided(rows64, 64, length=64), None, False),
        ("headline batch: %d rows of 1 KiB, whitespace" % c2.shape[0], M.DeviceBatch.strided(c2.reshape(-1), 1024, length=1024), None, True),
        ("csv: %d lines, delim b\",\"" % csv.n, csv, b",", False),
    ]

    # the routes agree before anything is timed
    rx_comma = M.compile_regex(b",")
    for cols in COLUMNS:
        prefix, rows, nf = csv.fields(cols, b",")
        want_rows, want_nf = split_route(rx_comma, csv, cols, None)
        assert torch.equal(rows, want_rows.to(torch.int32)) and torch.equal(nf, want_nf), cols
        del prefix, rows, nf, want_rows, want_nf
    torch.cuda.empty_cache()

    say("Times in ms: median (fastest - slowest) of 7 calls after 2 warm-up calls, the routes of a row taking turns.  "
        "G by the rule unless a column says otherwise.\n")
    say("| input | MiB | columns | counts | fields | copy | fields / copy | GiB/s | split + torch | fields vs split | captures_all | fields vs captures |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|")
    losses = []
    for title, batch, delim, with_captures in inputs:
        mib = batch.data.numel() / 2**20
        dst = torch.empty_like(batch.data)
        rx = M.compile_regex(delim) if delim else None
        cap = None
        if rx is not None:
            cap = int(rx.split_dev(batch)[2])
        for cols in COLUMNS:
            for counts in (True, False):
                out = (torch.empty(batch.n + 1, dtype=torch.int64, device="cuda"),
                       torch.empty((batch.n, len(cols), 2), dtype=torch.int32, device="cuda"),
                       torch.empty(batch.n, dtype=torch.int32, device="cuda") if counts else None)
                fns = [lambda: batch.fields_async(out, cols, delim), lambda: dst.copy_(batch.data)]
                names = ["fields", "copy"]
                if rx is not None and counts:
                    fns.append(lambda: split_route(rx, batch, cols, cap))
                    names.append("split")
                if with_captures and counts and min(cols) > 0:
                    try:
                        crx = M.compile_regex(capture_pattern(cols))
                        crx.captures_all(batch, count=1)
                        fns.append(lambda: crx.captures_all(batch, count=1))
                        names.append("captures")
                    except M.MrxError as e:
                        print("... captures_all refused: %s" % str(e)[:80], flush=True)
                t = dict(zip(names, timed_alternating(fns)))
                f, c = t["fields"], t["copy"]
                cells = []
                for other in ("split", "captures"):
                    if other in t:
                        cells += [fmt(t[other]), "%.2fx" % (f[0] / t[other][0])]
                        if f[0] > t[other][0]:
                            losses.append("%s, columns %s: fields %.3f ms, %s %.3f ms" % (title, cols, f[0], other, t[other][0]))
                    else:
                        cells += ["-", "-"]
                say("| %s | %.0f | %s | %s | %s | %s | %.2fx | %.0f | %s |" % (
                    title, mib, cols, "yes" if counts else "no", fmt(f), fmt(c), f[0] / c[0], mib / 1024 / (f[0] / 1e3),
                    " | ".join(cells)))
                del out
        del dst
        torch.cuda.empty_cache()
    say("")
    say("Rows where fields is the slower route: %s\n" % ("; ".join(losses) if losses else "none"))

    say("### G, the lanes that share a text: fields in ms, median of 7\n")
    groups = (1, 2, 4, 8, 16, 32, 64)
    say("| input | mean length | columns | counts | " + " | ".join("G = %d" % g for g in groups) + " | rule |")
    say("|---|---|---|---|" + "---|" * (len(groups) + 1))
    for title, batch, delim, _ in inputs:
        mean = batch.data.numel() / max(batch.n, 1)
        for cols, counts in (([1, 4, 10], True), ([1], False), ([-1], True)):
            out = (None, torch.empty((batch.n, len(cols), 2), dtype=torch.int32, device="cuda"),
                   torch.empty(batch.n, dtype=torch.int32, device="cuda") if counts else None)
            row = []
            for g in groups + (0,):
                lib.mrx_debug_fields_group(g)
                row.append("%.3f" % timed_alternating([lambda: batch.fields_async(out, cols, delim)])[0][0])
            lib.mrx_debug_fields_group(0)
            say("| %s | %.0f | %s | %s | %s |" % (title, mean, cols, "yes" if counts else "no", " | ".join(row)))
            del out
    if args.out:
        print("wrote", args.out)


if __name__ == "__main__":
    main()
