#!/usr/bin/env python3
"""Lines on one GPU (profiles/lines.md).  Inputs, all generated on the device from a seed:
  one buffer of 1 GiB with lines of U[40, 160] bytes (mean 100), of U[512, 1536] (mean 1 KiB) and of U[2, 14] (mean 8),
  every line ended by b"\\n"; the first buffer again as 64 texts of 16 MiB at a fixed pitch, and its first 48 MiB as one
  buffer (the old route is timed only on texts below 2^26 bytes: above that findall walks a text with a single lane); the ragged CSR cut of the
  headline batch (2^20 rows of 1 KiB cut to U[64, 1024] bytes and packed) with a separator at one byte in a hundred; the
  first buffer with b"\\r\\n" line ends under crlf, and as it is under keepends (from_lines: offsets only, no byte moves).
Per input, in the same run, each as median (fastest - slowest) of device-event timings after warm-up, lines and the old
route alternating call by call:
  call     DeviceBatch.lines with capacities that fit: the kernels and the one read-back of the totals
  kernels  DeviceBatch.lines_async on the caller's tensors: what the call enqueues, nothing read back
  split    compile_regex(b"\\n").split_batch on the same input: the route the API offered before (findall, sizes, scan,
           gather; it keeps a trailing empty piece)
  copy     a plain device copy of the input
and once, by the host clock: bytes.split plus DeviceBatch.from_texts on an eighth of the buffer, times eight.
Then the piece length P swept on the first input (kernels).  Before anything is timed the lines are compared with the old
route's pieces.

  python tools/bench_lines.py [--out TABLE.md] [--small] [--skip-split]
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


SPLIT_MAX_TEXT = 1 << 26


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
    return "%.2f (%.2f - %.2f)" % t


def line_buffer(nbytes, lo, hi, seed, crlf=False):
    """nbytes of lower-case letters cut into lines of U[lo, hi] bytes, separator included; the last line is cut by the
    buffer's end and ends in a separator too."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    data = torch.randint(97, 123, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
    count = 2 * nbytes // (lo + hi) + 1024
    ends = torch.cumsum(torch.randint(lo, hi + 1, (count,), device="cuda", generator=g), 0) - 1
    ends = ends[ends < nbytes - 1]
    data[ends] = 10
    data[-1] = 10
    if crlf:
        data[ends[ends > 0] - 1] = 13
    return data


def ragged_with_separators(n, seed):
    """The headline batch's rows cut to U[64, 1024] bytes and packed, one byte in a hundred a separator."""
    L = 1024
    data = make_c2_batch(n).reshape(-1).clone()
    g = torch.Generator(device="cuda").manual_seed(seed)
    data[torch.rand(data.numel(), device="cuda", generator=g) < 0.01] = 10
    lens = torch.randint(64, L + 1, (n,), device="cuda", generator=g)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), lens, output_size=total)
    src = row * L + (torch.arange(total, device="cuda") - off[:-1][row])
    return M.DeviceBatch.csr_known(data[src], off, total, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--skip-split", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lines.py measures on a GPU"
    lib = M.load_library()
    k = 64 if args.small else 1
    nbytes = (1 << 30) // k
    rx = M.compile_regex(b"\n")   # (the newline byte itself: the dialect has no \n escape)
    out_lines = []

    def say(line):
        out_lines.append(line)
        print(line, flush=True)

    def one(data):
        return M.DeviceBatch.strided(data, data.numel(), length=data.numel())

    first = line_buffer(nbytes, 40, 160, 1)
    inputs = [
        ("1 buffer, lines of U[40, 160] bytes", one(first), dict()),
        ("1 buffer of %d MiB, lines of U[40, 160] bytes" % (3 * nbytes // 64 >> 20), one(first[:3 * nbytes // 64]), dict()),
        ("1 buffer, lines of U[512, 1536] bytes", one(line_buffer(nbytes, 512, 1536, 2)), dict()),
        ("1 buffer, lines of U[2, 14] bytes", one(line_buffer(nbytes, 2, 14, 3)), dict()),
        ("64 texts of %d KiB, lines of U[40, 160]" % (nbytes // 64 >> 10), M.DeviceBatch.strided(first, nbytes // 64, length=nbytes // 64), dict()),
        ("ragged CSR, %d texts of U[64, 1024], a separator per 100 bytes" % ((1 << 20) // k),
         ragged_with_separators((1 << 20) // k, 4), dict()),
        ("1 buffer, lines of U[40, 160], \\r\\n ends, crlf", one(line_buffer(nbytes, 40, 160, 1, crlf=True)), dict(crlf=True)),
        ("1 buffer, lines of U[40, 160], keepends (from_lines: offsets only)", one(first), dict(keepends=True)),
    ]

    # the results agree before anything is timed (first input, at a 64th of its size)
    head = first[:nbytes // 64].clone()
    head[-1] = 10
    probe = one(head)
    res, prefix, _ = probe.lines()
    if not args.skip_split:
        pieces, pprefix, _ = rx.split_batch(probe)
        assert int(pprefix[-1]) == res.n + 1 and torch.equal(pieces.offsets[:res.n + 1], res.offsets)   # + the empty last piece
        assert torch.equal(pieces.data[:res._end_offset], res.data[:res._end_offset])
        del pieces, pprefix
    del res, prefix, probe

    say("Piece length %d bytes.  Times in ms: median (fastest - slowest) of 7 calls after 2 warm-up calls, lines and split "
        "alternating.\n" % lib.mrx_debug_lines_piece(-1))
    say("| input | MiB | lines | call | kernels | split_batch | copy | kernels / copy | GiB/s (kernels) | call vs split |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    verdicts = []
    for title, batch, opts in inputs:
        mib = batch.data.numel() / 2**20
        offsets_only = "from_lines" in title
        res = M.DeviceBatch.from_lines(batch.data, **opts) if offsets_only else batch.lines(**opts)[0]
        nlines, nb = res.n, res._end_offset
        del res
        outs = (torch.empty(batch.n + 1, dtype=torch.int64, device="cuda"), torch.empty(max(nlines, 1), dtype=torch.int64, device="cuda"),
                torch.empty(nlines + 1, dtype=torch.int64, device="cuda"),
                torch.empty(1 if offsets_only else max(nb, 1), dtype=torch.uint8, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda"))
        dst = torch.empty_like(batch.data)
        fns = [(lambda: M.DeviceBatch.from_lines(batch.data, piece_cap=nlines, **opts)) if offsets_only else
               (lambda: batch.lines(piece_cap=nlines, out_cap=nb, **opts)),
               lambda: batch.lines_async(outs, **opts), lambda: dst.copy_(batch.data)]
        split = None
        print("... %s: %d lines, %d bytes" % (title, nlines, nb), flush=True)   # (a phase that stalls is then known)
        # findall serves a text of 2^26 bytes and more with one lane for the whole text (its event records count a
        # text's matches in 26 bits, mrx_kernels.hip, kStreamMaxText): minutes for a GiB, so the old route is timed only
        # below that
        longest = batch.stride if batch.offsets is None else batch._max_len
        if not args.skip_split and not opts and longest >= SPLIT_MAX_TEXT:
            split = "not run (a text of 2^26 bytes or more)"
        elif not args.skip_split and not opts:
            print("... split_batch", flush=True)
            try:
                rx.split_batch(batch)
                fns.append(lambda: rx.split_batch(batch))
            except M.MrxError as e:
                split = "refused: %s" % str(e)[:60]
        t = timed_alternating(fns)
        call, kern, copy = t[0], t[1], t[2]
        if len(t) > 3:
            spread = max(call[2] - call[1], t[3][2] - t[3][1])
            verdict = "level or faster" if call[0] <= t[3][0] + spread else "SLOWER"
            verdicts.append((title, call[0], t[3][0], spread, verdict))
            split = fmt(t[3])
            versus = "%.2fx, %s" % (call[0] / t[3][0], verdict)
        else:
            versus = "-"
        say("| %s | %.0f | %d | %s | %s | %s | %s | %.1fx | %.1f | %s |" % (
            title, mib, nlines, fmt(call), fmt(kern),
            split or ("not run (split has no such option)" if opts else "not run (--skip-split)"), fmt(copy), kern[0] / copy[0],
            mib / 1024 / (kern[0] / 1e3), versus))
        del outs, dst
        torch.cuda.empty_cache()
    say("")
    for title, c, s, spread, verdict in verdicts:
        say("- %s: call %.2f ms, split_batch %.2f ms, spread of the repeats %.2f ms: %s." % (title, c, s, spread, verdict))

    say("\n### The host route: bytes.split and from_texts on an eighth of the first buffer (host clock)\n")
    host = first[:nbytes // 8].cpu().numpy().tobytes()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parts = host.split(b"\n")
    t1 = time.perf_counter()
    hb = M.DeviceBatch.from_texts(parts)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    say("%d MiB, %d pieces: bytes.split %.0f ms, from_texts %.0f ms; times eight for the whole buffer: %.0f ms.\n" % (
        len(host) >> 20, len(parts), (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 8e3))
    del parts, hb, host

    say("### The piece length: kernels on the first input, ms\n")
    sizes = (1024, 2048, 4096, 8192, 16384, 65536)
    say("| " + " | ".join("P = %d" % p for p in sizes) + " |")
    say("|" + "---|" * len(sizes))
    batch = inputs[0][1]
    res, _, _ = batch.lines()
    nlines, nb = res.n, res._end_offset
    del res
    outs = (torch.empty(2, dtype=torch.int64, device="cuda"), torch.empty(nlines, dtype=torch.int64, device="cuda"),
            torch.empty(nlines + 1, dtype=torch.int64, device="cuda"), torch.empty(nb, dtype=torch.uint8, device="cuda"),
            torch.empty(4, dtype=torch.int64, device="cuda"))
    row = []
    for p in sizes:
        lib.mrx_debug_lines_piece(p)
        row.append(fmt(timed_alternating([lambda: batch.lines_async(outs)])[0]))
    lib.mrx_debug_lines_piece(0)
    say("| " + " | ".join(row) + " |")

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(out_lines) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
