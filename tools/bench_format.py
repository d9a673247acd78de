#!/usr/bin/env python3
"""format on one GPU (profiles/format.md).  Cases:
  words     2^24 rows of "\\1 \\2\\n": an 8-byte word and a count of 1 to 7 digits;
  ints      2^24 int64 of 1 to 19 digits, some negative, as "\\1\\n";
  fixed     2^22 float64 as ".3f" cells, "\\1\\n";
  headline  the distinct values and counts of the headline batch's extract pieces (2^20 x 1 KiB, [a-z]+\\d+), "\\2 \\1\\n";
  top10     the report of value_counts(sort="count", top=10) on those pieces: ten rows.
Per case:
  (c) the C call alone: mrx_format_dev on buffers allocated before, its three launches between two device events;
  (s) the same call with out_cap = 0: k_format_sizes and the scan, no gather (the kernels alone are read from a kernel
      trace, a run of its own: tools/kernel_times_cmd.sh);
  (w) the whole call: format_records(), the allocations and the one read-back of the totals included;
  (h) what the API offers without format: every column copied to the host and b"..." % row in Python, on the first
      eighth of the rows, host clock, reported per million rows;
  (d) a plain device copy of the output's bytes.
(c), (s), (w) and (d) are medians of 10 device-event timings after warm-up.  Every output is checked before it is timed,
on a sample of rows against Python's %.

  python tools/bench_format.py [--out TABLE.md] [--small] [--case NAME]
"""
import argparse
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402
from bench_distinct import case_headline as headline_pieces, timed  # noqa: E402


def case_words(k):
    n = (1 << 24) // k
    g = torch.Generator(device="cuda").manual_seed(3)
    data = (torch.randint(0, 26, (n * 8,), generator=g, device="cuda") + 97).to(torch.uint8)
    words = M.DeviceBatch.strided(data, 8, length=8)
    digits = torch.randint(1, 8, (n,), generator=g, device="cuda")
    counts = (torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 9 + 1) * 10.0 ** (digits - 1).to(torch.float64)
    return "%d rows, an 8-byte word and a count of 1 to 7 digits" % n, rb"\1 \2" + b"\n", [words, counts.to(torch.int64)], b"%s %d\n"


def case_ints(k):
    n = (1 << 24) // k
    g = torch.Generator(device="cuda").manual_seed(4)
    v = torch.randint(-(1 << 62), 1 << 62, (n,), generator=g, device="cuda") >> torch.randint(0, 62, (n,), generator=g, device="cuda")
    return "%d int64 of 1 to 19 digits" % n, rb"\1" + b"\n", [v], b"%d\n"


def case_fixed(k):
    n = (1 << 22) // k
    g = torch.Generator(device="cuda").manual_seed(5)
    v = torch.randn(n, generator=g, device="cuda", dtype=torch.float64) * 10.0 ** torch.randint(-2, 7, (n,), generator=g, device="cuda").to(torch.float64)
    return "%d float64 as .3f" % n, rb"\1" + b"\n", [(v, ".3f")], b"%.3f\n"


def _headline_counts(k):
    _, pieces, _ = headline_pieces(k)
    values, counts, _, _ = pieces.distinct()
    return values, counts


def case_headline(k):
    values, counts = _headline_counts(k)
    return "the %d distinct values of the headline batch's pieces and their counts" % values.n, rb"\2 \1" + b"\n", [values, counts], b"%d %s\n"


def case_top10(k):
    values, counts = _headline_counts(k)
    values, counts = M.api._sort_counts(values, counts, "count", 10)
    return "top 10 of those by count", rb"\2 \1" + b"\n", [values, counts], b"%d %s\n"


CASES = {"words": case_words, "ints": case_ints, "fixed": case_fixed, "headline": case_headline, "top10": case_top10}


def host_rows(columns, tpl_refs, fmt, m):
    """Seconds for the first m rows by the host route: copy every column, build bytes objects, % per row."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cols = []
    for c in columns:
        c = c[0] if isinstance(c, tuple) else c
        if isinstance(c, M.DeviceBatch):
            if c.offsets is None:
                raw = c.data[:m * c.stride].cpu().numpy().tobytes()
                cols.append([raw[i * c.stride:i * c.stride + c.length] for i in range(m)])
            else:
                off = c.offsets[:m + 1].cpu().numpy()
                raw = c.data[:int(off[-1])].cpu().numpy().tobytes()
                cols.append([raw[off[i]:off[i + 1]] for i in range(m)])
        else:
            cols.append(c[:m].cpu().numpy().tolist())
    rows = [fmt % tuple(cols[j - 1][i] for j in tpl_refs) for i in range(m)]
    return time.perf_counter() - t0, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--case", choices=list(CASES), action="append")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_format.py measures on a GPU"
    k = 64 if args.small else 1
    lib = M.load_library()
    lines = ["| case | rows | MiB of records | (c) C call ms | GB/s of output | M rows/s | (s) sizes + scan ms | (w) format_records ms | "
             "(h) host route, s per million rows (rows timed) | (h)/(w) at these rows | (d) copy ms | (c)/(d) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in args.case or list(CASES):
        title, tpl, columns, fmt = CASES[name](k)
        refs = M.api._template_ref_list(tpl)
        records = M.format_records(tpl, columns)
        torch.cuda.synchronize()
        n, nbytes = records.n, int(records.data.numel())
        # a sample of rows against Python
        mh = max(1, min(n, (1 << 21) // k))
        secs, host = host_rows(columns, refs, fmt, mh)
        off = records.offsets[:mh + 1].cpu().numpy()
        raw = records.data[:int(off[-1])].cpu().numpy().tobytes()
        assert raw == b"".join(host), "format_records differs from Python's %"
        arr, _, _, _, _, keep = M.api._fmt_device_columns(tpl, columns)
        out_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        out = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        d_totals = torch.empty(2, dtype=torch.int64, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call(cap=nbytes):
            assert lib.mrx_format_dev(tpl, len(tpl), C.cast(arr, C.c_void_p), len(arr), n, out_off.data_ptr(),
                                      out.data_ptr() if cap else None, cap, None, d_totals.data_ptr(), None, stream) == 0
        call()
        torch.cuda.synchronize()
        assert torch.equal(out[:nbytes], records.data) and d_totals.tolist() == [n, nbytes]
        c_ms = timed(call)[0]
        s_ms = timed(lambda: call(0))[0]
        w_ms = timed(lambda: M.format_records(tpl, columns))[0]
        dst = torch.empty_like(records.data)
        d_ms = timed(lambda: dst.copy_(records.data))[0]
        del dst
        lines.append("| %s | %d | %.1f | %.3f | %.1f | %.0f | %.3f | %.3f | %.2f (%d) | %.0fx | %.3f | %.1fx |" % (
            title, n, nbytes / 2**20, c_ms, nbytes / c_ms / 1e6, n / c_ms / 1e3, s_ms, w_ms, secs / mh * 1e6, mh,
            secs / mh * n * 1e3 / w_ms, d_ms, c_ms / d_ms))
        print(lines[-1], flush=True)
        del records, out, out_off, columns, keep, arr
        torch.cuda.empty_cache()
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
