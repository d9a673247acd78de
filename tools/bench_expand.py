#!/usr/bin/env python3
"""expand on one GPU (profiles/expand.md): per case
  (a) captures_all alone: the floor, it is part of the call;
  (b) expand;
  (c) what the public API offered before: captures_all once, then one gather_spans per distinct referenced group.
      That yields the group bytes but not the interleaved records, so it is a lower bound of that route;
  (d) a plain device copy of as many bytes as the records hold.
Cases: the three batches of profiles/captures_all.md (tools/bench_captures_all.py: 2^20 x 1 KiB at a fixed pitch) --
'(\\d{3})(\\d{3})(\\d{4})' -> '(\\1) \\2-\\3' on phone-like texts (fixed route), '(\\w+) (\\w+)' -> '\\2 \\1' on words
(chain route), '(a|ab)(c|bcd)(d*)' -> '\\3\\2\\1' (general route) -- and the first cut to a ragged CSR batch of
64..1024-byte texts.  Times are medians of device-event timings after warm-up, (b) with its fastest and slowest call.
Before anything is timed, expand's owners and offsets are compared with (c)'s over every record, and its bytes with the
records assembled from (c)'s pieces and the literals by torch ops, over the first and the last 2^18 records.

  python tools/bench_expand.py [--out TABLE.md] [--small] [--only-expand CASE]

The table is printed; --out also writes it to a file (profiles/expand.md is a write-up around a copy of it: do not
point --out at it).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402
from bench_captures_all import batch as make_batch  # noqa: E402
from bench_extract import ragged_of, timed  # noqa: E402

CASES = [("phone", b"(\\d{3})(\\d{3})(\\d{4})", b"(\\1) \\2-\\3"), ("words", b"(\\w+) (\\w+)", b"\\2 \\1"),
         ("alt", b"(a|ab)(c|bcd)(d*)", b"\\3\\2\\1")]


def parse(tpl):
    """[(group, literal)]: sub's template grammar, only \\1..\\9 are references."""
    segs, i, lit = [], 0, b""
    while i < len(tpl):
        if tpl[i] == 0x5C and i + 1 < len(tpl) and 0x31 <= tpl[i + 1] <= 0x39:
            if lit:
                segs.append((0, lit))
            segs.append((tpl[i + 1] - 0x30, b""))
            i, lit = i + 2, b""
        else:
            lit += tpl[i:i + 1]
            i += 1
    if lit:
        segs.append((0, lit))
    return segs


def assemble(segs, pieces, lo, hi, dev):
    """(offsets, bytes) of the records [lo, hi) from the group pieces of (c) and the literals, by torch ops."""
    m = hi - lo
    seg_len = []
    for g, lit in segs:
        if g:
            o = pieces[g].offsets
            seg_len.append(o[lo + 1:hi + 1] - o[lo:hi])
        else:
            seg_len.append(torch.full((m,), len(lit), dtype=torch.int64, device=dev))
    off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(sum(seg_len), 0)
    out = torch.empty(int(off[-1]), dtype=torch.uint8, device=dev)
    at = off[:-1].clone()
    for (g, lit), ln in zip(segs, seg_len):
        tot = int(ln.sum())
        if tot:
            first = torch.cumsum(ln, 0) - ln
            idx = torch.repeat_interleave(at - first, ln, output_size=tot) + torch.arange(tot, device=dev)
            if g:
                o = pieces[g].offsets
                out[idx] = pieces[g].data[int(o[lo]):int(o[hi])]
            else:
                out[idx] = torch.tensor(list(lit), dtype=torch.uint8, device=dev).repeat(m)
        at += ln
    return off, out


def cell(name, b, rx, tpl, lines):
    segs = parse(tpl)
    groups = sorted({g for g, _ in segs if g})
    dev = b.data.device
    prefix, rows = rx.captures_all(b)   # warm-up; sizes the buffer of (a) and (c)
    kernel = M.load_library().mrx_last_kernel_name().decode()
    m = int(rows.shape[0])
    cap = m + 64

    def route_c():
        p, r = rx._captures_all_dev(b, 0, match_cap=cap)
        return p, {g: b.gather_spans(p, r, pair=g - 1) for g in groups}

    records, eprefix, eowner = rx.expand(tpl, b)
    p, got = route_c()
    assert torch.equal(eprefix, p) and records.n == m, name
    for g in groups:
        assert torch.equal(eowner, got[g][1]), name
    pieces = {g: got[g][0] for g in groups}
    want_len = sum((pieces[g].offsets[1:] - pieces[g].offsets[:-1]) if g else len(lit) for g, lit in segs)
    assert torch.equal(records.offsets[1:] - records.offsets[:-1], want_len), name
    for lo, hi in {(0, min(m, 1 << 18)), (max(0, m - (1 << 18)), m)}:
        off, want = assemble(segs, pieces, lo, hi, dev)
        a0, a1 = int(records.offsets[lo]), int(records.offsets[hi])
        assert torch.equal(records.data[a0:a1], want), (name, lo, hi)
    nbytes = int(records.data.numel())
    del records, eprefix, eowner, p, got, pieces, want_len, off, want, prefix, rows
    torch.cuda.empty_cache()
    a, _, _ = timed(lambda: rx._captures_all_dev(b, 0, match_cap=cap), warmup=2, reps=3)
    wu, reps = (1, 5) if a > 100 else (3, 10)   # the general route runs for half a second a call
    a, _, _ = timed(lambda: rx._captures_all_dev(b, 0, match_cap=cap), wu, reps)
    bt, b_lo, b_hi = timed(lambda: rx.expand(tpl, b), wu, reps)
    c, c_lo, c_hi = timed(route_c, wu, reps)
    dst = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    src = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    d, _, _ = timed(lambda: dst.copy_(src))
    lines.append("| %s | %s | %d | %.1f | %.1f | %.3f | %.3f | %.3f - %.3f | %.3f | %.3f - %.3f | %.3f | %.3f | %.3f |" % (
        name, kernel, m, nbytes / 2**20, nbytes / max(m, 1), a, bt, b_lo, b_hi, c, c_lo, c_hi, bt - a, c - a, d))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--only-expand", default=None, metavar="CASE",
                    help="run expand of one case (phone, words, alt) a few times and stop (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_expand.py measures on a GPU"
    n, L = (1 << 20) // (64 if args.small else 1), 1024
    rng = np.random.default_rng(20261015)
    lines = ["| case | captures_all route | records | MiB out | bytes a record | (a) captures_all ms | (b) expand ms "
             "| (b) fastest - slowest | (c) captures_all + gathers ms | (c) fastest - slowest | (b)-(a) ms | (c)-(a) ms "
             "| (d) copy ms |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for kind, pat, tpl in CASES:
        data = make_batch(kind, n, L, rng)
        b = M.DeviceBatch.strided(data, L, length=L)
        rx = M.compile_regex(pat)
        if args.only_expand:
            if kind == args.only_expand:
                for _ in range(5):
                    records, _, _ = rx.expand(tpl, b)
                torch.cuda.synchronize()
                print("records %d bytes %d" % (records.n, records.data.numel()))
            continue
        label = "%s -> %s" % (pat.decode(), tpl.decode())
        cell("%d x 1 KiB, fixed pitch, %s" % (n, label), b, rx, tpl, lines)
        if kind == "phone":
            rag = ragged_of(data, n, L, 64, 1024, 2)
            cell("%d ragged CSR, U[64, 1024], %s" % (n, label), rag, rx, tpl, lines)
            del rag
        del b, data
        torch.cuda.empty_cache()
    if args.out and not args.only_expand:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
