#!/usr/bin/env python3
"""Translate and strip on one GPU (profiles/translate.md).  Inputs, all generated on the device from a seed:
  the 1 GiB buffer of tools/bench_lines.py (lower-case letters, lines of U[40, 160] bytes) as one text and as the batch
  of its lines; the ragged CSR cut of the headline batch (2^20 rows of 1 KiB cut to U[64, 1024] bytes and packed); the
  headline batch itself, 2^20 rows at a fixed pitch of 1 KiB.
Forms on each: upper(), a random permutation table, delete=b"\\r" (almost nothing goes), delete of the lower-case letters
(most bytes go), squeeze=b" ", and strip().
Per row, in the same run, each as median (fastest - slowest) of 7 device-event timings after 2 warm-up calls, the routes
taking turns call by call:
  call     the DeviceBatch method: the kernels, the allocation of the result and (packed form) the read-back of the totals
  kernels  the _async form on the caller's tensors: what the call enqueues, nothing read back
  copy     a plain device copy of the same bytes
  torch    the route the API left before: lut[data.long()] for a map; data[keep[data.long()]] plus a cumsum of the kept
           flags read at the offsets for delete; none for squeeze and strip (no row)
and once, by the host clock: bytes.translate / bytes.strip plus DeviceBatch.from_texts on an eighth of the lines, times
eight.  Before anything is timed the results are compared with the torch route's.

  python tools/bench_translate.py [--out TABLE.md] [--small]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402
from bench_lines import fmt, line_buffer, ragged_with_separators, timed_alternating  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch  # noqa: E402

IDENTITY = bytes(range(256))
LETTERS = bytes(range(97, 123))


def lut_tensor(table):
    return torch.from_numpy(np.frombuffer(table, np.uint8).copy()).cuda()


def keep_tensor(delete):
    keep = np.ones(256, bool)
    keep[list(delete)] = False
    return torch.from_numpy(keep).cuda()


def torch_delete(batch, keep, offsets):
    mask = keep[batch.data.long()]
    out = batch.data[mask]
    csum = torch.zeros(mask.numel() + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(mask, 0, dtype=torch.int64, out=csum[1:])
    return out, csum[offsets]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_translate.py measures on a GPU"
    lib = M.load_library()
    k = 64 if args.small else 1
    nbytes, n = (1 << 30) // k, (1 << 20) // k
    out_lines = []

    def say(line):
        out_lines.append(line)
        print(line, flush=True)

    first = line_buffer(nbytes, 40, 160, 1)
    lines = M.DeviceBatch.from_lines(first)
    inputs = [
        ("1 buffer of log lines as one text", M.DeviceBatch.strided(first, nbytes, length=nbytes)),
        ("its %d lines (CSR, known bounds)" % lines.n, lines),
        ("ragged CSR, %d texts of U[64, 1024]" % n, ragged_with_separators(n, 4)),
        ("%d rows at a fixed pitch of 1 KiB" % n, M.DeviceBatch.strided(make_c2_batch(n).reshape(-1), 1024, length=1024)),
    ]
    perm = bytes(np.random.default_rng(256).permutation(256).astype(np.uint8).tolist())
    forms = [
        ("upper()", dict(table=IDENTITY.upper())),
        ("a permutation table", dict(table=perm)),
        ("delete \\r", dict(delete=b"\r")),
        ("delete a-z", dict(delete=LETTERS)),
        ("squeeze ' '", dict(squeeze=b" ")),
    ]

    # the torch route agrees before anything is timed (the lines, at a 64th of their count)
    probe = M.DeviceBatch.from_lines(first[:nbytes // 64].clone())
    for title, params in forms:
        res = probe.translate(**params)
        got = res.data[:res._end_offset]
        if "table" in params:
            assert torch.equal(got, lut_tensor(params["table"])[probe.data[:probe._end_offset].long()]), title
        elif "delete" in params:
            data, off = torch_delete(probe, keep_tensor(params["delete"]), probe.offsets)
            assert torch.equal(got, data) and torch.equal(res.offsets, off), title
    del probe, got, res

    say("Piece length %d bytes.  Times in ms: median (fastest - slowest) of 7 calls after 2 warm-up calls, the routes taking "
        "turns.  A row in bold: the call is slower than the torch route.\n" % lib.mrx_debug_translate_piece(-1))
    say("| input | form | MiB in | MiB out | call | kernels | copy | torch route | kernels / copy | GiB/s in (kernels) | call vs torch |")
    say("|---|---|---|---|---|---|---|---|---|---|---|")
    for ititle, batch in inputs:
        mib = batch.data.numel() / 2**20
        offsets = batch.csr_offsets()
        dst = torch.empty_like(batch.data)
        for title, params in forms:
            packed = "table" not in params
            res = batch.translate(**params)
            nb = res._end_offset if packed else batch.data.numel()
            del res
            outs = (torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda"), torch.empty(batch.n + 1, dtype=torch.int64, device="cuda"),
                    torch.empty(2, dtype=torch.int64, device="cuda"))
            fns = [lambda: batch.translate(**params), lambda: batch.translate_async(outs, **params), lambda: dst.copy_(batch.data)]
            if "table" in params:
                lut = lut_tensor(params["table"])
                fns.append(lambda: lut[batch.data.long()])
            elif "delete" in params:
                keep = keep_tensor(params["delete"])
                fns.append(lambda: torch_delete(batch, keep, offsets))
            print("... %s, %s" % (ititle, title), flush=True)   # (a phase that stalls is then known)
            t = timed_alternating(fns)
            call, kern, copy = t[0], t[1], t[2]
            old = fmt(t[3]) if len(t) > 3 else "none"
            versus = "%.2fx" % (call[0] / t[3][0]) if len(t) > 3 else "-"
            b = "**" if len(t) > 3 and call[0] > t[3][0] else ""
            say("| %s%s%s | %s%s%s | %.0f | %.0f | %s | %s | %s | %s | %.2fx | %.0f | %s |" % (
                b, ititle, b, b, title, b, mib, nb / 2**20, fmt(call), fmt(kern), fmt(copy), old, kern[0] / copy[0],
                mib / 1024 / (kern[0] / 1e3), versus))
            del outs
            torch.cuda.empty_cache()
        # strip: rows only, and the stripped batch
        rows = torch.empty((batch.n, 1, 2), dtype=torch.int32, device="cuda")
        prefix = torch.empty(batch.n + 1, dtype=torch.int64, device="cuda")
        print("... %s, strip" % ititle, flush=True)
        t = timed_alternating([lambda: batch.strip(), lambda: batch.strip_async((prefix, rows)), lambda: dst.copy_(batch.data)])
        say("| %s | strip(): call is rows and gather_spans, kernels the rows alone | %.0f | - | %s | %s | %s | none | %.2fx | %.0f | - |" % (
            ititle, mib, fmt(t[0]), fmt(t[1]), fmt(t[2]), t[1][0] / t[2][0], mib / 1024 / (t[1][0] / 1e3)))
        del dst, rows, prefix
        torch.cuda.empty_cache()

    say("\n### The host route: bytes methods and from_texts on an eighth of the lines (host clock)\n")
    raw, off = lines.data.cpu().numpy().tobytes(), lines.offsets.cpu().numpy()
    texts = [raw[off[i]:off[i + 1]] for i in range(lines.n // 8)]
    del raw
    for title, fn in (("t.upper()", lambda t: t.upper()), ("t.translate(None, a-z)", lambda t: t.translate(None, LETTERS)), ("t.strip()", lambda t: t.strip())):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = [fn(t) for t in texts]
        t1 = time.perf_counter()
        hb = M.DeviceBatch.from_texts(outs)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        say("- %s on %d lines: Python %.0f ms, from_texts %.0f ms; times eight for all lines: %.0f ms." % (
            title, len(texts), (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 8e3))
        del outs, hb

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(out_lines) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
