#!/usr/bin/env python3
"""numbers on one GPU (profiles/parse.md).  Cases:
  digits    2^24 pieces of 1 to 10 digits as a packed batch, DeviceBatch.parse("int");
  headline  the \\d+ pieces of the headline batch (2^20 x 1 KiB), CompiledRegex.numbers;
  log       (\\d+) (\\d+\\.\\d+) over 2^20 log-like lines: group 1 as int, group 2 as float;
  floats    2^22 pieces "123.456" to "1234567.123456e-3" as a packed batch, DeviceBatch.parse("float").
Per case and kind:
  (k) the kernel alone: the C entry point on buffers allocated before, one launch between two device events (for the
      cases with a pattern the spans are found once, before);
  (n) the whole call: numbers() -- findall or captures_all, then the parse, the allocations included -- or parse();
  (e) what the parent commit offers: extract (a packed batch: nothing to extract), then a copy to the host and int() or
      float() on the first eighth of the pieces, host clock, reported per million pieces next to the extract itself;
  (t) for pieces that are digits only (digits, headline): gather_spans (a packed batch: nothing to gather) plus a torch
      computation on rows padded to 32 bytes: (byte - '0') times a power of ten by column, masked by length, summed per
      row; pieces of more than 18 digits do not fit it and are left to it as they come (its values are compared with
      the kernel's on the rows of at most 18 digits);
  (d) a plain device copy of the same bytes: the batch's for a packed batch, else the bytes under the spans.
(k), (n), (t) and (d) are medians of 10 device-event timings after warm-up.  Every result is checked before it is timed,
on a sample against Python's int() / float(), and the share of rows that end as RANGE, MALFORMED and EMPTY is reported.

  python tools/bench_parse.py [--out TABLE.md] [--small] [--case NAME]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mojo_regex_amd as M  # noqa: E402
from bench_distinct import csr_of_picks, padded_rows, timed  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch  # noqa: E402

KIND_CODE = {"int": 0, "hex": 1, "float": 2}


def packed_from_lens(digits, lens):
    """A CSR batch whose text i is the first lens[i] bytes of row i of `digits` (uint8[n, w]), built on the device."""
    n, w = digits.shape
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens, 0)
    keep = torch.arange(w, device="cuda")[None, :] < lens[:, None]
    return M.DeviceBatch.csr_known(digits[keep].contiguous(), off, int(off[-1]), int(lens.max()))


def case_digits(k):
    n = (1 << 24) // k
    g = torch.Generator(device="cuda").manual_seed(11)
    digits = (torch.randint(0, 10, (n, 10), generator=g, device="cuda") + 48).to(torch.uint8)
    lens = torch.randint(1, 11, (n,), generator=g, device="cuda")
    return "%d pieces of 1 to 10 digits, packed" % n, packed_from_lens(digits, lens), None, [("int", None)]


def case_headline(k):
    n = (1 << 20) // k
    batch = M.DeviceBatch.strided(make_c2_batch(n).reshape(-1), 1024, length=1024)
    return "\\d+ on %d x 1 KiB" % n, batch, M.compile_regex(b"\\d+"), [("int", None)]


def case_log(k):
    n = (1 << 20) // k
    rng = np.random.default_rng(20261019)
    hosts = [b"10.0.%d.%d" % (a, b) for a in range(4) for b in range(64)]
    vocab = [b"%s GET /api/v%d/items/%d %d %d.%03d" % (hosts[int(rng.integers(0, len(hosts)))], rng.integers(1, 4),
                                                      rng.integers(0, 10 ** 6), rng.integers(0, 10 ** int(rng.integers(1, 8))),
                                                      rng.integers(0, 30), rng.integers(0, 1000)) for _ in range(1 << 14)]
    picks = torch.from_numpy(rng.integers(0, len(vocab), size=n)).cuda()
    return ("(\\d+) (\\d+\\.\\d+) on %d log lines" % n, csr_of_picks(vocab, picks), M.compile_regex(b"(\\d+) (\\d+\\.\\d+)"),
            [("int", 1), ("float", 2)])


def case_floats(k):
    n = (1 << 22) // k
    rng = np.random.default_rng(7)
    vocab = []
    for _ in range(1 << 16):
        w = int(rng.integers(1, 7))
        vocab.append(b"%d.%0*d" % (rng.integers(0, 10 ** int(rng.integers(1, 8))), w, rng.integers(0, 10 ** w)) +
                     (b"e-%d" % rng.integers(0, 9) if rng.random() < 0.25 else b""))
    picks = torch.from_numpy(rng.integers(0, len(vocab), size=n)).cuda()
    return "%d float pieces, packed" % n, csr_of_picks(vocab, picks), None, [("float", None)]


CASES = {"digits": case_digits, "headline": case_headline, "log": case_log, "floats": case_floats}


def find_rows(batch, rx, group):
    """(prefix, rows tensor, pair) of the case's pattern; None for a packed batch."""
    if rx is None:
        return None
    if group is None:
        prefix, spans, total = rx._dev_findall(batch)
        return prefix, spans[:total], 0
    prefix, rows = rx._captures_all_dev(batch)
    return prefix, rows, (group - 1) % (rx.num_groups + 1)


def kernel_call(batch, rows, kind):
    """A closure that makes the one C call on buffers allocated here, and its outputs."""
    lib = M.load_library()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    m = batch.n if rows is None else int(rows[1].shape[0])
    values = torch.empty(m, dtype=torch.int64, device="cuda")
    status = torch.empty(m, dtype=torch.uint8, device="cuda")
    if rows is None:
        def call():
            assert batch.call(lib, "mrx_parse", (), (KIND_CODE[kind], 0, values.data_ptr(), status.data_ptr(), stream)) == 0
        return call, values, status, None
    prefix, sp, pair = rows
    owner = torch.empty(m, dtype=torch.int64, device="cuda")
    d_totals = torch.empty(1, dtype=torch.int64, device="cuda")
    row_pairs = int(sp.shape[1]) if sp.dim() == 3 else 1

    def call():
        assert batch.call(lib, "mrx_parse_spans", (), (prefix.data_ptr(), sp.data_ptr(), row_pairs, pair, KIND_CODE[kind], 0, m,
                                                      values.data_ptr(), status.data_ptr(), owner.data_ptr(),
                                                      d_totals.data_ptr(), None, stream)) == 0
    return call, values, status, owner


def pieces_of(batch, rx, group):
    """The pieces as a packed batch, by the parent commit's route (the batch itself when it is packed already)."""
    return batch if rx is None else rx.extract(batch, group)[0]


def host_numbers(pieces, m, kind):
    """Seconds for the first m pieces: copy to the host, bytes objects, int() / float() with the refusals caught."""
    conv = float if kind == "float" else int
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    off = pieces.offsets[:m + 1].cpu().numpy()
    raw = pieces.data[:int(off[-1])].cpu().numpy().tobytes()
    out = []
    for i in range(m):
        try:
            out.append(conv(raw[off[i]:off[i + 1]]))
        except ValueError:
            out.append(None)
    return time.perf_counter() - t0, out


POW10 = None


def torch_digits(pieces):
    """int of digit-only pieces by torch on rows padded to 32 bytes (the 33rd byte of padded_rows is the length)."""
    global POW10
    if POW10 is None:
        POW10 = torch.tensor([10 ** min(j, 18) for j in range(33)], dtype=torch.int64, device="cuda")
    rows = padded_rows(pieces)
    lens = rows[:, 32].to(torch.int64)
    col = torch.arange(32, device="cuda")[None, :]
    place = POW10[(lens[:, None] - 1 - col).clamp_(min=0)]
    return ((rows[:, :32].to(torch.int64) - 48) * place * (col < lens[:, None])).sum(1)


def check(values, status, pieces, kind, sample=4096):
    """The kernel's rows against Python on a sample of the pieces."""
    m = pieces.n
    idx = torch.arange(0, m, max(1, m // sample), device="cuda")
    taken = pieces.take(idx)
    off = taken.offsets.cpu().numpy()
    raw = taken.data.cpu().numpy().tobytes()
    vals = (values.view(torch.float64) if kind == "float" else values)[idx].cpu().numpy().tolist()
    st = status[idx].cpu().numpy().tolist()
    for j in range(len(st)):
        t = raw[off[j]:off[j + 1]]
        if st[j] == 0:
            assert vals[j] == (float(t) if kind == "float" else int(t)), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="1/64 of every shape (a rehearsal, not a measurement)")
    ap.add_argument("--case", choices=list(CASES), action="append")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_parse.py measures on a GPU"
    k = 64 if args.small else 1
    lines = ["| case | kind | rows | MiB of pieces | RANGE / MALFORMED / EMPTY share | (k) kernel ms | M rows/s | (n) whole call ms | "
             "(e) extract ms + host, s per million pieces (pieces timed) | (e)/(n) at these rows | (t) gather + torch on 32-byte rows ms "
             "| (t)/(n) | (d) copy ms | (k)/(d) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in args.case or list(CASES):
        title, batch, rx, kinds = CASES[name](k)
        for kind, group in kinds:
            rows = find_rows(batch, rx, group)
            call, values, status, _ = kernel_call(batch, rows, kind)
            call()
            torch.cuda.synchronize()
            pieces = pieces_of(batch, rx, group)
            m = pieces.n
            assert m == values.numel()
            check(values, status, pieces, kind)
            shares = [float((status == s).sum()) / max(m, 1) for s in (3, 2, 1)]
            kern = timed(call)[0]
            if rx is None:
                whole = timed(lambda: batch.parse(kind))[0]
                ext = 0.0
            else:
                whole = timed(lambda: rx.numbers(batch, kind, group))[0]
                ext = timed(lambda: rx.extract(batch, group), warmup=1, reps=3)[0]
            mh = max(1, min(m, (1 << 21) // k))
            secs, host = host_numbers(pieces, mh, kind)
            e_total_ms = ext + secs / mh * m * 1e3
            longest = int((pieces.offsets[1:] - pieces.offsets[:-1]).max()) if m else 0
            if kind == "int" and name in ("digits", "headline") and longest <= 32:
                tv = torch_digits(pieces)
                short = (status == 0) & ((pieces.offsets[1:] - pieces.offsets[:-1]) <= 18)
                assert bool((tv[short] == values[short]).all()), "the torch route gives other values"
                t_ms = timed(lambda: torch_digits(pieces_of(batch, rx, group)), warmup=1, reps=3)[0]
                t_txt, t_ratio = "%.2f" % t_ms, "%.1fx" % (t_ms / whole)
            else:
                t_txt = "not applicable: %s" % ("pieces of up to %d bytes" % longest if kind == "int" and name != "log" else "not digits only")
                t_ratio = ""
            dst = torch.empty_like(pieces.data)
            d = timed(lambda: dst.copy_(pieces.data))[0]
            del dst
            lines.append("| %s | %s%s | %d | %.1f | %.4f / %.4f / %.4f | %.3f | %.0f | %.3f | %.2f + %.2f (%d) | %.0fx | %s | %s | %.3f | %.1fx |" % (
                title, kind, "" if group is None else ", group %d" % group, m, int(pieces.data.numel()) / 2**20, shares[0],
                shares[1], shares[2], kern, m / kern / 1e3, whole, ext, secs / mh * 1e6, mh, e_total_ms / whole, t_txt, t_ratio,
                d, kern / d))
            print(lines[-1], flush=True)
            del pieces, values, status, rows, call
        del batch
        torch.cuda.empty_cache()
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
