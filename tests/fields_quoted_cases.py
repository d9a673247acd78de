"""The batches of the quoted-fields tests, shared by the host walk (tests/test_fields_quoted_host.py) and the kernel
(tests/test_gpu_fields_quoted.py): the smallest texts at which the quote parity of a group of G lanes can go wrong.  A
lane takes an aligned 16-byte word and a group G of them a round, so the parity crosses an edge at bytes 15 | 16 (from
lane to lane, through the ballot) and at bytes 16 G - 1 | 16 G (from round to round, through the carried bit)."""
from __future__ import annotations

import csv
import io

import numpy as np

Q = b'"'
GROUPS = (1, 2, 4, 16, 64)
SKEWS = (0, 1, 7, 15)
MODES = (b",", None)   # a delimiter byte, whitespace
# (columns, rest)
REQUESTS = (
    ([1, 2, 3], False), ([2, 1, 2, 2], False), ([-1], False), ([-2, 1, -1], False), ([1, 1000, -1000], False),
    ([1], True), ([2], True), ([3, 1], True),
)
WIDE = [j // 2 + 1 if j % 2 == 0 else -(j // 2 + 1) for j in range(32)]   # f = 32, both signs

# (text, delim, rest, columns, row, quoted): include/mrx.h, "quoted fields"
TABLE = (
    (b'a,"b,c",d', b",", False, [1, 2, 3], [(0, 1), (3, 6), (8, 9)], [0, 1, 0]),
    (b'a,"b""c",d', b",", False, [2], [(3, 7)], [1]),
    (b'x,"",y', b",", False, [2], [(3, 3)], [1]),
    (b'"a,b', b",", False, [1, 2], [(0, 4), (-1, -1)], [0, 0]),
    (b'a"b,c"d', b",", False, [1], [(0, 7)], [0]),
    (b'"ab"cd,e', b",", False, [1, 2], [(0, 6), (7, 8)], [0, 0]),
    (b'"', b",", False, [1], [(0, 1)], [0]),
    (b'a "b c"  d', None, False, [1, 2, 3, -1], [(0, 1), (3, 6), (9, 10), (9, 10)], [0, 1, 0, 0]),
    (b'a,"b,c",d', b",", True, [2], [(2, 9)], [0]),
)


def _at(length, placed, fill=b"x"):
    t = bytearray(fill * length)
    for p, byte in placed.items():
        if 0 <= p < length:
            t[p] = byte
    return bytes(t)


def edges(G: int, sep: int):
    """One text per case for a group of G lanes; `sep` is the delimiter byte, or a whitespace byte."""
    R, q = 16 * G, Q[0]
    cases = {}
    for name, p in (("word", 16), ("round", R)):
        # ... sep " | sep(ignored) ... " sep ...
        cases["an opening quote ends a %s" % name] = _at(p + 30, {p - 2: sep, p - 1: q, p: sep, p + 9: q, p + 10: sep})
        cases["an opening quote ends a %s, never closed" % name] = _at(p + 20, {p - 1: q, p: sep, p + 5: sep})
        cases["a closing quote begins a %s" % name] = _at(p + 20, {p - 8: sep, p - 7: q, p - 3: sep, p: q, p + 1: sep, p + 6: sep})
        cases["a doubled quote across a %s edge" % name] = _at(
            p + 30, {p - 9: sep, p - 8: q, p - 4: sep, p - 1: q, p: q, p + 1: sep, p + 7: q, p + 8: sep})
        cases["a doubled quote behind a %s edge" % name] = _at(p + 30, {p - 6: sep, p - 5: q, p: q, p + 1: q, p + 2: sep, p + 7: q, p + 8: sep})
        cases["an empty quoted field across a %s edge" % name] = _at(p + 9, {p - 2: sep, p - 1: q, p: q, p + 1: sep})
    cases["a quoted field longer than two rounds"] = _at(
        3 * R + 20, {2: sep, 3: q, R + 1: sep, 2 * R - 1: sep, 2 * R: sep, 2 * R + 30: q, 2 * R + 31: sep})
    cases["unquoted, then a quote two rounds on"] = _at(2 * R + 20, {5: sep, 2 * R + 3: q, 2 * R + 5: sep, 2 * R + 9: q})
    for n in (1, 2, 3, 4, 15, 16, 17, R - 1, R, R + 1, 2 * R + 1):
        cases["%d quotes" % n] = Q * n
    s = bytes([sep])
    cases["quotes at both ends"] = Q + b"ab" + s + b"cd" + Q
    cases["a quote at byte 0"] = Q + b"ab" + s + b"cd"
    cases["a quote at the last byte"] = b"ab" + s + b"cd" + Q
    cases["a quote at both ends of every field"] = s.join(Q + b"f%d" % k + s + Q for k in range(2 * G + 3))
    cases["empty"] = b""
    cases["one separator"] = s
    cases["a separator between quotes"] = Q + s + Q
    for row in TABLE:
        cases["the table's %r" % row[0]] = row[0]
    return cases


def generated_texts(n: int, seed: int = 0):
    """n texts of 0 to 70 bytes over quotes, delimiters, whitespace and letters; empty ones first, last and in a run."""
    rng = np.random.default_rng(4000 + 13 * n + seed)
    al = np.frombuffer(b'ab,," \t"x', np.uint8)
    texts = [al[rng.integers(0, len(al), size=int(rng.integers(0, 71)))].tobytes() for _ in range(n)]
    for k in (0, n - 1, n // 2, n // 2 + 1):
        if 0 <= k < n:
            texts[k] = b""
    return texts


def csv_rows(n: int = 2000, seed: int = 20260101):
    """(lines, cells): n rows of 1 to 6 cells of 0 to 6 bytes over the alphabet ab," + space + x, written by csv.writer
    with QUOTE_MINIMAL and QUOTE_ALL in turn; the line terminator is taken off."""
    rng = np.random.default_rng(seed)
    al = 'ab," x'
    lines, cells = [], []
    for k in range(n):
        row = ["".join(al[int(c)] for c in rng.integers(0, len(al), size=int(rng.integers(0, 7))))
               for _ in range(int(rng.integers(1, 7)))]
        buf = io.StringIO()
        csv.writer(buf, quoting=csv.QUOTE_ALL if k % 2 else csv.QUOTE_MINIMAL, lineterminator="\n").writerow(row)
        line = buf.getvalue()
        assert line.endswith("\n") and len(line) > 1   # never an empty line for a row with a cell
        lines.append(line[:-1].encode())
        cells.append([c.encode() for c in row])
    return lines, cells


def combined_log_lines(n: int, seed: int = 0):
    """Access-log lines in the combined format: the request, the referrer and the agent stand in quotes, the agent with
    spaces, so that in whitespace mode the status is $7 and the size $8 only for a walk that knows the quotes."""
    rng = np.random.default_rng(90 + seed)
    out = []
    for _ in range(n):
        agent = b" ".join([b"Mozilla/5.0", b"(X11; Linux x86_64)", b"Gecko"][:int(rng.integers(1, 4))])
        out.append(b'10.0.0.%d - - [21/Oct/2026:13:00:%02d +0000] "GET /p/%d a HTTP/1.1" %d %d "-" "%s"' % (
            int(rng.integers(1, 255)), int(rng.integers(0, 60)), int(rng.integers(0, 1000)),
            (200, 404, 500)[int(rng.integers(0, 3))], int(rng.integers(0, 100000)), agent))
    return out
