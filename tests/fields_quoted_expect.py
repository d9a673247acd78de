"""What quoted fields must give, in pure Python (include/mrx.h, "quoted fields"): one pass over the bytes with a
two-state machine (outside / inside) that knows no words, groups, rounds or parities of masks, and never calls the
library.  tests/test_fields_quoted_host.py pins it against the contract's table, against csv.reader and against
tests/fields_expect.py."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from fields_expect import WHITESPACE


def separators(t: bytes, quote: bytes, delim: Optional[bytes] = None) -> List[bool]:
    """Per byte: does it separate.  A quote byte turns the state over; a delimiter (a whitespace byte with delim=None)
    separates when the state is outside."""
    q, inside, out = quote[0], False, []
    for b in t:
        if b == q:
            inside = not inside
            out.append(False)
        else:
            out.append(not inside and (b == delim[0] if delim is not None else b in WHITESPACE))
    return out


def parts(t: bytes, quote: bytes, delim: Optional[bytes] = None, maxsplit: int = -1) -> List[Tuple[int, int]]:
    """The (start, end) of every part, quotes still on: split(delim, maxsplit) over the separating bytes alone."""
    sep, out, L = separators(t, quote, delim), [], len(t)
    if delim is not None:
        start = 0
        for i in range(L):
            if sep[i] and (maxsplit < 0 or len(out) < maxsplit):
                out.append((start, i))
                start = i + 1
        out.append((start, L))
        return out
    i = 0
    while True:
        while i < L and sep[i]:
            i += 1
        if i == L:
            return out
        if 0 <= maxsplit == len(out):
            out.append((i, L))
            return out
        start = i
        while i < L and not sep[i]:
            i += 1
        out.append((start, i))


def content(t: bytes, quote: bytes, s: int, e: int) -> Tuple[int, int, int]:
    """(start, end, quoted) of a part's content: a part of two bytes or more between two quotes loses both."""
    if e - s >= 2 and t[s] == quote[0] and t[e - 1] == quote[0]:
        return s + 1, e - 1, 1
    return s, e, 0


def row(t: bytes, columns: Sequence[int], quote: bytes, delim: Optional[bytes] = None, rest: bool = False):
    """(pairs, nf, quoted) of one text."""
    ps = parts(t, quote, delim, max(columns) - 1 if rest else -1)
    nf = len(ps)
    pairs, quoted = [], []
    for c in columns:
        k = c - 1 if c > 0 else nf + c
        s, e, was = content(t, quote, *ps[k]) if 0 <= k < nf else (-1, -1, 0)
        pairs.append((s, e))
        quoted.append(was)
    return pairs, nf, quoted


def expected(texts: Sequence[bytes], columns: Sequence[int], quote: bytes, delim: Optional[bytes] = None, rest: bool = False):
    """(rows int32[n, f, 2], nf int32[n], prefix int64[n + 1], quoted uint8[n, f])."""
    n = len(texts)
    rows, nf, quoted = np.zeros((n, len(columns), 2), np.int32), np.zeros(n, np.int32), np.zeros((n, len(columns)), np.uint8)
    for i, t in enumerate(texts):
        pairs, nf[i], quoted[i] = row(t, columns, quote, delim, rest)
        rows[i] = pairs
    return rows, nf, np.arange(n + 1, dtype=np.int64), quoted


def decoded(t: bytes, quote: bytes, s: int, e: int) -> bytes:
    """The decoded cell of a content: every leftmost non-overlapping QQ is one Q.  bytes.replace is exactly that."""
    return t[s:e].replace(quote + quote, quote) if s >= 0 else b""


def cells(t: bytes, quote: bytes = b'"', delim: bytes = b",") -> List[bytes]:
    """All decoded cells of a text, as csv.reader would list them for a well-formed row."""
    return [decoded(t, quote, *content(t, quote, s, e)[:2]) for s, e in parts(t, quote, delim)]
