"""What fields must give, in pure Python: a walk over byte positions that knows no words, groups or rounds, and never
calls the library.  tests/test_fields_host.py pins it against bytes.split itself."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

WHITESPACE = b"\t\n\x0b\x0c\r "   # the six bytes of the contract (include/mrx.h, "fields")


def parts(t: bytes, delim: Optional[bytes] = None, maxsplit: int = -1) -> List[Tuple[int, int]]:
    """The (start, end) of every part of t.split(delim, maxsplit), delim=None being bytes.split()'s whitespace rule."""
    out, L = [], len(t)
    if delim is not None:
        d, start = delim[0], 0
        for i in range(L):
            if t[i] == d and (maxsplit < 0 or len(out) < maxsplit):
                out.append((start, i))
                start = i + 1
        out.append((start, L))
        return out
    i = 0
    while True:
        while i < L and t[i] in WHITESPACE:
            i += 1
        if i == L:
            return out
        if 0 <= maxsplit == len(out):
            out.append((i, L))   # the rest, trailing whitespace included
            return out
        start = i
        while i < L and t[i] not in WHITESPACE:
            i += 1
        out.append((start, i))


def row(t: bytes, columns: Sequence[int], delim: Optional[bytes] = None, rest: bool = False):
    """(pairs, nf) of one text."""
    ps = parts(t, delim, max(columns) - 1 if rest else -1)
    nf = len(ps)
    pairs = []
    for c in columns:
        q = c - 1 if c > 0 else nf + c
        pairs.append(ps[q] if 0 <= q < nf else (-1, -1))
    return pairs, nf


def expected(texts: Sequence[bytes], columns: Sequence[int], delim: Optional[bytes] = None, rest: bool = False):
    """(rows int32[n, f, 2], nf int32[n], prefix int64[n + 1])."""
    n = len(texts)
    rows, nf = np.zeros((n, len(columns), 2), np.int32), np.zeros(n, np.int32)
    for i, t in enumerate(texts):
        pairs, nf[i] = row(t, columns, delim, rest)
        rows[i] = pairs
    return rows, nf, np.arange(n + 1, dtype=np.int64)
