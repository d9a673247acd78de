"""What Keywords.leftmost and Keywords.sub answer (include/mrx.h, "keywords: leftmost-longest matches and replacement"),
computed without any automaton: re.finditer over the escaped distinct entries, longest first, joined by `|` -- at every
position the alternation tries the longest entry first, and finditer goes on behind a match, which is the definition's
loop.  leftmost_slow is that loop itself, letter by letter; the host tests hold the two together."""
from __future__ import annotations

import re
from typing import List, Sequence, Tuple

import numpy as np

from keywords_expect import arrays, distinct_entries, generated  # noqa: F401  (arrays and generated: for the tests)


def _matcher(entries: Sequence[bytes], ignore_case: bool):
    d = distinct_entries(entries, ignore_case)
    if not d:
        return None, {}
    d.sort(key=lambda je: len(je[1]), reverse=True)
    rx = re.compile(b"|".join(re.escape(e) for _, e in d), re.IGNORECASE if ignore_case else 0)
    return rx, {e: j for j, e in d}


def leftmost_dict(entries: Sequence[bytes], texts: Sequence[bytes], ignore_case: bool = False, count: int = 0):
    """The definition with a dict of the entries, for sets of 10^4 entries, where an alternation of as many branches
    takes a minute: at every position from pos on the slices of every entry length, longest first."""
    index = {e: j for j, e in distinct_entries(entries, ignore_case)}
    lengths = sorted({len(e) for e in index}, reverse=True)
    out = []
    for t in texts:
        t = bytes(t).lower() if ignore_case else bytes(t)
        row, s = [], 0
        while s < len(t) and not (count and len(row) == count):
            for k in lengths:
                j = index.get(t[s:s + k]) if s + k <= len(t) else None
                if j is not None:
                    row.append((j, s, s + k))
                    s += k
                    break
            else:
                s += 1
        out.append(row)
    return out


def leftmost(entries: Sequence[bytes], texts: Sequence[bytes], ignore_case: bool = False, count: int = 0):
    """Per text the (entry, start, end) of its leftmost-longest matches in ascending start order, the first `count` of
    them with count > 0."""
    if len(entries) > 2000:
        return leftmost_dict(entries, texts, ignore_case, count)
    rx, index = _matcher(entries, ignore_case)
    out = []
    for t in texts:
        t = bytes(t)
        row = []
        if rx is not None:
            for m in rx.finditer(t):
                g = m.group()
                row.append((index[g.lower() if ignore_case else g], m.start(), m.end()))
                if count and len(row) == count:
                    break
        out.append(row)
    return out


def leftmost_slow(entries: Sequence[bytes], texts: Sequence[bytes], ignore_case: bool = False, count: int = 0):
    """The definition: the smallest s >= pos at which an entry occurs, the longest entry there, pos = its end."""
    d = distinct_entries(entries, ignore_case)
    out = []
    for t in texts:
        t = bytes(t).lower() if ignore_case else bytes(t)
        row, pos = [], 0
        while pos < len(t) and not (count and len(row) == count):
            best = None
            for s in range(pos, len(t)):
                for j, e in d:
                    if t.startswith(e, s) and (best is None or len(e) > best[2] - best[1]):
                        best = (j, s, s + len(e))
                if best:
                    break
            if not best:
                break
            row.append(best)
            pos = best[2]
        out.append(row)
    return out


def sub(entries: Sequence[bytes], repl, texts: Sequence[bytes], ignore_case: bool = False, count: int = 0):
    """(outputs List[bytes], nsub int32[n]): every text with its kept matches replaced -- by repl (bytes: one for all)
    or by repl[entry] -- and every other byte as it stands."""
    outs, ns = [], []
    for t, row in zip(texts, leftmost(entries, texts, ignore_case, count)):
        t = bytes(t)
        parts, prev = [], 0
        for j, s, e in row:
            parts += [t[prev:s], repl if isinstance(repl, bytes) else repl[j]]
            prev = e
        parts.append(t[prev:])
        outs.append(b"".join(parts))
        ns.append(len(row))
    return outs, np.array(ns, np.int32)
