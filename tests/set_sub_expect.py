"""PatternSet.sub's expected answers, restated from the oracle (the contract is in include/mrx.h, mrx_set_sub_dev):
the candidates are every member's findall hits (s, j, e); in ascending (s, j) order a candidate is selected iff it
starts at or after pos, then pos = max(e, s + 1); each selected [s, e) is replaced by member j's replacement.

Host-only: imports the oracle and numpy, neither torch nor the product library.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from mrx_ref import hybrid as O


def expected_sub(patterns: Sequence[bytes], repls: Sequence[bytes], text: bytes, count: int = 0,
                 cache=None) -> Tuple[bytes, int]:
    """(output, number of replacements) for one text.  `cache` (a dict) keeps the oracle's findall per (pattern, text)."""
    hits = []
    for j, p in enumerate(patterns):
        spans = cache.get((p, text)) if cache is not None else None
        if spans is None:
            spans = [tuple(x) for x in O.findall(p, text)]
            if cache is not None:
                cache[(p, text)] = spans
        hits += [(s, j, e) for s, e in spans]
    hits.sort()
    out, cur, pos, reps = [], 0, 0, 0
    for s, j, e in hits:
        if s < pos:
            continue
        out += [text[cur:s], repls[j]]
        cur, pos, reps = e, max(e, s + 1), reps + 1
        if count and reps == count:
            break
    return b"".join(out) + text[cur:], reps


def expected_lists(patterns, repls, texts, count: int = 0, cache=None) -> Tuple[List[bytes], List[int]]:
    """expected_sub over a batch: (outputs, replacement counts)."""
    res = [expected_sub(patterns, repls, t, count, cache) for t in texts]
    return [r[0] for r in res], [r[1] for r in res]


def expected_arrays(patterns, repls, texts, count: int = 0, cache=None):
    """The device's output form: (out_offsets int64[n+1], out_data uint8[total], nsub int32[n])."""
    outs, reps = expected_lists(patterns, repls, texts, count, cache)
    off = np.zeros(len(outs) + 1, dtype=np.int64)
    np.cumsum([len(o) for o in outs], out=off[1:])
    data = np.frombuffer(b"".join(outs), dtype=np.uint8).copy()
    return off, data, np.array(reps, dtype=np.int32)
