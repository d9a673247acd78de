"""filter's expected answers, from the oracle only: text i is kept when `mrx_ref.hybrid.compile_regex(p).test(text)`
says so -- for a set, when some member's test does (mode "any") or every member's (mode "all"); invert negates.  With no
member at all, "any" is false and "all" is true for every text.  Kept texts keep their order; a kept empty text adds no
byte and repeats its offset (the contract is in include/mrx.h, mrx_filter_dev).

Host-only: imports the oracle and numpy, neither torch nor the product library.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from mrx_ref import hybrid as O


def keep_flags(patterns: Sequence[bytes], texts: Sequence[bytes], mode: str = "any", invert: bool = False,
               cache=None) -> List[bool]:
    """One flag per text.  `patterns` is a list (a single pattern: a list of one).  `cache` (a dict) keeps the oracle's
    answer per (pattern, text)."""
    assert mode in ("any", "all")
    rxs = [O.compile_regex(p) for p in patterns]

    def hit(j, t):
        key = (patterns[j], t)
        if cache is not None and key in cache:
            return cache[key]
        v = bool(rxs[j].test(t))
        if cache is not None:
            cache[key] = v
        return v

    out = []
    for t in texts:
        if mode == "all":
            h = all(hit(j, t) for j in range(len(rxs)))
        else:
            h = any(hit(j, t) for j in range(len(rxs)))
        out.append(h != bool(invert))
    return out


def expected(patterns: Sequence[bytes], texts: Sequence[bytes], mode: str = "any", invert: bool = False,
             cache=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The device's output form: (kept_idx int64[kept], out_offsets int64[kept + 1], out_data uint8[bytes])."""
    flags = keep_flags(patterns, texts, mode, invert, cache)
    idx = np.array([i for i, f in enumerate(flags) if f], dtype=np.int64)
    kept = [texts[int(i)] for i in idx]
    off = np.zeros(len(kept) + 1, dtype=np.int64)
    if kept:
        np.cumsum([len(t) for t in kept], out=off[1:])
    data = np.frombuffer(b"".join(kept), dtype=np.uint8).copy()
    return idx, off, data


def expected_lists(patterns, texts, mode: str = "any", invert: bool = False, cache=None) -> Tuple[List[bytes], np.ndarray]:
    """The host-list wrappers' form: (kept texts, kept_idx int64[kept])."""
    idx, _, _ = expected(patterns, texts, mode, invert, cache)
    return [texts[int(i)] for i in idx], idx
