"""PatternSet.findall's expected answers, restated from the oracle: for each text, the oracle's findall of member 0, then
of member 1, and so on (the contract is in include/mrx.h, mrx_set_findall_dev).

Host-only: imports the oracle, neither torch nor the product library.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from mrx_ref import hybrid as O

Hit = Tuple[int, int, int]   # (member, start, end)


def expected_lists(patterns: Sequence[bytes], texts: Sequence[bytes], cache=None) -> List[List[Hit]]:
    """Per text: every member's findall spans, member order then match order.  `cache` (a dict) keeps the oracle's
    answers per (pattern, text) across calls."""
    out = []
    for t in texts:
        row = []
        for j, p in enumerate(patterns):
            key = (p, t)
            spans = cache.get(key) if cache is not None else None
            if spans is None:
                spans = [tuple(s) for s in O.findall(p, t)]
                if cache is not None:
                    cache[key] = spans
            row += [(j, a, b) for a, b in spans]
        out.append(row)
    return out


def expected_arrays(patterns: Sequence[bytes], texts: Sequence[bytes], cache=None):
    """The same in the device's output form: (text_prefix int64[n+1], members int32[total], spans int32[total, 2])."""
    return to_arrays(expected_lists(patterns, texts, cache))


def to_arrays(lists: Sequence[Sequence[Hit]]):
    prefix = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in lists], out=prefix[1:])
    flat = [h for r in lists for h in r]
    members = np.array([h[0] for h in flat], dtype=np.int32)
    spans = np.array([(h[1], h[2]) for h in flat], dtype=np.int32).reshape(-1, 2)
    return prefix, members, spans


def regroup(per_member: Sequence[Tuple[np.ndarray, np.ndarray]], n: int):
    """The members' own findall results (counts_prefix int64[n+1], spans int32[t, 2]) regrouped by text, in the set's
    output form: a stable sort by text of the members' hits laid out member after member."""
    text_of, member_of, spans_of = [], [], []
    for j, (prefix, spans) in enumerate(per_member):
        prefix = np.asarray(prefix)
        text_of.append(np.repeat(np.arange(n, dtype=np.int64), np.diff(prefix)))
        member_of.append(np.full(int(prefix[n]), j, dtype=np.int32))
        spans_of.append(np.asarray(spans, dtype=np.int32).reshape(-1, 2)[: int(prefix[n])])
    text_of = np.concatenate(text_of) if text_of else np.zeros(0, np.int64)
    order = np.argsort(text_of, kind="stable")
    out_prefix = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(text_of, minlength=n)[:n], out=out_prefix[1:])
    members = np.concatenate(member_of)[order] if member_of else np.zeros(0, np.int32)
    spans = np.concatenate(spans_of)[order] if spans_of else np.zeros((0, 2), np.int32)
    return out_prefix, members, spans
