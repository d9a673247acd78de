"""extract's expected answers, from the oracle only: the bytes under findall's spans (`mrx_ref.hybrid.findall`), under
split's ranges (`layouts.split_ranges` of those spans) and under one group of every captures_all row
(`captures_all_expect.expected_rows`), packed as the device packs them (the contract is in include/mrx.h,
mrx_gather_spans_dev).  The clamp of a span to its text is written once, in clamp().

Host-only: imports the oracle and numpy, neither torch nor the product library.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

import captures_all_expect as CA
import layouts as LY
from mrx_ref import hybrid as O

Pair = Tuple[int, int]
Packed = Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]   # prefix, owner, out_offsets, out_data


def clamp(s: int, e: int, length: int) -> Pair:
    """The piece of a text of `length` bytes under the pair (s, e): s' = min(max(s, 0), L), e' = min(max(e, s'), L)."""
    s2 = min(max(int(s), 0), length)
    return s2, min(max(int(e), s2), length)


def pack(rows: Sequence[Sequence[Pair]], texts: Sequence[bytes]) -> Packed:
    """rows[i]: the pairs of text i, in order.  (prefix int64[n + 1], owner int64[pieces], out_offsets
    int64[pieces + 1], out_data uint8[bytes])."""
    assert len(rows) == len(texts)
    prefix = np.zeros(len(texts) + 1, dtype=np.int64)
    owner, lens, parts = [], [], []
    for i, (t, rs) in enumerate(zip(texts, rows)):
        prefix[i + 1] = prefix[i] + len(rs)
        for s, e in rs:
            a, b = clamp(s, e, len(t))
            owner.append(i)
            lens.append(b - a)
            parts.append(t[a:b])
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    if lens:
        np.cumsum(lens, out=off[1:])
    data = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return prefix, np.array(owner, dtype=np.int64), off, data


def findall_rows(pat: bytes, texts: Sequence[bytes], cache=None) -> List[List[Pair]]:
    out = []
    for t in texts:
        key = (pat, t)
        if cache is not None and key in cache:
            out.append(cache[key])
            continue
        r = [(int(s), int(e)) for s, e in O.findall(pat, t)]
        if cache is not None:
            cache[key] = r
        out.append(r)
    return out


def expected_findall(pat: bytes, texts: Sequence[bytes], cache=None) -> Packed:
    """CompiledRegex.extract(texts): findall's matches."""
    return pack(findall_rows(pat, texts, cache), texts)


def expected_split(pat: bytes, texts: Sequence[bytes], maxsplit: int = 0, cache=None) -> Packed:
    """CompiledRegex.split_batch(texts, maxsplit)."""
    rows = [LY.split_ranges(r, len(t), maxsplit) for r, t in zip(findall_rows(pat, texts, cache), texts)]
    return pack(rows, texts)


def group_pair(group: int, g: int) -> int:
    """captures_all rows hold groups 1..g, then group 0: the pair of `group`."""
    return (group - 1) % (g + 1)


def expected_group(pat: bytes, texts: Sequence[bytes], group: int, count: int = 0) -> Packed:
    """CompiledRegex.extract(texts, group=group, count=count)."""
    g = CA.num_groups(pat)
    rows = [[tuple(row[group_pair(group, g)]) for row in CA.expected_rows(pat, t, count, g)] for t in texts]
    return pack(rows, texts)


def lists(packed: Packed) -> List[List[bytes]]:
    """The host-list form: the pieces of each text."""
    prefix, _, off, data = packed
    raw = data.tobytes()
    return [[raw[off[r]:off[r + 1]] for r in range(prefix[i], prefix[i + 1])] for i in range(len(prefix) - 1)]
