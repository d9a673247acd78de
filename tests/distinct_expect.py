"""distinct's expected answers from a Python dict in insertion order: the group of every text, the first index and the
count of every group, and the values packed as the device packs them (the contract is in include/mrx.h, "distinct").

Host-only: numpy, neither torch nor the product library.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

Expected = Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]   # group_of, first, counts, offsets, data


def expected(texts: Sequence[bytes]) -> Expected:
    """(group_of int64[n], first int64[u], counts int64[u], out_offsets int64[u + 1], out_data uint8[bytes])."""
    groups = {}   # text -> group, in the order of first occurrence
    group_of, first, counts = [], [], []
    for i, t in enumerate(texts):
        t = bytes(t)
        g = groups.setdefault(t, len(groups))
        if g == len(first):
            first.append(i)
            counts.append(0)
        counts[g] += 1
        group_of.append(g)
    values = list(groups)
    off = np.zeros(len(values) + 1, dtype=np.int64)
    if values:
        np.cumsum([len(v) for v in values], out=off[1:])
    data = np.frombuffer(b"".join(values), dtype=np.uint8).copy()
    return (np.array(group_of, dtype=np.int64), np.array(first, dtype=np.int64), np.array(counts, dtype=np.int64), off,
            data)


def values(exp: Expected) -> List[bytes]:
    raw = exp[4].tobytes()
    return [raw[exp[3][g]:exp[3][g + 1]] for g in range(len(exp[1]))]


def value_counts(pieces: Sequence[bytes]) -> List[Tuple[bytes, int]]:
    """[(value, count)] in first-occurrence order: list(collections.Counter(pieces).items())."""
    exp = expected(pieces)
    return list(zip(values(exp), exp[2].tolist()))
