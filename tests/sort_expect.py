"""sort's and take's expected answers from Python itself: bytes compare bytewise and unsigned with a proper prefix first,
sorted() is stable, and collections.Counter.most_common() orders by descending count with ties in first-occurrence
order (the contract is in include/mrx.h, "sort" and "take").

Host-only: numpy, neither torch nor the product library.
"""
from __future__ import annotations

from collections import Counter
from typing import List, Optional, Sequence, Tuple

import numpy as np


def order(texts: Sequence[bytes]) -> np.ndarray:
    """order int64[n]: order[p] is the index of the text at sorted position p; equal texts in index order."""
    texts = [bytes(t) for t in texts]
    return np.array(sorted(range(len(texts)), key=texts.__getitem__), dtype=np.int64)


def rank(texts: Sequence[bytes]) -> Tuple[np.ndarray, int]:
    """(rank int64[n], u): the number of different texts smaller than text i, and the number of different texts."""
    texts = [bytes(t) for t in texts]
    where = {v: r for r, v in enumerate(sorted(set(texts)))}
    return np.array([where[t] for t in texts], dtype=np.int64), len(where)


def expected(texts: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray, int]:
    r, u = rank(texts)
    return order(texts), r, u


def packed(texts: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """(out_offsets int64[k + 1], out_data uint8[bytes]) of texts packed back to back, as take packs them."""
    texts = [bytes(t) for t in texts]
    off = np.zeros(len(texts) + 1, dtype=np.int64)
    if texts:
        np.cumsum([len(t) for t in texts], out=off[1:])
    return off, np.frombuffer(b"".join(texts), dtype=np.uint8).copy()


def take(texts: Sequence[bytes], index: Sequence[int]) -> List[bytes]:
    return [bytes(texts[int(i)]) for i in index]


def value_counts(pieces: Sequence[bytes], sort: Optional[str] = None, top: Optional[int] = None) -> List[Tuple[bytes, int]]:
    """[(value, count)]: None = first-occurrence order (Counter.items()), "value" = ascending by value, "count" =
    Counter.most_common(); top keeps the first rows of that order."""
    counted = Counter(bytes(p) for p in pieces)
    rows = {None: list(counted.items()), "value": sorted(counted.items()), "count": counted.most_common()}[sort]
    return rows if top is None else rows[:top]
