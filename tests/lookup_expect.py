"""A dictionary's expected answers from a Python dict: for every text the lowest index of an entry equal to it, or -1, and
the filter's output packed as the device packs it (the contract is in include/mrx.h, "dictionaries").

Host-only: numpy, neither torch nor the product library.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np


def expected(entries: Sequence[bytes], texts: Sequence[bytes]) -> np.ndarray:
    """int64[n]: the lowest j with entries[j] == texts[i], -1 when there is none."""
    lowest = {}
    for j, e in enumerate(entries):
        lowest.setdefault(bytes(e), j)
    return np.array([lowest.get(bytes(t), -1) for t in texts], dtype=np.int64)


def filtered(entries: Sequence[bytes], texts: Sequence[bytes], invert: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The device's output form: (kept_idx int64[kept], out_offsets int64[kept + 1], out_data uint8[bytes]); a text is
    kept when it is an entry, with `invert` when it is none."""
    index = expected(entries, texts)
    idx = np.array([i for i in range(len(texts)) if (index[i] >= 0) != bool(invert)], dtype=np.int64)
    kept = [bytes(texts[int(i)]) for i in idx]
    off = np.zeros(len(kept) + 1, dtype=np.int64)
    if kept:
        np.cumsum([len(t) for t in kept], out=off[1:])
    data = np.frombuffer(b"".join(kept), dtype=np.uint8).copy()
    return idx, off, data
