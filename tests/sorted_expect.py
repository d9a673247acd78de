"""What the sorted index (include/mrx.h, "sorted index") must answer, in plain Python: sorted() for the order, bisect for
EQUAL, startswith over the sorted entries for PREFIX and a brute force over all entries for LONGEST.  Host-only."""
from bisect import bisect_left, bisect_right
from typing import List, Sequence, Tuple

import numpy as np

EQUAL, PREFIX, LONGEST = 0, 1, 2


def order(entries: Sequence[bytes]) -> np.ndarray:
    """order[p]: the original index of the entry at sorted position p; equal entries in ascending index (sorted() is
    stable)."""
    return np.array(sorted(range(len(entries)), key=entries.__getitem__), dtype=np.int64)


def search(entries: Sequence[bytes], texts: Sequence[bytes], mode: int) -> Tuple[np.ndarray, np.ndarray]:
    """(lo int64[n], hi int64[n]) of one mode."""
    srt = sorted(entries)
    lo, hi = np.zeros(len(texts), np.int64), np.zeros(len(texts), np.int64)
    for i, t in enumerate(texts):
        if mode == EQUAL:
            lo[i], hi[i] = bisect_left(srt, t), bisect_right(srt, t)
        elif mode == PREFIX:
            with_it = [p for p, e in enumerate(srt) if e.startswith(t)]
            if with_it:
                assert with_it == list(range(with_it[0], with_it[-1] + 1))   # one contiguous range of the order
                lo[i], hi[i] = with_it[0], with_it[-1] + 1
            else:
                lo[i] = hi[i] = bisect_left(srt, t)
        else:
            best = -1
            for p, e in enumerate(srt):   # the lowest position of the longest one: a later one must be longer
                if t.startswith(e) and (best < 0 or len(e) > len(srt[best])):
                    best = p
            lo[i], hi[i] = best, (len(srt[best]) if best >= 0 else -1)
    return lo, hi


def index(entries: Sequence[bytes], texts: Sequence[bytes]) -> List[int]:
    """The lowest original index of an entry equal to the text, or -1."""
    where = {}
    for j, e in enumerate(entries):
        where.setdefault(e, j)
    return [where.get(t, -1) for t in texts]
