"""What a keyword set answers (include/mrx.h, "keywords"), computed without any automaton: bytes.find per entry, every
occurrence, sorted by (end, start).  Equal entries stand under the lowest index among them; with ignore_case the entries
and the text go through bytes.lower(), which folds ASCII A-Z and nothing else."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np


def distinct_entries(entries: Sequence[bytes], ignore_case: bool = False) -> List[Tuple[int, bytes]]:
    """(lowest index, folded bytes) of every different entry."""
    seen = {}
    for j, e in enumerate(entries):
        e = bytes(e).lower() if ignore_case else bytes(e)
        assert e, "an empty entry is refused by the build"
        seen.setdefault(e, j)
    return [(j, e) for e, j in seen.items()]


def findall_one(distinct, text: bytes, ignore_case: bool = False) -> List[Tuple[int, int, int]]:
    t = text.lower() if ignore_case else text
    hits = []
    for j, e in distinct:
        at = t.find(e)
        while at >= 0:
            hits.append((j, at, at + len(e)))
            at = t.find(e, at + 1)
    hits.sort(key=lambda h: (h[2], h[1]))
    return hits


def findall(entries: Sequence[bytes], texts: Sequence[bytes], ignore_case: bool = False) -> List[List[Tuple[int, int, int]]]:
    """Per text the (entry, start, end) of every hit, in ascending (end, start) order."""
    d = distinct_entries(entries, ignore_case)
    return [findall_one(d, bytes(t), ignore_case) for t in texts]


def arrays(hits: List[List[Tuple[int, int, int]]]):
    """(text_prefix int64[n + 1], entries int32[total], spans int32[total, 2]) of findall()'s lists."""
    prefix = np.zeros(len(hits) + 1, np.int64)
    np.cumsum([len(h) for h in hits], out=prefix[1:])
    flat = [h for row in hits for h in row]
    ents = np.array([h[0] for h in flat], np.int32)
    spans = np.array([[h[1], h[2]] for h in flat], np.int32).reshape(-1, 2)
    return prefix, ents, spans


def counts(hits) -> np.ndarray:
    return np.array([len(h) for h in hits], np.int64)


def filtered(hits, texts: Sequence[bytes], invert: bool = False):
    """(kept_idx int64[kept], out_offsets int64[kept + 1], out bytes) of filter with the predicate `contains`."""
    idx = [i for i, h in enumerate(hits) if bool(h) != invert]
    off = np.zeros(len(idx) + 1, np.int64)
    np.cumsum([len(texts[i]) for i in idx], out=off[1:])
    return np.array(idx, np.int64), off, b"".join(bytes(texts[i]) for i in idx)


def generated(rng, m: int, n: int, alphabet: bytes = b"abc", max_entry: int = 40, max_text: int = 100):
    """m entries of 1..max_entry bytes and n texts of 0..max_text bytes over a small alphabet, so that failure links and
    output chains are taken; some entries are cut out of the texts, some are prefixes or suffixes of others, some repeat."""
    al = np.frombuffer(alphabet, np.uint8)

    def run(k):
        return al[rng.integers(0, len(al), size=int(k))].tobytes()

    texts = [run(rng.integers(0, max_text + 1)) for _ in range(n)]
    entries = []
    while len(entries) < m:
        kind = int(rng.integers(0, 6))
        if kind == 0 and entries:
            e = entries[int(rng.integers(0, len(entries)))]                 # a duplicate
        elif kind == 1 and entries:
            e = entries[int(rng.integers(0, len(entries)))]
            e = e[int(rng.integers(0, len(e))):]                            # a suffix of another entry
        elif kind == 2 and entries:
            e = entries[int(rng.integers(0, len(entries)))]
            e = e[:int(rng.integers(1, len(e) + 1))]                        # a prefix
        elif kind == 3:
            t = texts[int(rng.integers(0, n))] if n else b""
            a = int(rng.integers(0, len(t) + 1))
            e = t[a:a + int(rng.integers(1, max_entry + 1))]                # cut out of a text
        else:
            short = rng.random() < 0.6
            e = run(rng.integers(1, 5 if short else max_entry + 1))
        if e:
            entries.append(e[:max_entry])
    return entries, texts
