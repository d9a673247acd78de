"""The batches of the fields tests, shared by the host walk (tests/test_fields_host.py) and the kernel
(tests/test_gpu_fields.py): the smallest texts at which a group of G lanes can go wrong.  A lane takes an aligned
16-byte word, a group G of them a round, so the edges are bytes 15 / 16 / 17 and 16 G - 1 / 16 G / 16 G + 1."""
from __future__ import annotations

import numpy as np

GROUPS = (1, 4, 16, 64)
# (columns, rest): every shape of request that the contract names
REQUESTS = (
    ([1], False), ([2, 1, 2], False), ([-1], False), ([-2, 1], False), ([1, 1000, -1000], False),
    ([1, 3, -1], False), ([1], True), ([3], True),
)
WIDE = [j // 2 + 1 if j % 2 == 0 else -(j // 2 + 1) for j in range(32)]   # f = 32, both signs
MODES = (b",", None)   # a delimiter byte, whitespace


def _at(length, positions, byte, fill=b"x"):
    t = bytearray(fill * length)
    for p in positions:
        if 0 <= p < length:
            t[p] = byte
    return bytes(t)


def edges(G: int, sep: int):
    """One text per case for a group of G lanes; `sep` is the delimiter byte, or a whitespace byte."""
    R = 16 * G   # a round
    s = bytes([sep])
    cases = {}
    for p in (15, 16, 17, R - 1, R, R + 1):
        cases["one separator at %d" % p] = _at(p + 9, [p], sep)
        cases["separators up to %d" % p] = _at(p + 3, [0, p - 1, p], sep)
        cases["the text ends behind %d" % p] = _at(p + 1, [p], sep)
    cases["a field from one round into the next"] = _at(R + 40, [R - 5, R + 7], sep)
    cases["a field longer than two rounds"] = _at(3 * R + 20, [3, 2 * R + 11], sep)
    cases["a run across a word edge"] = _at(40, [14, 15, 16, 17], sep)
    cases["a run across a round edge"] = _at(R + 20, [R - 2, R - 1, R, R + 1], sep)
    cases["a run that ends at a round's last byte"] = _at(R + 20, [R - 2, R - 1], sep)
    cases["a run that begins at a round's first byte"] = _at(R + 20, [R, R + 1], sep)
    cases["only separators"] = s * (R + 5)
    cases["only whitespace"] = b" \t\n\r\x0b\x0c" * (R // 6 + 2)
    for n in (0, 1, 15, 16, 17):
        cases["%d letters" % n] = b"y" * n
        cases["%d separators" % n] = s * n
        cases["%d bytes, separators at both ends" % n] = _at(n, [0, n - 1], sep)
    cases["three fields"] = b"a" + s + b"bb" + s + b"ccc"   # REST with cmax = 1, nf and nf + 1: columns [1], [3], [4]
    return cases


def rest_requests(nf: int):
    return [([1], True), ([nf], True), ([nf + 1], True), ([1, nf], True)] if nf > 0 else [([1], True)]


def short_texts(n: int, seed: int = 0):
    """n short texts over delimiters, whitespace and letters, with empty ones first, last and in runs."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    al = np.frombuffer(b"ab,, \t\n1;", np.uint8)
    texts = [al[rng.integers(0, len(al), size=int(rng.integers(0, 61)))].tobytes() for _ in range(n)]
    for k in (0, n - 1, n // 2, n // 2 + 1, n // 2 + 2):
        if 0 <= k < n:
            texts[k] = b""
    return texts


def log_lines(n: int, seed: int = 0):
    """Access-log-like lines: a key, 8 to 12 space-separated fields, a number in column 10 where there is one."""
    rng = np.random.default_rng(77 + seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(8, 13))
        fs = [b"host%d" % int(rng.integers(0, 9))] + [b"f%d" % int(rng.integers(0, 10 ** int(rng.integers(1, 6)))) for _ in range(k - 1)]
        if k >= 10:
            fs[9] = b"%d" % int(rng.integers(0, 100000))
        out.append(b" ".join(fs))
    return out
