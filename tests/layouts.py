"""Device-batch layouts whose out-of-text bytes are adversarial for a pattern.

Every device entry point takes the same texts as CSR (`offsets`), as fixed-pitch rows with one common `length`, or as
fixed-pitch rows with per-text `lens`.  Text i's answer may depend on text i's bytes only: its CSR neighbours, the
bytes before offsets[0] and after offsets[n], and a row's tail past its length are never text.  The builders here put
bytes there that a careless kernel WOULD turn into a different answer: the pattern's own literal bytes and class
members, the literal's remainder after any of its prefixes, and the text itself repeated (so that a partial match at
the end of a text continues, and an end-anchored match stops being at the end).  The poison always lies inside the
allocated buffer.

Host-only (numpy and the oracle); `Layout.device()` uploads a layout as a DeviceBatch.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from mrx_ref import hybrid as O

# One pattern per plan family (the GPU module asserts from describe() that every family is present).
PATTERNS = [
    b"[a-z]+\\d+", b"\\d+", b"[^0-9]+", b"(x|y|foo|bar)+",                           # streamable: byte columns
    b"(\\d{3})(\\d{3})(\\d{4})",                                                      # streamable: class table
    b"aaaaaaaaaaaaaaaaaaaaaa", b"xyxyxyxyxyxyxyxyxyxyxyxyxy", b"hello world this is long",  # exact literals
    b"hello", b"abab",                                                                # pure literals
    b"\\w+@\\w+\\.com",                                                               # prefilter
    b"^[a-z]+\\d+", b"^abc",                                                          # '^'
    b"^abc$", b"a$",                                                                  # '$' on the anchored DFA
    b"[a-z]+$", b"(foo|[0-9]+)$",                                                     # '$' on the LazyDFA search
    b"\\w+\\d{2}", b"\\d+(\\.\\d+)?",                                                 # stepper, multi-walk
    b"foo|[a-z]{3}\\d|[ab]",                                                          # pending-tries walk
    b"\\d{3}-\\d{4}",                                                                 # required-byte route
    b"[A-Z]{10,20}[0-9]{15,25}|ab",                                                   # backward marks + stepper
    b"x*", b"a+b*",                                                                   # empty matches
    b"(a|b)*a(a|b){12}",                                                              # bitset NFA
    b"hello.*", b".*",                                                                # backtracker route, '.*'
    b"x(\\d)?",                                                                       # fixed-width groups
    b"(\\w+) (\\w+)", b"(a|ab)(c|bcd)(d*)",                                           # general groups
]

CSR_SHIFTS = (1, 7, 15)
WHOLE_ROW_STRIDES = (48, 64, 50, 1001)
FIXED_LENGTH = ((64, 45), (50, 37))   # (stride, common length)

_CLASSES = {
    ord("d"): b"0123456789", ord("w"): b"abcxyzAZ_0189", ord("s"): b" \t\n", ord("D"): b"ax -", ord("W"): b" -.@",
    ord("S"): b"ax19", ord("b"): b"", ord("B"): b"",
}


def pattern_bytes(pat: bytes) -> Tuple[bytes, bytes]:
    """(bytes that can extend a match of `pat`: its literal bytes and class members, its longest literal run)."""
    members, runs, cur = bytearray(), [], bytearray()
    i = 0

    def cut():
        if cur:
            runs.append(bytes(cur))
            cur.clear()

    while i < len(pat):
        c = pat[i]
        if c == 0x5C and i + 1 < len(pat):                       # escape
            e = pat[i + 1]
            i += 2
            if e in _CLASSES:
                members.extend(_CLASSES[e])
                cut()
            elif e == ord("x") and i + 2 <= len(pat):
                v = int(pat[i:i + 2], 16)
                i += 2
                cur.append(v)
                members.append(v)
            else:
                cur.append(e)
                members.append(e)
        elif c == ord("["):                                       # class: its members (a sample of the complement)
            j = i + 1
            neg = j < len(pat) and pat[j] == ord("^")
            j += 1 if neg else 0
            body = bytearray()
            while j < len(pat) and (pat[j] != ord("]") or j == i + 1 + neg):
                if pat[j] == 0x5C and j + 1 < len(pat):
                    e = pat[j + 1]
                    body.extend(_CLASSES.get(e, bytes([e])))
                    j += 2
                elif j + 2 < len(pat) and pat[j + 1] == ord("-") and pat[j + 2] != ord("]"):
                    lo, hi = pat[j], pat[j + 2]
                    body.extend(range(lo, hi + 1, max(1, (hi - lo) // 6)))
                    body.append(hi)
                    j += 3
                else:
                    body.append(pat[j])
                    j += 1
            i = j + 1
            members.extend(bytes(b for b in b"abxyz019 -.@_AZ" if b not in body) if neg else body)
            cut()
        elif c == ord("{"):
            i = pat.index(b"}", i) + 1
            cut()
        elif c == ord("(") and pat[i + 1:i + 3] == b"?:":
            i += 3
            cut()
        elif c in b"()|*+?^$":
            i += 1
            cut()
        elif c == ord("."):
            members.extend(b"ax0 ")
            i += 1
            cut()
        else:
            cur.append(c)
            members.append(c)
            i += 1
    cut()
    lit = max(runs, key=len) if runs else b""
    return bytes(members) or b"a", lit


def poison(pat: bytes, text: bytes, size: int, rng) -> bytes:
    """`size` bytes that would change `pat`'s answer on `text` if a kernel read them as text following it."""
    if size <= 0:
        return b""
    members, lit = pattern_bytes(pat)
    m = np.frombuffer(members, dtype=np.uint8)

    def run(k):
        return bytes(m[rng.integers(0, len(m), size=k)].tolist())

    parts = []
    kind = int(rng.integers(0, 4))
    if kind == 0:                          # continue a run of the pattern's classes
        parts.append(run(int(rng.integers(1, 9))))
    elif kind == 1 and lit:                # complete a prefix of the literal that ends the text
        parts.append(lit[int(rng.integers(0, len(lit))):])
    elif kind == 2 and text:               # the text once more: its partial match at the end goes on
        parts.append(text[-64:])
    parts += [lit, run(6), text[:32], lit, run(12)]
    out = b"".join(parts)
    while len(out) < size:
        out += lit + run(16) + text[:16]
    return out[:size]


def make_texts(pat: bytes, n: int, n_long: int = 8, seed: int = 0) -> List[bytes]:
    """Seeded texts for one pattern: mostly 0-200 bytes over an alphabet rich in the pattern's bytes, empty texts,
    texts cut right after a match (it ends at their last byte), texts that are one match, and `n_long` texts of
    2-6 KiB."""
    rng = np.random.default_rng(zlib.crc32(pat) + seed)
    members, lit = pattern_bytes(pat)
    al = np.frombuffer(b"abcxyz0189 -.@_fohelw" + members * 2 + lit, dtype=np.uint8)

    def rnd(k):
        t = al[rng.integers(0, len(al), size=k)].tobytes()
        if lit and k > len(lit) and rng.random() < 0.5:      # plant the literal, at the start one time in three
            p = 0 if rng.random() < 0.33 else int(rng.integers(0, k - len(lit) + 1))
            t = t[:p] + lit + t[p + len(lit):]
        return t

    texts = [b"", b"", lit, lit + lit, lit[:-1] if lit else b"a"]
    n_cut = max(1, n // 10)
    while len(texts) < n - n_long - 2 * n_cut:
        texts.append(rnd(int(rng.integers(0, 201))))
    for k in range(2 * n_cut):        # a match ends at the text's last byte; every other one is that match alone
        t = rnd(int(rng.integers(8, 160)))
        spans = [s for s in O.findall(pat, t) if s[1] > s[0]]
        s = spans[int(rng.integers(0, len(spans)))] if spans else (0, len(t))
        texts.append(t[s[0] if k % 2 else 0:s[1]])
    for _ in range(n_long):
        texts.append(rnd(int(rng.integers(2048, 6 * 1024 + 1))))
    order = rng.permutation(len(texts))
    return [texts[int(k)] for k in order]


@dataclass
class Layout:
    """One batch: `texts[i]` lies in `buf` at offsets[i]..offsets[i+1] (CSR) or at i * stride, length lens[i] or
    `length` (fixed pitch).  Everything else in `buf` is poison."""
    name: str
    buf: np.ndarray
    texts: List[bytes]
    offsets: Optional[np.ndarray] = None
    stride: int = 0
    length: int = 0
    lens: Optional[np.ndarray] = None
    known: bool = False       # CSR built with from_texts (offsets[n] and the longest text known on the host)

    @property
    def csr(self) -> bool:
        return self.offsets is not None

    @property
    def aligned(self) -> bool:
        return self.csr or self.stride % 16 == 0

    def span(self, i: int) -> Tuple[int, int]:
        if self.csr:
            return int(self.offsets[i]), int(self.offsets[i + 1])
        a = i * self.stride
        return a, a + (int(self.lens[i]) if self.lens is not None else self.length)

    def outside(self, i: int, k: int = 128) -> bytes:
        """The bytes a kernel that overran text i's end would read first (rest of the row, the next texts)."""
        b = self.span(i)[1]
        return self.buf[b:b + k].tobytes()

    def before(self, i: int, k: int = 16) -> bytes:
        """The bytes a kernel that started reading ahead of text i would see (the previous text, the poison in front
        of offsets[0], the tail of the previous row)."""
        a = self.span(i)[0]
        return self.buf[max(0, a - k):a].tobytes()

    def check(self):
        for i, t in enumerate(self.texts):
            a, b = self.span(i)
            assert self.buf[a:b].tobytes() == t, (self.name, i)

    def device(self, device="cuda"):
        import torch
        import mojo_regex_amd as M
        d = torch.from_numpy(self.buf.copy()).to(device)
        if self.csr:
            if self.known:
                return M.DeviceBatch.from_texts(self.texts, device=device)
            return M.DeviceBatch(d, torch.from_numpy(self.offsets.copy()).to(device))
        if self.lens is not None:
            return M.DeviceBatch.strided(d, self.stride, lens=torch.from_numpy(self.lens.copy()).to(device))
        return M.DeviceBatch.strided(d, self.stride, length=self.length)


Poison = Callable[[int, bytes, int], bytes]   # (text index, text, size) -> bytes


def csr_packed(texts: Sequence[bytes]) -> Layout:
    offsets = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=offsets[1:])
    buf = np.frombuffer(b"".join(texts), dtype=np.uint8).copy()
    return Layout("csr_packed", buf, list(texts), offsets=offsets, known=True)


def csr_shifted(texts: Sequence[bytes], shift: int, pz: Poison) -> Layout:
    """CSR inside a larger buffer: `shift` poison bytes before offsets[0], 160 after offsets[n]."""
    head = pz(-1, b"", shift)
    tail = pz(len(texts), texts[-1] if texts else b"", 160)
    body = b"".join(texts)
    offsets = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=offsets[1:])
    offsets += shift
    buf = np.frombuffer(head + body + tail, dtype=np.uint8).copy()
    return Layout("csr_shift%d" % shift, buf, list(texts), offsets=offsets)


def whole_rows(texts: Sequence[bytes], stride: int, pz: Poison) -> Layout:
    """Fixed pitch, length == stride: row i is the text `texts[i]` cut or continued with poison to `stride` bytes; the
    next row is the only outside (and the last row has none)."""
    rows = [(t + pz(i, t, stride))[:stride] for i, t in enumerate(texts)]
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    return Layout("rows%d" % stride, buf, rows, stride=stride, length=stride)


def fixed_length(texts: Sequence[bytes], stride: int, length: int, pz: Poison) -> Layout:
    """Fixed pitch, one common length < stride: text i = texts[i] cut or continued to `length`, then a poisoned tail."""
    cut = [(t + pz(i, t, length))[:length] for i, t in enumerate(texts)]
    rows = [c + pz(i, c, stride - length) for i, c in enumerate(cut)]
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    return Layout("fixed%d_len%d" % (stride, length), buf, cut, stride=stride, length=length)


def ragged_rows(texts: Sequence[bytes], aligned: bool, pz: Poison) -> Layout:
    """Fixed pitch with per-text lens: every row has a poisoned tail of at least 16 bytes; the pitch is a multiple of
    16 or (aligned=False) 7 more than one."""
    longest = max((len(t) for t in texts), default=0)
    stride = (longest + 16 + 15) // 16 * 16 + (0 if aligned else 7)
    rows = [t + pz(i, t, stride - len(t)) for i, t in enumerate(texts)]
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    lens = np.array([len(t) for t in texts], dtype=np.int32)
    return Layout("lens%d" % stride, buf, list(texts), stride=stride, lens=lens)


def pattern_poison(pat: bytes, seed: int = 0) -> Poison:
    rng = np.random.default_rng((zlib.crc32(pat) ^ 0x5EED) + seed)
    return lambda i, t, k: poison(pat, t, k, rng)


def layouts_for(texts: Sequence[bytes], pz: Poison, row_texts: Optional[Sequence[bytes]] = None) -> List[Layout]:
    """Every layout of the module: the three with `texts` themselves (CSR packed, CSR shifted by 1 / 7 / 15, fixed
    pitch with lens at an aligned and an unaligned pitch), and the fixed-length ones, whose texts are `row_texts`
    (default: `texts`) cut or continued to the row."""
    row_texts = list(texts if row_texts is None else row_texts)
    out = [csr_packed(texts)] + [csr_shifted(texts, s, pz) for s in CSR_SHIFTS]
    out += [ragged_rows(texts, True, pz), ragged_rows(texts, False, pz)]
    out += [whole_rows(row_texts, s, pz) for s in WHOLE_ROW_STRIDES]
    out += [fixed_length(row_texts, s, k, pz) for s, k in FIXED_LENGTH]
    for lay in out:
        lay.check()
    return out


def split_ranges(spans, length: int, maxsplit: int) -> List[Tuple[int, int]]:
    """The byte ranges of regex.split (matcher.mojo:1357-1393) from findall's spans: piece q runs from the end of
    match q-1 to the start of match q -- empty, not reversed, where the two overlap (an exact literal's findall
    returns overlapping occurrences)."""
    out, prev, done = [], 0, 0
    for s, e in spans:
        if maxsplit != 0 and done >= maxsplit:
            break
        out.append((prev, max(prev, s)))
        prev = e
        done += 1
    out.append((prev, length))
    return out
