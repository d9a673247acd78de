"""expand's expected answers, from the oracle only: one record per row of captures_all
(`captures_all_expect.expected_rows`), the template (`mrx_ref.hybrid._parse_repl_template`, the one template grammar)
with each reference replaced by the row's group clamped to its text (`extract_expect.clamp`), packed as
`extract_expect.pack` packs pieces (the contract is in include/mrx.h, mrx_expand_spans_dev).

Host-only: imports the oracle and numpy, neither torch nor the product library.  expected() raises
O.ReferenceDoesNotTerminate where the reference's loop would not end; corpus() keeps only pairs on which it never does.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

import captures_all_expect as CA
import extract_expect as X
import layouts as LY
from mrx_ref import hybrid as O

Pair = Tuple[int, int]
Row = Sequence[Pair]


def record(template: bytes, row: Row, text: bytes) -> bytes:
    """The record of one row (g + 1 pairs: groups 1..g, then the whole match) of `text`."""
    g = len(row) - 1
    out = []
    for gref, s, ln in O._parse_repl_template(template):
        if gref > 0:
            if gref <= g:
                a, b = X.clamp(row[gref - 1][0], row[gref - 1][1], len(text))
                out.append(text[a:b])
        else:
            out.append(template[s:s + ln])
    return b"".join(out)


def from_rows(template: bytes, rows: Sequence[Sequence[Row]], texts: Sequence[bytes]) -> X.Packed:
    """rows[i]: the rows of text i, in order.  (prefix int64[n + 1], owner int64[records], out_offsets
    int64[records + 1], out_data uint8[bytes]): X.pack's packing, of records instead of pieces."""
    assert len(rows) == len(texts)
    recs = [[record(template, r, t) for r in rs] for rs, t in zip(rows, texts)]
    # every record as a text of its own with the one pair that covers it: pack() then lays them out
    flat = [r for rs in recs for r in rs]
    _, _, off, data = X.pack([[(0, len(r))] for r in flat], flat)
    prefix = np.zeros(len(texts) + 1, dtype=np.int64)
    if texts:
        np.cumsum([len(rs) for rs in recs], out=prefix[1:])
    owner = np.repeat(np.arange(len(texts), dtype=np.int64), np.diff(prefix))
    return prefix, owner, off, data


_rows = {}   # (pattern, count, text) -> rows: computed once, shared by every test that needs them, never changed


def rows_of(pat: bytes, texts: Sequence[bytes], count: int = 0) -> List[List[List[Pair]]]:
    g = CA.num_groups(pat)
    out = []
    for t in texts:
        key = (pat, count, t)
        if key not in _rows:
            _rows[key] = CA.expected_rows(pat, t, count, g)
        out.append(_rows[key])
    return out


def expected(pat: bytes, template: bytes, texts: Sequence[bytes], count: int = 0) -> X.Packed:
    """CompiledRegex.expand(template, texts, count)."""
    return from_rows(template, rows_of(pat, texts, count), texts)


def all_groups_template(g: int) -> bytes:
    """A template that names every group of a g-group pattern, with literals between them."""
    return b"<" + b"|".join(b"\\%d" % j for j in range(1, g + 1)) + b">"


def candidates() -> List[Tuple[bytes, bytes]]:
    """The (pattern, template) pairs of captures_all's three corpora; a fixed pattern takes \\2-\\1 and one template that
    names every group."""
    out = list(CA.GROUP_PATTERNS) + list(CA.CHAIN_SUBS)
    for pat in CA.FIXED_PATTERNS:
        out += [(pat, b"\\2-\\1"), (pat, all_groups_template(CA.num_groups(pat)))]
    return list(dict.fromkeys(out))


def corpus_texts(pat: bytes) -> List[bytes]:
    return LY.make_texts(pat, 60, n_long=2)


MIN_ROWS = 10
_corpus = None


def corpus() -> List[Tuple[bytes, bytes, List[bytes]]]:
    """(pattern, template, texts) for every candidate pair on which the oracle ends on every text and the batch has at
    least MIN_ROWS rows, so that no text is ever skipped at compare time.  Computed once."""
    global _corpus
    if _corpus is None:
        _corpus, by_pat = [], {}
        for pat, tpl in candidates():
            if pat not in by_pat:
                texts = corpus_texts(pat)
                try:
                    by_pat[pat] = (texts, sum(len(r) for r in rows_of(pat, texts)))
                except O.ReferenceDoesNotTerminate:
                    by_pat[pat] = (texts, -1)
            texts, nrows = by_pat[pat]
            if nrows >= MIN_ROWS:
                _corpus.append((pat, tpl, texts))
    return _corpus


# hand-written texts that do match, for the shapes the seeded texts leave without rows (the reference's group loop
# finds nothing for (ab)+(c), x(.*)y and (\\s+)(\\S?) on any text tried: they stay out)
HAND_TEXTS = {
    b"(\\d{4})-(\\d{2})-(\\d{2})": [b"2026-04-12 and 2025-12-25", b"on 1999-01-31", b"2024-02-29"],
    b"(\\w+)@(\\w+)\\.com": [b"mail bob@example.com or amy@corp.com now", b"x@y.com"],
    b"([a-z]+)@([a-z]+)\\.(com|org)": [b"bob@example.org, amy@corp.com", b"a@b.com"],
    b"^(\\w+)\\s+(\\w+)$": [b"hello world", b"a \t b_1"],
    b"(foo|bar|baz)=(\\d+|x)": [b"foo=12 bar=x baz=007", b"bar=x"],
    b"(?:hello) (\\w+)": [b"hello world, hello there", b"say hello you"],
    b"(cat|dog)s? (\\w+)": [b"cats sleep, dog barks", b"dog x"],
    b"(h.llo) (w.*d)": [b"hello world", b"say hallo wd"],
}
# the candidate patterns that corpus() leaves out: the hand-written ones, three without any row, and one on whose seeded
# texts the reference's loop does not end.  Written out so that a test can be parametrised without running the oracle;
# tests/test_expand_host.py asserts that this is what corpus() computes.
UNQUALIFIED = frozenset(HAND_TEXTS) | {b"(ab)+(c)", b"x(.*)y", b"(\\s+)(\\S?)", b"(a(b|c)d)+"}


def lists(packed: X.Packed) -> List[List[bytes]]:
    return X.lists(packed)


def reassemble(text: bytes, rows: Sequence[Row], records: Sequence[bytes]) -> bytes:
    """sub()'s output for `text` from the gaps between its matches (the whole-match pair of each row) and one record per
    match, with the byte the loop copies behind an empty match."""
    if not text:
        return text
    out, pos = [], 0
    for r, rec in zip(rows, records):
        ms, me = r[-1]
        if ms > pos:
            out.append(text[pos:ms])
        out.append(rec)
        if me == ms:
            if pos < len(text):
                out.append(text[pos:pos + 1])
            pos = me + 1
        else:
            pos = me
    if pos < len(text):
        out.append(text[pos:])
    return b"".join(out)
