"""The poison of tests/layouts.py bites: for every pattern family, the oracle's answer on a text followed by the bytes
a careless kernel would read next (the rest of its row, its CSR neighbour, the poison after offsets[n]) differs from
its answer on the text alone, for a stated share of the texts.  Without this, padding could quietly degenerate into
bytes that cannot change a result, and the GPU layout tests (test_gpu_layouts.py) would prove nothing.  No GPU."""
import pytest

import layouts as LY
from mrx_ref import hybrid as O

# minimum share of the texts with an outside whose answer the outside changes
MIN_FINDALL = 0.10        # findall / count, every pattern not anchored at its start, over all its layouts
MIN_SEARCH = 0.20         # search, the unanchored patterns pooled
MIN_SEARCH_EACH = 0.01    # ... and each of them
MIN_END_ANCHORED = 0.02   # is_match / match_first of the '$' patterns pooled
MIN_START_ANCHORED = 0.05  # findall of the '^' patterns with the bytes in FRONT of the text, pooled


def _shares(pat):
    texts = LY.make_texts(pat, 60, n_long=2)
    lays = LY.layouts_for(texts, LY.pattern_poison(pat), texts[:30])
    orx = O.compile_regex(pat)
    ops = {"findall": lambda t: O.findall(pat, t), "search": lambda t: O.search(pat, t),
           "is_match": lambda t: orx.is_match(t, 0), "match_first": lambda t: O.match_first(pat, t)}
    hit = dict.fromkeys(list(ops) + ["front"], 0)
    seen = 0
    for lay in lays:
        for i, t in enumerate(lay.texts):
            out = lay.outside(i)
            if not out:
                continue
            seen += 1
            for op, f in ops.items():
                hit[op] += f(t) != f(t + out)
            hit["front"] += ops["findall"](t) != ops["findall"](lay.before(i) + t)
    return hit, seen


_CACHE = {}


def shares(pat):
    if pat not in _CACHE:
        _CACHE[pat] = _shares(pat)
    return _CACHE[pat]


def test_every_layout_keeps_its_texts_and_has_an_outside():
    pat = LY.PATTERNS[0]
    texts = LY.make_texts(pat, 40, n_long=1)
    lays = LY.layouts_for(texts, LY.pattern_poison(pat))
    names = [lay.name for lay in lays]
    assert len(set(names)) == len(names), names
    for lay in lays:
        lay.check()
        if lay.name != "csr_packed":      # packed CSR: only the last text has nothing behind it
            assert all(lay.outside(i) for i in range(len(lay.texts) - 1)), lay.name
        if lay.csr:
            assert lay.name == "csr_packed" or lay.offsets[0] > 0 and lay.offsets[-1] < len(lay.buf)
        else:
            assert len(lay.buf) == lay.stride * len(lay.texts)
    assert any(not lay.aligned for lay in lays) and any(lay.lens is not None for lay in lays)
    assert sum(len(t) >= 2048 for t in texts) == 1 and b"" in texts


@pytest.mark.parametrize("pat", [p for p in LY.PATTERNS if not p.startswith(b"^")])
def test_poison_changes_findall(pat):
    hit, seen = shares(pat)
    assert seen > 0 and hit["findall"] / seen >= MIN_FINDALL, (pat, hit, seen)


def test_poison_changes_search_of_unanchored_patterns():
    pats = [p for p in LY.PATTERNS if b"^" not in p and b"$" not in p]
    hits = seen = 0
    for p in pats:
        h, s = shares(p)
        assert h["search"] / s >= MIN_SEARCH_EACH, (p, h, s)
        hits, seen = hits + h["search"], seen + s
    assert hits / seen >= MIN_SEARCH, (hits, seen)


def test_poison_changes_is_match_and_match_of_end_anchored_patterns():
    pats = [p for p in LY.PATTERNS if p.endswith(b"$")]
    assert len(pats) >= 4
    for op in ("is_match", "match_first"):
        hits = sum(shares(p)[0][op] for p in pats)
        seen = sum(shares(p)[1] for p in pats)
        assert hits / seen >= MIN_END_ANCHORED, (op, hits, seen)


def test_poison_in_front_changes_findall_of_start_anchored_patterns():
    """A '^' pattern's answer hardly depends on what follows the text; it does on what precedes it."""
    pats = [p for p in LY.PATTERNS if p.startswith(b"^")]
    assert len(pats) >= 3
    hits = sum(shares(p)[0]["front"] for p in pats)
    seen = sum(shares(p)[1] for p in pats)
    assert hits / seen >= MIN_START_ANCHORED, (hits, seen)


def test_split_ranges_of_overlapping_matches_are_empty_not_reversed():
    t = b"a" * 25 + b" x " + b"a" * 22
    spans = O.findall(b"a" * 22, t)
    assert spans == [(0, 22), (1, 23), (2, 24), (3, 25), (28, 50)]
    r = LY.split_ranges(spans, len(t), 0)
    assert r == [(0, 0), (22, 22), (23, 23), (24, 24), (25, 28), (50, 50)]
    assert [t[a:b] for a, b in r] == O.split(b"a" * 22, t)
    assert LY.split_ranges(spans, len(t), 2) == [(0, 0), (22, 22), (23, len(t))]
    assert LY.split_ranges(spans, len(t), -1) == [(0, len(t))]
