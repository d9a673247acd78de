"""tests/chain_cases.py alone, through its expectations and without a GPU: the base corpus makes every producer and
every consumer do something, the degenerate corpora give the empty shapes, and the two lists name every public method
that takes a batch."""
import inspect

import numpy as np
import pytest

import chain_cases as CC
import mojo_regex_amd as M


def _affordable(c, texts):
    return [t for t in texts if not c.limit or len(t) <= c.limit]


def test_the_base_corpus_has_the_shapes_the_issue_names():
    lens = sorted(len(t) for t in CC.BASE)
    assert 140 <= len(CC.BASE) <= 160 and lens[0] == 0 and CC.BASE.count(b"") >= 3
    assert [5000 <= k <= 20480 for k in lens[-4:]] == [True] * 4 and lens[-5] <= 300
    assert lens[-1] > 16384 and lens[-4] > 4096
    assert max(len(t) for t in CC.SHORT) <= 300 and len(CC.SHORT) == len(CC.BASE) - 4
    blob = b"".join(CC.BASE)
    for needle in (b"\n", b" ", b",", b"7", b"A", b"a", b"\r\n") + tuple(CC.KW):
        assert needle in blob, needle


@pytest.mark.parametrize("p", CC.PRODUCERS, ids=lambda p: p.name)
def test_producer_expectation_on_the_base_corpus(p):
    out = p.expect(CC.BASE)
    assert len(out) > 0 and any(out), p.name
    assert out != list(CC.BASE), p.name
    assert any(len(t) == 0 for t in out) == p.can_empty, p.name


def test_degenerate_corpora_give_no_texts_and_empty_texts():
    none, empties = set(), set()
    for p in CC.PRODUCERS:
        assert p.expect([]) == [], p.name
        for name, texts in CC.DEGENERATE.items():
            out = p.expect(texts)
            if texts and not out:
                none.add(p.name)
            if out and not any(out):
                empties.add(p.name)
    assert {"filter", "set_filter", "kw_filter", "extract", "expand", "lines", "from_lines"} <= none, none
    assert {"dict_filter", "sort", "take", "distinct", "lower", "strip", "sub_dev", "kw_sub"} <= empties, empties
    for p in CC.PRODUCERS:   # on "nothing" a filter keeps nothing and a finder finds nothing
        if p.name in ("filter", "set_filter", "kw_filter", "dict_filter", "extract", "extract_group", "expand"):
            assert p.expect(CC.DEGENERATE["nothing"]) == [], p.name


@pytest.mark.parametrize("c", CC.CONSUMERS, ids=lambda c: c.name)
def test_consumer_expectation_on_the_base_corpus(c):
    texts = _affordable(c, CC.BASE)
    exp = c.expect(texts)
    hit = np.asarray(c.hit(exp, texts))
    assert hit.any() and not hit.all(), c.name
    exp0 = c.expect([])   # the shapes of a batch without texts come out of the same code
    assert len(exp0) == len(exp)


def _public(cls):
    return {"%s.%s" % (cls.__name__, name) for name, v in inspect.getmembers(cls)
            if not name.startswith("_") and callable(v)}


def test_the_lists_name_every_batch_taking_public_method():
    public = set()
    for cls in (M.DeviceBatch, M.CompiledRegex, M.PatternSet, M.Dictionary, M.Keywords):
        public |= _public(cls)
    covered = {m for case in CC.PRODUCERS + CC.CONSUMERS for m in case.covers}
    assert covered <= public, sorted(covered - public)
    assert not covered & set(CC.NOT_COVERED), sorted(covered & set(CC.NOT_COVERED))
    assert set(CC.NOT_COVERED) <= public, sorted(set(CC.NOT_COVERED) - public)
    missing = public - covered - set(CC.NOT_COVERED)
    assert not missing, "no producer or consumer runs %s" % sorted(missing)
    assert all(CC.NOT_COVERED.values())


def test_names_are_unique():
    for cases in (CC.PRODUCERS, CC.CONSUMERS):
        names = [c.name for c in cases]
        assert len(names) == len(set(names))
