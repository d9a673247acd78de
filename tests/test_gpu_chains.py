"""A batch made on the device behaves as the same texts uploaded from the host: every producer of tests/chain_cases.py,
on a batch with known bounds and on one without, on the base corpus and on the degenerate ones, feeds every consumer.

    B = P(x) on the device;  L = the texts read back from B;  L == expect_P(x)
    for every consumer C:  C(B) == expect_C(L)  and  C(B) == C(DeviceBatch.from_texts(L)) bit for bit

The reference is the host expectation; the second equality points at the producer's FORM when the two disagree: a view
into a larger buffer, a clone, loose or missing bounds, a fixed pitch with lens, the caller's own tensor, no text at all,
texts without a byte.  The last test asserts that the matrix has seen each of these."""
import numpy as np
import pytest

import chain_cases as CC
import distinct_expect as DX
import extract_expect as XX
import format_expect as FMX
import kw_sub_expect as KSX
import lines_expect as LNX
import mojo_regex_amd as M
import parse_expect as PX
import sort_expect as SX

pytestmark = pytest.mark.gpu

FORMS = ("known", "plain")
SEEN = {}        # a property of a producer's result -> the first (corpus, producer, form) that showed it
_H = []
_EXPECT = {}     # (consumer, texts) -> expectation: computed once, shared, never changed


def handles():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test on a box without a GPU")
    if not _H:
        _H.append(CC.Handles())
    return _H[0]


def to_np(out):
    """Every output of a call as numpy arrays and ints; a CSR DeviceBatch as (offsets, data)."""
    if not isinstance(out, (tuple, list)):
        out = (out,)
    flat = []
    for o in out:
        if isinstance(o, M.DeviceBatch):
            assert o.offsets is not None
            flat += [o.offsets.cpu().numpy(), o.data.cpu().numpy()]
        elif hasattr(o, "cpu"):
            flat.append(o.cpu().numpy())
        else:
            flat.append(o)
    return flat


def run(c, H, batch):
    """(outputs, None), or (None, the refusal's type)."""
    try:
        return to_np(c.device(H, batch)), None
    except (M.UnsupportedPattern, M.MrxError) as e:
        return None, type(e)


def first_text(g, w, texts):
    """The first text at which two outputs differ, for per-text arrays and CSR offsets; else the first flat index."""
    g, w = np.asarray(g), np.asarray(w)
    n = len(texts)
    if g.shape != w.shape:
        return "shapes %s and %s" % (g.shape, w.shape)
    if g.ndim >= 1 and g.shape[0] in (n, n + 1):
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        i = int(bad[0]) - (1 if g.shape[0] == n + 1 and bad[0] > 0 else 0)
        return "text %d (len %d) %r: %s, expected %s" % (i, len(texts[i]), texts[i][:80], g[bad[0]].tolist(), w[bad[0]].tolist())
    k = int(np.nonzero(g.reshape(-1) != w.reshape(-1))[0][0])
    return "flat index %d: %s, expected %s" % (k, g.reshape(-1)[k], w.reshape(-1)[k])


def expect_equal(got, want, what, texts):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, np.ndarray) or isinstance(g, np.ndarray):
            if not np.array_equal(np.asarray(g), np.asarray(w)):
                raise AssertionError("%s, output %d: %s" % (what, k, first_text(g, w, texts)))
        else:
            assert g == w, "%s, output %d: %r, expected %r" % (what, k, g, w)


def expect_same_bits(got, ref, what, texts):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for k, (g, r) in enumerate(zip(got, ref)):
        if isinstance(g, np.ndarray):
            if g.dtype != r.dtype or g.shape != r.shape or g.tobytes() != r.tobytes():
                raise AssertionError("%s, output %d differs from the run on from_texts: %s" % (what, k, first_text(g, r, texts)))
        else:
            assert g == r, "%s, output %d: %r, on from_texts %r" % (what, k, g, r)


def restrict(got, keep):
    """(prefix, rows) of the texts `keep` alone."""
    prefix, rows = got
    parts = [rows[prefix[i]:prefix[i + 1]] for i in keep]
    return [CC._prefix([len(p) for p in parts]), np.concatenate(parts) if parts else rows[:0]]


def expectation(c, texts):
    key = (c.name, tuple(texts))
    if key not in _EXPECT:
        _EXPECT[key] = list(c.expect(texts))
    return _EXPECT[key]


def produce(corpus, p, form):
    """(B, L): the producer's result on the corpus in that form, checked against its expectation and recorded."""
    H = handles()
    texts = CC.CORPORA[corpus]
    x = M.DeviceBatch.from_texts(texts)
    if form == "plain":
        x = M.DeviceBatch(x.data, x.offsets)
    B = p.device(H, texts, x)
    L = CC.texts_of(B)
    want = p.expect(texts)
    if L != want:
        i = next((i for i, (a, b) in enumerate(zip(L, want)) if a != b), min(len(L), len(want)))
        raise AssertionError("%s on %s (%s): %d texts, expected %d; first difference at text %d: %r, expected %r" % (
            p.name, corpus, form, len(L), len(want), i, L[i:i + 1], want[i:i + 1]))
    longest, nbytes = max((len(t) for t in L), default=0), sum(len(t) for t in L)
    facts = []
    if B.data.numel() > 0:
        facts.append("view" if B.data.untyped_storage().nbytes() > B.data.numel() * B.data.element_size() else "clone")
    if B.offsets is not None:
        facts.append("no_bounds" if B._max_len is None else "loose_max_len" if B._max_len > longest else "exact_max_len")
        # the bounds that a result carries forward must be true
        assert (B._max_len is None) == (B._end_offset is None), p.name
        if B._max_len is not None:
            assert B._max_len >= longest and B._end_offset >= int(B.offsets[-1].item()), (p.name, B._max_len, longest, B._end_offset)
    elif B.lens is not None:
        facts.append("strided_lens")
    if B.data is x.data:
        facts.append("callers_tensor")
    if B.n == 0:
        facts.append("no_texts")
    elif nbytes == 0:
        facts.append("texts_without_bytes")
    for f in facts:
        SEEN.setdefault(f, (corpus, p.name, form))
    return B, L


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("p", CC.PRODUCERS, ids=lambda p: p.name)
@pytest.mark.parametrize("corpus", list(CC.CORPORA))
def test_every_consumer_on_a_producers_result(corpus, p, form):
    H = handles()
    B, L = produce(corpus, p, form)
    ref = M.DeviceBatch.from_texts(L)
    for c in CC.CONSUMERS:
        what = "%s(%s) -> %s, %s corpus, %s input" % (p.name, "x", c.name, corpus, form)
        got, refused = run(c, H, B)
        got_ref, refused_ref = run(c, H, ref)
        assert refused == refused_ref, "%s: refused with %s, on from_texts with %s" % (what, refused, refused_ref)
        if refused is not None:
            continue   # (refused on the host form too: not a pass of the pair, and not a difference)
        if c.limit and any(len(t) > c.limit for t in L):
            keep = [i for i, t in enumerate(L) if len(t) <= c.limit]
            short = [L[i] for i in keep]
            expect_equal(restrict(got, keep), expectation(c, short), what, short)
        else:
            expect_equal(got, expectation(c, L), what, L)
        expect_same_bits(got, got_ref, what, L)


def _lists(batch):
    return CC.texts_of(batch)


def test_lines_fields_gather_strip_parse():
    """The CSV snippet of the README: the third blank-separated cell of every line, stripped where it lies, as a number."""
    handles()
    lines = M.DeviceBatch.from_texts(CC.BASE).lines()[0]
    prefix, rows, _ = lines.fields([3], delim=b" ")
    cells, _ = lines.gather_spans(prefix, rows)
    sp, srows = cells.strip(chars=b"\r ", spans=True)
    values, status, owner = cells.parse_spans(sp, srows, kind="int", fill=-1)
    py_lines = CC.flat(LNX.lines(t)[0] for t in CC.BASE)
    py_cells = [p[2] if len(p) >= 3 else b"" for p in (l.split(b" ") for l in py_lines)]
    assert _lists(lines) == py_lines and _lists(cells) == py_cells
    want_status, want_values = PX.expect_many([c.strip(b"\r ") for c in py_cells], "int", -1)
    assert (want_status == 0).sum() > 100 and (want_status != 0).sum() > 10
    assert np.array_equal(values.cpu().numpy(), want_values) and np.array_equal(status.cpu().numpy(), want_status)
    assert np.array_equal(owner.cpu().numpy(), np.arange(len(py_lines)))


def test_kw_sub_lower_distinct():
    H = handles()
    names, counts, _, _ = H.kw.sub(CC.KW_REPL, M.DeviceBatch.from_texts(CC.BASE)).lower().distinct()
    want = DX.value_counts([t.lower() for t in KSX.sub(CC.KW, CC.KW_REPL, CC.BASE)[0]])
    assert list(zip(_lists(names), counts.cpu().numpy().tolist())) == want
    assert 1 < len(want) < len(CC.BASE)


def test_value_counts_top_format_records():
    H = handles()
    values, counts = H.rx[CC.GROUPS].value_counts(M.DeviceBatch.from_texts(CC.BASE), group=1, sort="count", top=10)
    report = M.format_records(rb"\2 \1" + b"\n", [values, counts])
    rows = SX.value_counts(CC.flat(XX.lists(XX.expected_group(CC.GROUPS, CC.BASE, 1))), "count", 10)
    want = FMX.records(rb"\2 \1" + b"\n", [[v for v, _ in rows], ([c for _, c in rows], "d")])[0]
    assert len(rows) == 10 and rows[0][1] > rows[-1][1]
    assert _lists(report) == want and report.data.cpu().numpy().tobytes() == b"".join(want)


def test_the_matrix_saw_every_form_of_a_result():
    """Runs last: among the producers' results there was at least one of each form that a consumer could trip over."""
    handles()
    for corpus in CC.CORPORA:          # (when run on its own: the producers alone, which record the forms)
        for p in CC.PRODUCERS:
            for form in FORMS:
                produce(corpus, p, form)
    need = ("view", "clone", "loose_max_len", "no_bounds", "strided_lens", "callers_tensor", "no_texts", "texts_without_bytes")
    missing = [f for f in need if f not in SEEN]
    assert not missing, (missing, SEEN)
