"""expand without a GPU: the expectation helper (tests/expand_expect.py) on hand-traced cases, the identity that ties
its records to sub() on the whole corpus, the corpus condition itself, and the C ABI's symbols, argument errors and
refusals, all of which return before any device call."""
import numpy as np

import mojo_regex_amd as M
import captures_all_expect as CA
import expand_expect as E
from mrx_ref import hybrid as O

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C
REFUSED = b"(" * 17 + b"a" + b")" * 17 + b"(b)"   # captures_all refuses it (tests/test_gpu_captures_all.py)


def _recs(pat, tpl, texts, count=0):
    return E.lists(E.expected(pat, tpl, texts, count))


def test_hand_traces():
    assert _recs(b"(\\d+)-(\\d+)", b"\\2/\\1", [b"10-20 3-4"]) == [[b"20/10", b"4/3"]]
    got = E.expected(b"(\\d+)-(\\d+)", b"\\2/\\1", [b"10-20 3-4", b"", b"7-8"])
    assert got[0].tolist() == [0, 2, 2, 3] and got[1].tolist() == [0, 0, 2] and got[2].tolist() == [0, 5, 8, 11]
    assert got[3].tobytes() == b"20/104/38/7"
    # the group behind the text: the raw row of 'x(\d)?' on "x" is group 1 = (1, 2)
    assert _recs(b"x(\\d)?", b"<\\1>", [b"x"]) == [[b"<>"]]
    assert _recs(b"x(\\d)?", b"<\\1>", [b"x5x"]) == [[b"<5>", b"<>"]]
    # a group without an entry contributes nothing
    assert _recs(b"(\\d+)|([a-z]+)", b"\\1:\\2", [b"ab12"]) == [[b":ab", b"12:"]]
    # a reference above the pattern's groups contributes nothing
    assert _recs(b"(\\d+)", b"[\\9\\1\\2]", [b"a1b22"]) == [[b"[1]", b"[22]"]]
    # \0, \\ and a trailing backslash stay literal
    assert _recs(b"(\\d)", b"\\0\\\\\\1\\", [b"7"]) == [[b"\\0\\\\7\\"]]
    assert _recs(b"(\\d)", b"\\\\1", [b"7"]) == [[b"\\7"]]   # the second backslash opens the reference, as in sub
    assert O.sub(b"(\\d)", b"\\\\1", b"7") == b"\\7"
    # an empty template: empty records, offsets repeat; a template without references: the same record for every match
    got = E.expected(b"(\\d)", b"", [b"1a2", b"3"])
    assert got[0].tolist() == [0, 2, 3] and got[2].tolist() == [0, 0, 0, 0] and got[3].size == 0
    assert _recs(b"(\\d)", b"n/a", [b"1a2", b"", b"x"]) == [[b"n/a", b"n/a"], [], []]
    # an empty text has no match, count limits the matches of a text
    assert _recs(b"(\\d*)", b"<\\1>", [b""]) == [[]]
    assert _recs(b"(\\d+)-(\\d+)", b"\\2/\\1", [b"10-20 3-4 5-6", b"1-2"], count=2) == [[b"20/10", b"4/3"], [b"2/1"]]
    rows = [[[(0, 2), (3, 5), (0, 5)]], [], [[(-1, -1), (4, 9), (0, 1)]]]
    got = E.from_rows(b"\\2+\\1+\\3", rows, [b"ab cd", b"zz", b"hello"])
    assert E.lists(got) == [[b"cd+ab+"], [], [b"o++"]] and got[1].tolist() == [0, 2]


def test_corpus_condition():
    corpus = E.corpus()
    pats = {p for p, _, _ in corpus}
    assert len(corpus) >= 28 and len(pats) >= 28
    for pat in (b"(\\w+)|(\\d+)", b"(\\d+)(ab)*", b"(?:(x)|(y)|(z))+"):   # rows with a group without an entry
        assert pat in pats
        assert any(p[0] < 0 for rs in E.rows_of(pat, E.corpus_texts(pat)) for r in rs for p in r[:-1]), pat
    assert b"(a(b|c)d)+" not in pats   # the reference's loop does not end on some of its texts
    assert {p for p, _ in E.candidates()} - pats == E.UNQUALIFIED
    for pat, texts in E.HAND_TEXTS.items():
        assert pat not in pats and any(pat == p for p, _ in E.candidates()), pat
        assert all(len(rs) > 0 for rs in E.rows_of(pat, texts)), pat


def _identity(pat, tpl, texts):
    for t, rows in zip(texts, E.rows_of(pat, texts)):
        records = [E.record(tpl, r, t) for r in rows]
        assert CA.sub_from_rows(tpl, t, rows) == E.reassemble(t, rows, records), (pat, tpl, t[:60])


def test_records_are_the_bytes_sub_puts_in_place_of_each_match():
    """sub_from_rows (the oracle's slicing) = the gaps joined with expected()'s records (the clamp rule), on every row
    the product can emit -- the byte copied behind an empty match included."""
    empties = 0
    for pat, tpl, texts in E.corpus():
        _identity(pat, tpl, texts)
        empties += sum(1 for rs in E.rows_of(pat, texts[:20]) for r in rs if r[-1][0] == r[-1][1])
    assert empties > 0
    tpl_of = dict(E.candidates())
    for pat, texts in E.HAND_TEXTS.items():
        _identity(pat, tpl_of[pat], texts)
        assert O.sub(pat, tpl_of[pat], texts[0]) == CA.sub_from_rows(tpl_of[pat], texts[0], E.rows_of(pat, texts[:1])[0])


SYMBOLS = ("mrx_expand_spans_dev", "mrx_expand_spans_strided_dev", "mrx_expand_spans_batch", "mrx_expand_dev",
           "mrx_expand_strided_dev", "mrx_expand_batch")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "mrx_debug_expand_grid" in M.api.TESTING_SYMBOLS and lib.mrx_debug_expand_grid is not None
    assert callable(M.expand) and callable(M.DeviceBatch.expand_spans) and callable(M.CompiledRegex.expand)


def _tot():
    tot = (C.c_int64 * 2)(-7, -7)
    return tot, C.cast(tot, C.c_void_p)


def test_expand_spans_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    tot, tp = _tot()
    forms = (lambda n, *t: lib.mrx_expand_spans_dev(FAKE, FAKE, n, *t, None),
             lambda n, *t: lib.mrx_expand_spans_strided_dev(FAKE, 64, None, 64, n, *t, None))
    T = b"\\2/\\1"
    # prefix, rows, row_pairs, tpl, tpl_len, piece_cap, owner, out_offsets, out_data, out_cap, d_totals, totals
    for call in forms:
        assert call(-1, FAKE, FAKE, 3, T, 5, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A      # negative n
        assert call(10, FAKE, FAKE, 3, T, 5, -1, FAKE, FAKE, FAKE, 16, FAKE, tp) == A     # negative piece_cap
        assert call(10, FAKE, FAKE, 3, T, 5, 8, FAKE, FAKE, FAKE, -1, FAKE, tp) == A      # negative out_cap
        assert call(10, FAKE, FAKE, 0, T, 5, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A      # row_pairs < 1
        assert call(10, FAKE, FAKE, 3, None, 5, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A   # null tpl with a length
        assert call(10, FAKE, FAKE + 4, 3, T, 5, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A  # misaligned d_rows
        assert call(10, None, FAKE, 3, T, 5, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A      # null d_prefix
        assert call(10, FAKE, None, 3, T, 5, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A      # null d_rows with a capacity
        assert call(10, FAKE, FAKE, 3, T, 5, 8, None, FAKE, FAKE, 16, FAKE, tp) == A      # null d_owner with a capacity
        assert call(10, FAKE, FAKE, 3, T, 5, 8, FAKE, None, FAKE, 16, FAKE, tp) == A      # null d_out_offsets
        assert call(10, FAKE, FAKE, 3, T, 5, 8, FAKE, FAKE, None, 16, FAKE, tp) == A      # null d_out_data with a capacity
        assert call(10, FAKE, FAKE, 3, T, 5, 8, FAKE, FAKE, FAKE, 16, None, tp) == A      # null d_totals
    good = (FAKE, FAKE, 3, T, 5, 8, FAKE, FAKE, FAKE, 16, FAKE, tp)
    assert lib.mrx_expand_spans_dev(FAKE, None, 10, *good, None) == A                  # null d_offsets
    assert lib.mrx_expand_spans_strided_dev(FAKE, 64, None, 65, 10, *good, None) == A  # a length beyond the pitch
    assert lib.mrx_expand_spans_strided_dev(FAKE, 0, None, 0, 10, *good, None) == A    # a non-positive pitch
    # host buffers
    data, off = M.pack_texts([b"10-20", b"3-4"])
    prefix = np.array([0, 1, 2], np.int64)
    rows = np.array([[[0, 2], [3, 5], [0, 5]], [[0, 1], [2, 3], [0, 3]]], np.int32)
    owner = np.full(2, -5, np.int64)
    out_off = np.full(3, -5, np.int64)
    out = np.full(8, 0xEE, np.uint8)
    batch = lib.mrx_expand_spans_batch
    d, o, p, s = data.ctypes.data, off.ctypes.data, prefix.ctypes.data, rows.ctypes.data
    outs = (owner.ctypes.data, out_off.ctypes.data, out.ctypes.data)
    assert batch(d, o, -1, p, s, 3, T, 5, 2, *outs, 8, tp) == A
    assert batch(d, o, 2, p, s, 3, T, 5, -1, *outs, 8, tp) == A
    assert batch(d, o, 2, p, s, 3, T, 5, 2, *outs, -1, tp) == A
    assert batch(d, o, 2, p, s, 0, T, 5, 2, *outs, 8, tp) == A
    assert batch(d, o, 2, p, s, 3, None, 5, 2, *outs, 8, tp) == A
    assert batch(d, None, 2, p, s, 3, T, 5, 2, *outs, 8, tp) == A
    assert batch(d, o, 2, None, s, 3, T, 5, 2, *outs, 8, tp) == A
    assert batch(d, o, 2, p, None, 3, T, 5, 2, *outs, 8, tp) == A
    assert batch(d, o, 2, p, s, 3, T, 5, 2, None, out_off.ctypes.data, out.ctypes.data, 8, tp) == A
    assert batch(d, o, 2, p, s, 3, T, 5, 2, owner.ctypes.data, None, out.ctypes.data, 8, tp) == A
    assert batch(d, o, 2, p, s, 3, T, 5, 2, owner.ctypes.data, out_off.ctypes.data, None, 8, tp) == A
    # nothing was written
    assert list(tot) == [-7, -7] and owner.tolist() == [-5, -5] and out_off.tolist() == [-5, -5, -5]
    assert out.tolist() == [0xEE] * 8


def _expand_entry_points(lib):
    """(csr, strided) callables taking (handle, tpl, tpl_len, count, n, match_prefix, owner, out_offsets, match_cap,
    out_data, out_cap, d_totals, totals) with a well-formed fake batch in between."""
    return (lambda h, t, tl, c, n, *r: lib.mrx_expand_dev(h, t, tl, c, FAKE, FAKE, n, *r, None),
            lambda h, t, tl, c, n, *r: lib.mrx_expand_strided_dev(h, t, tl, c, FAKE, 64, None, 64, n, *r, None))


def test_expand_argument_errors():
    lib = M.load_library()
    h = M.compile_regex(b"(\\d+)-(\\d+)")._h
    A = M.api.MRX_E_ARGUMENT
    tot, tp = _tot()
    T = b"\\2/\\1"
    good = (FAKE, FAKE, FAKE, 8, FAKE, 16, FAKE, tp)
    for call in _expand_entry_points(lib):
        assert call(h, T, 5, 0, -1, *good) == A                                          # negative n
        assert call(h, T, 5, -1, 10, *good) == A                                         # negative count
        assert call(h, T, 5, 0, 10, FAKE, FAKE, FAKE, -1, FAKE, 16, FAKE, tp) == A       # negative match_cap
        assert call(h, T, 5, 0, 10, FAKE, FAKE, FAKE, 8, FAKE, -1, FAKE, tp) == A        # negative out_cap
        assert call(None, T, 5, 0, 10, *good) == A                                       # null handle
        assert call(h, None, 5, 0, 10, *good) == A                                       # null tpl with a length
        assert call(h, T, 5, 0, 10, None, FAKE, FAKE, 8, FAKE, 16, FAKE, tp) == A        # null d_match_prefix
        assert call(h, T, 5, 0, 10, FAKE, None, FAKE, 8, FAKE, 16, FAKE, tp) == A        # null d_owner with a capacity
        assert call(h, T, 5, 0, 10, FAKE, FAKE, None, 8, FAKE, 16, FAKE, tp) == A        # null d_out_offsets
        assert call(h, T, 5, 0, 10, FAKE, FAKE, FAKE, 8, None, 16, FAKE, tp) == A        # null d_out_data with a capacity
        assert call(h, T, 5, 0, 10, FAKE, FAKE, FAKE, 8, FAKE, 16, None, tp) == A        # null d_totals
    assert lib.mrx_expand_dev(h, T, 5, 0, FAKE, None, 10, *good, None) == A              # null d_offsets
    assert lib.mrx_expand_strided_dev(h, T, 5, 0, FAKE, 64, None, 65, 10, *good, None) == A
    assert lib.mrx_expand_strided_dev(h, T, 5, 0, FAKE, 0, None, 0, 10, *good, None) == A
    data, off = M.pack_texts([b"10-20", b"3-4"])
    prefix = np.full(3, -5, np.int64)
    owner = np.full(2, -5, np.int64)
    out_off = np.full(3, -5, np.int64)
    out = np.full(8, 0xEE, np.uint8)
    batch = lib.mrx_expand_batch
    d, o = data.ctypes.data, off.ctypes.data
    p, w, oo, od = prefix.ctypes.data, owner.ctypes.data, out_off.ctypes.data, out.ctypes.data
    assert batch(None, T, 5, 0, d, o, 2, p, w, oo, 2, od, 8, tp) == A
    assert batch(h, None, 5, 0, d, o, 2, p, w, oo, 2, od, 8, tp) == A
    assert batch(h, T, 5, -1, d, o, 2, p, w, oo, 2, od, 8, tp) == A
    assert batch(h, T, 5, 0, d, o, -1, p, w, oo, 2, od, 8, tp) == A
    assert batch(h, T, 5, 0, d, o, 2, p, w, oo, -1, od, 8, tp) == A
    assert batch(h, T, 5, 0, d, o, 2, p, w, oo, 2, od, -1, tp) == A
    assert batch(h, T, 5, 0, d, None, 2, p, w, oo, 2, od, 8, tp) == A
    assert batch(h, T, 5, 0, d, o, 2, None, w, oo, 2, od, 8, tp) == A
    assert batch(h, T, 5, 0, d, o, 2, p, None, oo, 2, od, 8, tp) == A
    assert batch(h, T, 5, 0, d, o, 2, p, w, None, 2, od, 8, tp) == A
    assert batch(h, T, 5, 0, d, o, 2, p, w, oo, 2, None, 8, tp) == A
    assert list(tot) == [-7, -7] and prefix.tolist() == [-5] * 3 and owner.tolist() == [-5, -5]
    assert out_off.tolist() == [-5, -5, -5] and out.tolist() == [0xEE] * 8


def test_refused_captures_all_is_refused_by_expand_with_the_same_code_and_message():
    lib = M.load_library()
    rx = M.compile_regex(REFUSED)
    U = M.api.MRX_E_UNSUPPORTED
    total = C.c_int64(-7)
    assert lib.mrx_captures_all_dev(rx._h, FAKE, FAKE, 10, 0, FAKE, FAKE, 8, C.byref(total), None) == U
    why = lib.mrx_last_error()
    assert why
    tot, tp = _tot()
    for call in _expand_entry_points(lib):
        assert call(rx._h, b"\\1", 2, 0, 10, FAKE, FAKE, FAKE, 8, FAKE, 16, FAKE, tp) == U
        assert lib.mrx_last_error() == why
    data, off = M.pack_texts([b"abc1", b"zz9"])
    prefix = np.full(3, -5, np.int64)
    assert lib.mrx_expand_batch(rx._h, b"\\1", 2, 0, data.ctypes.data, off.ctypes.data, 2, prefix.ctypes.data, FAKE, FAKE, 2,
                                FAKE, 8, tp) == U
    assert lib.mrx_last_error() == why
    assert list(tot) == [-7, -7] and prefix.tolist() == [-5] * 3
