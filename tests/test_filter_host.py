"""filter without a GPU: the expectation helper (tests/filter_expect.py) on hand-traced cases, the C ABI's symbols,
its argument errors and its refusals, all of which return before any device call."""
import numpy as np
import pytest

import mojo_regex_amd as M
import filter_expect as E

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C
INV, ALL = M.api.MRX_FILTER_INVERT, M.api.MRX_FILTER_ALL
REFUSED = b"(a|b)*a(a|b){5}$"   # its search is refused (tests/test_set_sub_host.py)


def _triple(got):
    return got[0].tolist(), got[1].tolist(), got[2].tobytes()


def test_plain_and_inverted():
    texts = [b"a1", b"bb", b"", b"22"]
    assert _triple(E.expected([b"\\d+"], texts)) == ([0, 3], [0, 2, 4], b"a122")
    assert _triple(E.expected([b"\\d+"], texts, invert=True)) == ([1, 2], [0, 2, 2], b"bb")
    assert E.expected_lists([b"\\d+"], texts)[0] == [b"a1", b"22"]


def test_set_any_all_none():
    pats, texts = [b"foo", b"\\d+"], [b"foo1", b"foo", b"7", b"zz", b""]
    assert _triple(E.expected(pats, texts, "any")) == ([0, 1, 2], [0, 4, 7, 8], b"foo1foo7")
    assert _triple(E.expected(pats, texts, "all")) == ([0], [0, 4], b"foo1")
    assert _triple(E.expected(pats, texts, "any", invert=True)) == ([3, 4], [0, 2, 2], b"zz")
    assert _triple(E.expected(pats, texts, "all", invert=True)) == ([1, 2, 3, 4], [0, 3, 4, 6, 6], b"foo7zz")


def test_no_member_any_is_false_all_is_true():
    texts = [b"a", b"", b"bc"]
    assert _triple(E.expected([], texts, "any")) == ([], [0], b"")
    assert _triple(E.expected([], texts, "all")) == ([0, 1, 2], [0, 1, 1, 3], b"abc")
    assert _triple(E.expected([], texts, "any", invert=True)) == ([0, 1, 2], [0, 1, 1, 3], b"abc")


def test_empty_texts_are_kept_by_an_empty_match_and_repeat_their_offset():
    assert _triple(E.expected([b"x*"], [b"", b"ab", b""])) == ([0, 1, 2], [0, 0, 2, 2], b"ab")
    assert _triple(E.expected([b"x*"], [])) == ([], [0], b"")


def test_both_anchors():
    texts = [b"abc", b"abcd", b"xabc", b"", b"abc"]
    assert _triple(E.expected([b"^abc$"], texts)) == ([0, 4], [0, 3, 6], b"abcabc")
    assert _triple(E.expected([b"^abc$"], texts, invert=True)) == ([1, 2, 3], [0, 4, 8, 8], b"abcdxabc")


SYMBOLS = ("mrx_filter_dev", "mrx_filter_known_dev", "mrx_filter_strided_dev", "mrx_filter_batch",
           "mrx_set_filter_dev", "mrx_set_filter_known_dev", "mrx_set_filter_strided_dev", "mrx_set_filter_batch")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert callable(M.filter_texts) and callable(M.CompiledRegex.filter) and callable(M.CompiledRegex.filter_async)
    assert callable(M.PatternSet.filter)


def _entry_points(lib, single: bool):
    """(csr, known, strided) callables taking (handle, flags, n, kept_idx, out_offsets, out_data, out_cap, d_totals,
    totals) with a well-formed fake batch in between."""
    stem = "mrx_filter" if single else "mrx_set_filter"
    dev, known, strided = (getattr(lib, stem + s) for s in ("_dev", "_known_dev", "_strided_dev"))
    return (lambda h, f, n, *t: dev(h, f, FAKE, FAKE, n, *t, None),
            lambda h, f, n, *t: known(h, f, FAKE, FAKE, n, 100, 10, *t, None),
            lambda h, f, n, *t: strided(h, f, FAKE, 64, None, 64, n, *t, None))


@pytest.mark.parametrize("single", [True, False])
def test_argument_errors(single):
    lib = M.load_library()
    obj = M.compile_regex(b"[a-z]+\\d+") if single else M.compile_set([b"[a-z]+\\d+", b"foo"])
    h = obj._h
    A = M.api.MRX_E_ARGUMENT
    tot = (C.c_int64 * 2)(-7, -7)
    tp = C.cast(tot, C.c_void_p)
    good = (FAKE, FAKE, FAKE, 16, FAKE, tp)   # kept_idx, out_offsets, out_data, out_cap, d_totals, totals
    for call in _entry_points(lib, single):
        assert call(h, 0, -1, *good) == A                                  # negative n
        assert call(h, 0, 10, FAKE, FAKE, FAKE, -1, FAKE, tp) == A         # negative out_cap
        assert call(h, 4, 10, *good) == A                                  # unknown flag bits
        assert call(h, 0x80000001, 10, *good) == A
        assert call(None, 0, 10, *good) == A                               # null handle
        assert call(h, 0, 10, None, FAKE, FAKE, 16, FAKE, tp) == A         # null d_kept_idx (n > 0)
        assert call(h, 0, 10, FAKE, None, FAKE, 16, FAKE, tp) == A         # null d_out_offsets
        assert call(h, 0, 10, FAKE, FAKE, None, 16, FAKE, tp) == A         # null d_out_data with a capacity
        assert call(h, 0, 10, FAKE, FAKE, FAKE, 16, None, tp) == A         # null d_totals
    stem = "mrx_filter" if single else "mrx_set_filter"
    dev, known, strided, batch = (getattr(lib, stem + s) for s in ("_dev", "_known_dev", "_strided_dev", "_batch"))
    assert dev(h, 0, FAKE, None, 10, *good, None) == A                     # null d_offsets
    assert known(h, 0, FAKE, None, 10, 100, 10, *good, None) == A
    assert known(h, 0, FAKE, FAKE, 10, -1, 10, *good, None) == A           # negative known bounds
    assert known(h, 0, FAKE, FAKE, 10, 100, -1, *good, None) == A
    assert strided(h, 0, FAKE, 64, None, 65, 10, *good, None) == A         # a length beyond the pitch
    assert strided(h, 0, FAKE, 0, None, 0, 10, *good, None) == A           # a non-positive pitch
    # host buffers
    data, off = M.pack_texts([b"abc1", b"zz9"])
    idx = np.full(2, -5, np.int64)
    out_off = np.full(3, -5, np.int64)
    out = np.full(8, 0xEE, np.uint8)
    args = (idx.ctypes.data, out_off.ctypes.data, out.ctypes.data)
    assert batch(h, 0, data.ctypes.data, off.ctypes.data, -1, *args, 8, tp) == A
    assert batch(h, 0, data.ctypes.data, off.ctypes.data, 2, *args, -1, tp) == A
    assert batch(h, 8, data.ctypes.data, off.ctypes.data, 2, *args, 8, tp) == A
    assert batch(h, 0, data.ctypes.data, None, 2, *args, 8, tp) == A
    assert batch(h, 0, data.ctypes.data, off.ctypes.data, 2, None, out_off.ctypes.data, out.ctypes.data, 8, tp) == A
    assert batch(h, 0, data.ctypes.data, off.ctypes.data, 2, idx.ctypes.data, None, out.ctypes.data, 8, tp) == A
    assert batch(h, 0, data.ctypes.data, off.ctypes.data, 2, idx.ctypes.data, out_off.ctypes.data, None, 8, tp) == A
    assert batch(None, 0, data.ctypes.data, off.ctypes.data, 2, *args, 8, tp) == A
    # nothing was written
    assert list(tot) == [-7, -7] and idx.tolist() == [-5, -5] and out_off.tolist() == [-5, -5, -5]
    assert out.tolist() == [0xEE] * 8


def test_refused_search_is_refused_by_filter_with_the_same_code_and_message():
    lib = M.load_library()
    rx = M.compile_regex(REFUSED)
    U = M.api.MRX_E_UNSUPPORTED
    assert lib.mrx_search_dev(rx._h, FAKE, FAKE, 10, FAKE, FAKE, None) == U
    why = lib.mrx_last_error()
    assert why
    tot = (C.c_int64 * 2)(-7, -7)
    tp = C.cast(tot, C.c_void_p)
    good = (FAKE, FAKE, FAKE, 16, FAKE, tp)
    for call in _entry_points(lib, True):
        for flags in (0, INV):
            assert call(rx._h, flags, 10, *good) == U
            assert lib.mrx_last_error() == why
    data, off = M.pack_texts([b"abc1", b"zz9"])
    idx = np.full(2, -5, np.int64)
    out_off = np.full(3, -5, np.int64)
    assert lib.mrx_filter_batch(rx._h, 0, data.ctypes.data, off.ctypes.data, 2, idx.ctypes.data, out_off.ctypes.data,
                                FAKE, 8, tp) == U
    assert lib.mrx_last_error() == why
    assert list(tot) == [-7, -7] and idx.tolist() == [-5, -5] and out_off.tolist() == [-5, -5, -5]
    with pytest.raises(M.UnsupportedPattern) as ei:
        rx.filter([b"abc1"])
    assert str(ei.value) == why.decode()
    with pytest.raises(M.UnsupportedPattern):
        M.filter_texts(REFUSED, [b"abc1"], invert=True)


def test_refused_member_is_reported_before_anything_is_enqueued():
    lib = M.load_library()
    s = M.compile_set([b"[a-z]+\\d+", REFUSED])
    U = M.api.MRX_E_UNSUPPORTED
    assert lib.mrx_set_matches_dev(s._h, FAKE, FAKE, 10, FAKE, None) == U
    why = lib.mrx_last_error()
    assert why.startswith(b"member 1: ")
    tot = (C.c_int64 * 2)(-7, -7)
    good = (FAKE, FAKE, FAKE, 16, FAKE, C.cast(tot, C.c_void_p))
    for call in _entry_points(lib, False):
        for flags in (0, ALL, INV | ALL):
            assert call(s._h, flags, 10, *good) == U
            assert lib.mrx_last_error() == why
    assert list(tot) == [-7, -7]
    with pytest.raises(M.UnsupportedPattern, match="^member 1: "):
        s.filter([b"abc1"], mode="all")
    with pytest.raises(M.MrxError):
        s.filter([b"abc1"], mode="some")
