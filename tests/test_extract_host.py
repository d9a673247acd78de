"""extract without a GPU: the expectation helper (tests/extract_expect.py) on hand-traced cases, the C ABI's symbols, its
argument errors and its refusals, all of which return before any device call.

The oracle reports overlapping occurrences for exact literals of 21 bytes and more only (`aa` on "aaaa" is (0, 2),
(2, 4)), so the overlapping case is traced twice: on the helper with the spans written out, and through the oracle
with a literal of 21 bytes."""
import numpy as np
import pytest

import mojo_regex_amd as M
import extract_expect as X

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C
REFUSED = b"(a|b)*a(a|b){5}$"   # its search is refused (tests/test_set_sub_host.py)


def _quad(got):
    return got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3].tobytes()


def test_empty_matches_give_empty_pieces():
    assert _quad(X.expected_findall(b"z*", [b"ab"])) == ([0, 3], [0, 0, 0], [0, 0, 0, 0], b"")
    assert X.lists(X.expected_findall(b"z*", [b"ab"])) == [[b"", b"", b""]]


def test_overlapping_spans_are_each_copied_in_full():
    got = X.pack([[(0, 2), (1, 3), (2, 4)]], [b"aaaa"])
    assert _quad(got) == ([0, 3], [0, 0, 0], [0, 2, 4, 6], b"aaaaaa")   # 6 bytes from a 4-byte text
    lit = b"a" * 21
    got = X.expected_findall(lit, [b"a" * 23, b"b"])
    assert _quad(got) == ([0, 3, 3], [0, 0, 0], [0, 21, 42, 63], b"a" * 63)


def test_fixed_width_group_behind_its_text_is_cut():
    # the raw row of 'x(\d)?' on "x" is group 1 = (1, 2), whole match (0, 1)
    assert _quad(X.expected_group(b"x(\\d)?", [b"x"], 1)) == ([0, 1], [0], [0, 0], b"")
    assert _quad(X.expected_group(b"x(\\d)?", [b"x"], 0)) == ([0, 1], [0], [0, 1], b"x")
    assert _quad(X.expected_group(b"x(\\d)?", [b"x5x", b""], 1)) == ([0, 2, 2], [0, 0], [0, 1, 1], b"5")


def test_group_without_an_entry_is_an_empty_piece():
    texts = [b"ab12", b"", b"7"]
    assert _quad(X.expected_group(b"(\\d+)|([a-z]+)", texts, 1)) == ([0, 2, 2, 3], [0, 0, 2], [0, 0, 2, 3], b"127")
    assert _quad(X.expected_group(b"(\\d+)|([a-z]+)", texts, 2)) == ([0, 2, 2, 3], [0, 0, 2], [0, 2, 2, 2], b"ab")
    assert X.lists(X.expected_group(b"(\\d+)|([a-z]+)", texts, 0, count=1)) == [[b"ab"], [], [b"7"]]


def test_clamp_and_split():
    assert X.clamp(-1, -1, 5) == (0, 0) and X.clamp(3, 2, 5) == (3, 3) and X.clamp(4, 9, 5) == (4, 5)
    assert X.clamp(7, 9, 5) == (5, 5) and X.clamp(-3, 2, 5) == (0, 2)
    assert X.lists(X.expected_split(b",", [b"a,,b", b"", b","])) == [[b"a", b"", b"b"], [b""], [b"", b""]]
    assert X.lists(X.expected_split(b",", [b"a,b,c"], 1)) == [[b"a", b"b,c"]]
    assert X.lists(X.expected_split(b",", [b"a,b,c"], -1)) == [[b"a,b,c"]]


SYMBOLS = ("mrx_gather_spans_dev", "mrx_gather_spans_strided_dev", "mrx_gather_spans_batch", "mrx_extract_dev",
           "mrx_extract_known_dev", "mrx_extract_strided_dev", "mrx_extract_batch")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "mrx_debug_extract_grid" in M.api.TESTING_SYMBOLS and lib.mrx_debug_extract_grid is not None
    assert callable(M.findall_texts) and callable(M.DeviceBatch.gather_spans)
    for name in ("extract", "extract_async", "split_batch"):
        assert callable(getattr(M.CompiledRegex, name))
    assert callable(M.PatternSet.extract)


def _tot():
    tot = (C.c_int64 * 2)(-7, -7)
    return tot, C.cast(tot, C.c_void_p)


def test_gather_spans_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    tot, tp = _tot()
    forms = (lambda n, *t: lib.mrx_gather_spans_dev(FAKE, FAKE, n, *t, None),
             lambda n, *t: lib.mrx_gather_spans_strided_dev(FAKE, 64, None, 64, n, *t, None))
    # prefix, spans, row_pairs, pair, piece_cap, owner, out_offsets, out_data, out_cap, d_totals, totals
    for call in forms:
        assert call(-1, FAKE, FAKE, 1, 0, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A      # negative n
        assert call(10, FAKE, FAKE, 1, 0, -1, FAKE, FAKE, FAKE, 16, FAKE, tp) == A     # negative piece_cap
        assert call(10, FAKE, FAKE, 1, 0, 8, FAKE, FAKE, FAKE, -1, FAKE, tp) == A      # negative out_cap
        assert call(10, FAKE, FAKE, 0, 0, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A      # row_pairs < 1
        assert call(10, FAKE, FAKE, 3, 3, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A      # pair out of range
        assert call(10, FAKE, FAKE, 3, -1, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A
        assert call(10, FAKE, FAKE + 4, 1, 0, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A  # misaligned d_spans
        assert call(10, None, FAKE, 1, 0, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A      # null d_prefix
        assert call(10, FAKE, None, 1, 0, 8, FAKE, FAKE, FAKE, 16, FAKE, tp) == A      # null d_spans with a capacity
        assert call(10, FAKE, FAKE, 1, 0, 8, None, FAKE, FAKE, 16, FAKE, tp) == A      # null d_owner with a capacity
        assert call(10, FAKE, FAKE, 1, 0, 8, FAKE, None, FAKE, 16, FAKE, tp) == A      # null d_out_offsets
        assert call(10, FAKE, FAKE, 1, 0, 8, FAKE, FAKE, None, 16, FAKE, tp) == A      # null d_out_data with a capacity
        assert call(10, FAKE, FAKE, 1, 0, 8, FAKE, FAKE, FAKE, 16, None, tp) == A      # null d_totals
    good = (FAKE, FAKE, 1, 0, 8, FAKE, FAKE, FAKE, 16, FAKE, tp)
    assert lib.mrx_gather_spans_dev(FAKE, None, 10, *good, None) == A                  # null d_offsets
    assert lib.mrx_gather_spans_strided_dev(FAKE, 64, None, 65, 10, *good, None) == A  # a length beyond the pitch
    assert lib.mrx_gather_spans_strided_dev(FAKE, 0, None, 0, 10, *good, None) == A    # a non-positive pitch
    # host buffers
    data, off = M.pack_texts([b"abc1", b"zz9"])
    prefix = np.array([0, 1, 2], np.int64)
    spans = np.array([[0, 3], [2, 3]], np.int32)
    owner = np.full(2, -5, np.int64)
    out_off = np.full(3, -5, np.int64)
    out = np.full(8, 0xEE, np.uint8)
    batch = lib.mrx_gather_spans_batch
    d, o, p, s = data.ctypes.data, off.ctypes.data, prefix.ctypes.data, spans.ctypes.data
    outs = (owner.ctypes.data, out_off.ctypes.data, out.ctypes.data)
    assert batch(d, o, -1, p, s, 1, 0, 2, *outs, 8, tp) == A
    assert batch(d, o, 2, p, s, 1, 0, -1, *outs, 8, tp) == A
    assert batch(d, o, 2, p, s, 1, 0, 2, *outs, -1, tp) == A
    assert batch(d, o, 2, p, s, 0, 0, 2, *outs, 8, tp) == A
    assert batch(d, o, 2, p, s, 1, 1, 2, *outs, 8, tp) == A
    assert batch(d, None, 2, p, s, 1, 0, 2, *outs, 8, tp) == A
    assert batch(d, o, 2, None, s, 1, 0, 2, *outs, 8, tp) == A
    assert batch(d, o, 2, p, None, 1, 0, 2, *outs, 8, tp) == A
    assert batch(d, o, 2, p, s, 1, 0, 2, None, out_off.ctypes.data, out.ctypes.data, 8, tp) == A
    assert batch(d, o, 2, p, s, 1, 0, 2, owner.ctypes.data, None, out.ctypes.data, 8, tp) == A
    assert batch(d, o, 2, p, s, 1, 0, 2, owner.ctypes.data, out_off.ctypes.data, None, 8, tp) == A
    # nothing was written
    assert list(tot) == [-7, -7] and owner.tolist() == [-5, -5] and out_off.tolist() == [-5, -5, -5]
    assert out.tolist() == [0xEE] * 8


def _extract_entry_points(lib):
    """(csr, known, strided) callables taking (handle, n, piece_prefix, owner, out_offsets, piece_cap, out_data,
    out_cap, d_totals, totals) with a well-formed fake batch in between."""
    return (lambda h, n, *t: lib.mrx_extract_dev(h, FAKE, FAKE, n, *t, None),
            lambda h, n, *t: lib.mrx_extract_known_dev(h, FAKE, FAKE, n, 100, 10, *t, None),
            lambda h, n, *t: lib.mrx_extract_strided_dev(h, FAKE, 64, None, 64, n, *t, None))


def test_extract_argument_errors():
    lib = M.load_library()
    h = M.compile_regex(b"[a-z]+\\d+")._h
    A = M.api.MRX_E_ARGUMENT
    tot, tp = _tot()
    good = (FAKE, FAKE, FAKE, 8, FAKE, 16, FAKE, tp)
    for call in _extract_entry_points(lib):
        assert call(h, -1, *good) == A                                          # negative n
        assert call(h, 10, FAKE, FAKE, FAKE, -1, FAKE, 16, FAKE, tp) == A       # negative piece_cap
        assert call(h, 10, FAKE, FAKE, FAKE, 8, FAKE, -1, FAKE, tp) == A        # negative out_cap
        assert call(None, 10, *good) == A                                       # null handle
        assert call(h, 10, None, FAKE, FAKE, 8, FAKE, 16, FAKE, tp) == A        # null d_piece_prefix
        assert call(h, 10, FAKE, None, FAKE, 8, FAKE, 16, FAKE, tp) == A        # null d_owner with a capacity
        assert call(h, 10, FAKE, FAKE, None, 8, FAKE, 16, FAKE, tp) == A        # null d_out_offsets
        assert call(h, 10, FAKE, FAKE, FAKE, 8, None, 16, FAKE, tp) == A        # null d_out_data with a capacity
        assert call(h, 10, FAKE, FAKE, FAKE, 8, FAKE, 16, None, tp) == A        # null d_totals
    assert lib.mrx_extract_dev(h, FAKE, None, 10, *good, None) == A             # null d_offsets
    assert lib.mrx_extract_known_dev(h, FAKE, None, 10, 100, 10, *good, None) == A
    assert lib.mrx_extract_known_dev(h, FAKE, FAKE, 10, -1, 10, *good, None) == A   # negative known bounds
    assert lib.mrx_extract_known_dev(h, FAKE, FAKE, 10, 100, -1, *good, None) == A
    assert lib.mrx_extract_strided_dev(h, FAKE, 64, None, 65, 10, *good, None) == A
    assert lib.mrx_extract_strided_dev(h, FAKE, 0, None, 0, 10, *good, None) == A
    data, off = M.pack_texts([b"abc1", b"zz9"])
    prefix = np.full(3, -5, np.int64)
    owner = np.full(2, -5, np.int64)
    out_off = np.full(3, -5, np.int64)
    out = np.full(8, 0xEE, np.uint8)
    batch = lib.mrx_extract_batch
    d, o = data.ctypes.data, off.ctypes.data
    p, w, oo, od = prefix.ctypes.data, owner.ctypes.data, out_off.ctypes.data, out.ctypes.data
    assert batch(None, d, o, 2, p, w, oo, 2, od, 8, tp) == A
    assert batch(h, d, o, -1, p, w, oo, 2, od, 8, tp) == A
    assert batch(h, d, o, 2, p, w, oo, -1, od, 8, tp) == A
    assert batch(h, d, o, 2, p, w, oo, 2, od, -1, tp) == A
    assert batch(h, d, None, 2, p, w, oo, 2, od, 8, tp) == A
    assert batch(h, d, o, 2, None, w, oo, 2, od, 8, tp) == A
    assert batch(h, d, o, 2, p, None, oo, 2, od, 8, tp) == A
    assert batch(h, d, o, 2, p, w, None, 2, od, 8, tp) == A
    assert batch(h, d, o, 2, p, w, oo, 2, None, 8, tp) == A
    assert list(tot) == [-7, -7] and prefix.tolist() == [-5] * 3 and owner.tolist() == [-5, -5]
    assert out_off.tolist() == [-5, -5, -5] and out.tolist() == [0xEE] * 8


def test_refused_findall_is_refused_by_extract_with_the_same_code_and_message():
    lib = M.load_library()
    rx = M.compile_regex(REFUSED)
    U = M.api.MRX_E_UNSUPPORTED
    assert lib.mrx_findall_dev(rx._h, FAKE, FAKE, 10, FAKE, FAKE, 8, None, None) == U
    why = lib.mrx_last_error()
    assert why
    tot, tp = _tot()
    for call in _extract_entry_points(lib):
        assert call(rx._h, 10, FAKE, FAKE, FAKE, 8, FAKE, 16, FAKE, tp) == U
        assert lib.mrx_last_error() == why
    data, off = M.pack_texts([b"abc1", b"zz9"])
    prefix = np.full(3, -5, np.int64)
    assert lib.mrx_extract_batch(rx._h, data.ctypes.data, off.ctypes.data, 2, prefix.ctypes.data, FAKE, FAKE, 2, FAKE, 8,
                                 tp) == U
    assert lib.mrx_last_error() == why
    assert list(tot) == [-7, -7] and prefix.tolist() == [-5] * 3
