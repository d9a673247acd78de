"""PatternSet.sub without a GPU: the expectation helper (tests/set_sub_expect.py) on hand-traced cases, the C ABI's
symbols, its argument errors and both refusals (a group reference, a refused member), all of which return before any
device call."""
import numpy as np

import mojo_regex_amd as M
import set_sub_expect as E

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C


def test_tie_at_equal_start_goes_to_the_lower_member():
    assert E.expected_sub([b"ab", b"a"], [b"<0>", b"<1>"], b"xab") == (b"x<0>", 1)
    assert E.expected_sub([b"a", b"ab"], [b"<0>", b"<1>"], b"xab") == (b"x<0>b", 1)


def test_overlap_is_dropped_without_a_search_behind_the_selected_hit():
    assert E.expected_sub([b"[a-z]+", b"foo"], [b"W", b"F"], b"xfoo") == (b"W", 1)
    # 'b\w' hits (1, 3) only; an alternation would search again at 2 and replace "bc" as well
    assert E.expected_sub([b"ab", b"b\\w"], [b"X", b"Y"], b"abbc") == (b"Xbc", 1)


def test_self_overlapping_literal_selects_the_first_occurrence_only():
    # findall of the 22-byte literal on 23 a's is (0, 22) and (1, 23)
    assert E.expected_sub([b"a" * 22], [b"<A>"], b"a" * 23) == (b"<A>a", 1)


def test_empty_matches_anchors_count_and_empty_replacements():
    assert E.expected_sub([b"z*"], [b"-"], b"ab") == (b"-a-b-", 3)
    assert E.expected_sub([b"z*"], [b"-"], b"") == (b"-", 1)
    assert E.expected_sub([b"\\d+$", b"^[a-z]+"], [b"D", b"L"], b"ab 12") == (b"L D", 2)
    assert E.expected_sub([b"\\d"], [b"X"], b"1234", count=3) == (b"XXX4", 3)
    assert E.expected_sub([b"\\d"], [b"X"], b"1234", count=1) == (b"X234", 1)
    assert E.expected_sub([b"\\d+", b"[a-z]+"], [b"", b"w"], b"ab12cd") == (b"ww", 3)
    assert E.expected_sub([b"\\d+", b"[a-z]+"], [b"N", b"w"], b"") == (b"", 0)
    off, data, nsub = E.expected_arrays([b"z*"], [b"-"], [b"ab", b"", b"q"])
    assert off.tolist() == [0, 5, 6, 9] and data.tobytes() == b"-a-b--" + b"-q-" and nsub.tolist() == [3, 1, 2]


SYMBOLS = ("mrx_set_sub_dev", "mrx_set_sub_known_dev", "mrx_set_sub_strided_dev", "mrx_set_sub_batch")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None


def _table(reps):
    arr = (C.c_char_p * len(reps))(*reps)
    lens = (C.c_size_t * len(reps))(*[len(r) for r in reps])
    return arr, lens


def test_argument_errors():
    s = M.compile_set([b"[a-z]+\\d+", b"foo"])
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    arr, lens = _table([b"X", b"Y"])
    tot = C.c_int64(-7)
    bt = C.byref(tot)
    # negative n, count, out_cap
    assert lib.mrx_set_sub_dev(s._h, arr, lens, 0, FAKE, FAKE, -1, FAKE, FAKE, 16, None, bt, None) == A
    assert lib.mrx_set_sub_dev(s._h, arr, lens, -1, FAKE, FAKE, 10, FAKE, FAKE, 16, None, bt, None) == A
    assert lib.mrx_set_sub_dev(s._h, arr, lens, 0, FAKE, FAKE, 10, FAKE, FAKE, -1, None, bt, None) == A
    assert lib.mrx_set_sub_strided_dev(s._h, arr, lens, 0, FAKE, 64, None, 64, -1, FAKE, FAKE, 16, None, bt, None) == A
    # null required pointers
    assert lib.mrx_set_sub_dev(s._h, arr, lens, 0, FAKE, None, 10, FAKE, FAKE, 16, None, bt, None) == A
    assert lib.mrx_set_sub_dev(s._h, arr, lens, 0, FAKE, FAKE, 10, None, FAKE, 16, None, bt, None) == A
    assert lib.mrx_set_sub_dev(s._h, arr, lens, 0, FAKE, FAKE, 10, FAKE, None, 16, None, bt, None) == A
    assert lib.mrx_set_sub_dev(s._h, arr, None, 0, FAKE, FAKE, 10, FAKE, FAKE, 16, None, bt, None) == A
    assert lib.mrx_set_sub_dev(None, arr, lens, 0, FAKE, FAKE, 10, FAKE, FAKE, 16, None, bt, None) == A
    # a NULL entry of nonzero length; a NULL table with a nonzero length
    arr2, lens2 = _table([b"X", b"Y"])
    arr2[1] = None
    assert lib.mrx_set_sub_dev(s._h, arr2, lens2, 0, FAKE, FAKE, 10, FAKE, FAKE, 16, None, bt, None) == A
    assert lib.mrx_set_sub_dev(s._h, None, lens, 0, FAKE, FAKE, 10, FAKE, FAKE, 16, None, bt, None) == A
    # negative known bounds, a length beyond the pitch, a non-positive pitch
    assert lib.mrx_set_sub_known_dev(s._h, arr, lens, 0, FAKE, FAKE, 10, -1, 10, FAKE, FAKE, 16, None, bt, None) == A
    assert lib.mrx_set_sub_strided_dev(s._h, arr, lens, 0, FAKE, 64, None, 65, 10, FAKE, FAKE, 16, None, bt, None) == A
    assert lib.mrx_set_sub_strided_dev(s._h, arr, lens, 0, FAKE, 0, None, 0, 10, FAKE, FAKE, 16, None, bt, None) == A
    assert lib.mrx_set_sub_batch(s._h, arr, lens, 0, None, None, 1, None, None, 16, None, bt) == A
    data, off = M.pack_texts([b"abc1", b"zz9"])
    out_off = np.full(3, -5, np.int64)
    assert lib.mrx_set_sub_batch(s._h, arr, lens, -1, data.ctypes.data, off.ctypes.data, 2, out_off.ctypes.data,
                                 FAKE, 16, None, bt) == A
    assert lib.mrx_set_sub_batch(s._h, arr2, lens2, 0, data.ctypes.data, off.ctypes.data, 2, out_off.ctypes.data,
                                 FAKE, 16, None, bt) == A
    assert tot.value == -7 and out_off.tolist() == [-5, -5, -5]   # nothing was written


def test_group_reference_is_refused_before_anything_is_enqueued():
    s = M.compile_set([b"[a-z]+\\d+", b"foo"])
    lib = M.load_library()
    arr, lens = _table([b"ok \\0", b"<\\1>"])
    tot = C.c_int64(-7)
    for rc in (lib.mrx_set_sub_dev(s._h, arr, lens, 0, FAKE, FAKE, 10, FAKE, FAKE, 16, None, C.byref(tot), None),
               lib.mrx_set_sub_known_dev(s._h, arr, lens, 0, FAKE, FAKE, 10, 100, 10, FAKE, FAKE, 16, None,
                                         C.byref(tot), None),
               lib.mrx_set_sub_strided_dev(s._h, arr, lens, 0, FAKE, 64, None, 64, 10, FAKE, FAKE, 16, None,
                                           C.byref(tot), None)):
        assert rc == M.api.MRX_E_UNSUPPORTED, rc
        assert lib.mrx_last_error() == b"member 1: group references are not supported in a set's sub"
    assert tot.value == -7
    data, off = M.pack_texts([b"abc1", b"zz9"])
    out_off = np.full(3, -5, np.int64)
    rc = lib.mrx_set_sub_batch(s._h, arr, lens, 0, data.ctypes.data, off.ctypes.data, 2, out_off.ctypes.data, FAKE, 16,
                               None, None)
    assert rc == M.api.MRX_E_UNSUPPORTED and lib.mrx_last_error().startswith(b"member 1: group references")
    assert out_off.tolist() == [-5, -5, -5]
    import pytest
    with pytest.raises(M.UnsupportedPattern, match="^member 1: group references"):
        s.sub([b"x", b"<\\2>"], [b"abc1"])
    with pytest.raises(M.MrxError):
        s.sub([b"x"], [b"abc1"])   # one replacement for a set of two


def test_member_refusal_is_reported_before_anything_is_enqueued():
    s = M.compile_set([b"[a-z]+\\d+", b"(a|b)*a(a|b){5}$"])
    lib = M.load_library()
    arr, lens = _table([b"X", b"Y"])
    tot = C.c_int64(-7)
    for rc in (lib.mrx_set_sub_dev(s._h, arr, lens, 0, FAKE, FAKE, 10, FAKE, FAKE, 16, None, C.byref(tot), None),
               lib.mrx_set_sub_known_dev(s._h, arr, lens, 0, FAKE, FAKE, 10, 100, 10, FAKE, FAKE, 16, None,
                                         C.byref(tot), None),
               lib.mrx_set_sub_strided_dev(s._h, arr, lens, 0, FAKE, 64, None, 64, 10, FAKE, FAKE, 16, None,
                                           C.byref(tot), None)):
        assert rc == M.api.MRX_E_UNSUPPORTED, rc
        assert lib.mrx_last_error().startswith(b"member 1: "), lib.mrx_last_error()
    assert tot.value == -7
    data, off = M.pack_texts([b"abc1", b"zz9"])
    out_off = np.full(3, -5, np.int64)
    rc = lib.mrx_set_sub_batch(s._h, arr, lens, 0, data.ctypes.data, off.ctypes.data, 2, out_off.ctypes.data, FAKE, 16,
                               None, None)
    assert rc == M.api.MRX_E_UNSUPPORTED and lib.mrx_last_error().startswith(b"member 1: ")
    assert out_off.tolist() == [-5, -5, -5]
