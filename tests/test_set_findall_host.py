"""PatternSet.findall without a GPU: the expectation helper (tests/set_findall_expect.py) on hand-made cases, the C ABI's
symbols, its argument errors and its member refusals, all of which return before any device call."""
import numpy as np

import mojo_regex_amd as M
import set_findall_expect as E

FAKE = 1 << 40   # a device pointer that is never dereferenced


def test_member_order_then_match_order():
    got = E.expected_lists([b"b", b"a", b"[ab]"], [b"ab", b"", b"ba"])
    assert got == [[(0, 1, 2), (1, 0, 1), (2, 0, 1), (2, 1, 2)], [], [(0, 0, 1), (1, 1, 2), (2, 0, 1), (2, 1, 2)]]
    prefix, members, spans = E.expected_arrays([b"b", b"a", b"[ab]"], [b"ab", b"", b"ba"])
    assert prefix.tolist() == [0, 4, 4, 8]
    assert members.tolist() == [0, 1, 2, 2, 0, 1, 2, 2]
    assert spans.tolist() == [[1, 2], [0, 1], [0, 1], [1, 2], [0, 1], [1, 2], [0, 1], [1, 2]]


def test_self_overlapping_literal_empty_matches_dollar_and_no_match():
    # the exact-literal route of the reference returns overlapping occurrences of a long self-overlapping literal
    a22 = b"a" * 22
    got = E.expected_lists([b"aa", a22, b"z*", b"\\d+$", b"a$", b"xyz"], [b"a" * 23, b"abz", b"a1 22"])
    assert got[0] == ([(0, 0, 2), (0, 2, 4), (0, 4, 6), (0, 6, 8), (0, 8, 10), (0, 10, 12), (0, 12, 14), (0, 14, 16),
                       (0, 16, 18), (0, 18, 20), (0, 20, 22), (1, 0, 22), (1, 1, 23)]
                      + [(2, p, p) for p in range(24)] + [(4, 22, 23)])
    assert got[1] == [(2, 0, 0), (2, 1, 1), (2, 2, 3), (2, 3, 3)]
    assert got[2] == [(2, p, p) for p in range(6)] + [(3, 3, 5)]
    assert all(m != 5 for row in got for m, _, _ in row)   # 'xyz' never matches


def test_members_are_nondecreasing_within_a_text():
    pats = [b"\\d+", b"[a-z]+", b"\\w*", b"o"]
    texts = [b"foo 12 bar 345", b"", b"oo", b"99 bottles"]
    for row in E.expected_lists(pats, texts):
        ms = [m for m, _, _ in row]
        assert ms == sorted(ms)


def test_regroup_equals_the_restatement():
    pats = [b"\\d+", b"o", b"z*"]
    texts = [b"foo 12 bar 345", b"", b"oo", b"99 bottles"]
    from mrx_ref import hybrid as O
    per = []
    for p in pats:
        lists = [O.findall(p, t) for t in texts]
        prefix = np.zeros(len(texts) + 1, np.int64)
        np.cumsum([len(x) for x in lists], out=prefix[1:])
        per.append((prefix, np.array([s for x in lists for s in x], np.int32).reshape(-1, 2)))
    got = E.regroup(per, len(texts))
    want = E.expected_arrays(pats, texts)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_symbols_are_exported():
    lib = M.load_library()
    for name in ("mrx_set_findall_dev", "mrx_set_findall_known_dev", "mrx_set_findall_strided_dev",
                 "mrx_set_findall_batch"):
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None


def test_argument_errors():
    s = M.compile_set([b"[a-z]+\\d+", b"foo"])
    lib = M.load_library()
    tot = M.api.C.c_int64(-7)
    # n < 0
    assert lib.mrx_set_findall_dev(s._h, FAKE, FAKE, -1, FAKE, FAKE, FAKE, 16, M.api.C.byref(tot), None) == M.api.MRX_E_ARGUMENT
    assert lib.mrx_set_findall_strided_dev(s._h, FAKE, 64, None, 64, -1, FAKE, FAKE, FAKE, 16, None, None) == \
        M.api.MRX_E_ARGUMENT
    # null outputs with n > 0
    assert lib.mrx_set_findall_dev(s._h, FAKE, FAKE, 10, None, FAKE, FAKE, 16, None, None) == M.api.MRX_E_ARGUMENT
    assert lib.mrx_set_findall_dev(s._h, FAKE, FAKE, 10, FAKE, None, FAKE, 16, None, None) == M.api.MRX_E_ARGUMENT
    assert lib.mrx_set_findall_known_dev(s._h, FAKE, FAKE, 10, 100, 10, FAKE, FAKE, None, 16, None, None) == \
        M.api.MRX_E_ARGUMENT
    assert lib.mrx_set_findall_strided_dev(s._h, FAKE, 64, None, 64, 10, None, None, None, 16, None, None) == \
        M.api.MRX_E_ARGUMENT
    # negative span_cap, negative known bounds, null offsets, misaligned spans, a length beyond the pitch
    assert lib.mrx_set_findall_dev(s._h, FAKE, FAKE, 10, FAKE, FAKE, FAKE, -1, None, None) == M.api.MRX_E_ARGUMENT
    assert lib.mrx_set_findall_known_dev(s._h, FAKE, FAKE, 10, -1, 10, FAKE, FAKE, FAKE, 16, None, None) == \
        M.api.MRX_E_ARGUMENT
    assert lib.mrx_set_findall_dev(s._h, FAKE, None, 10, FAKE, FAKE, FAKE, 16, None, None) == M.api.MRX_E_ARGUMENT
    assert lib.mrx_set_findall_dev(s._h, FAKE, FAKE, 10, FAKE, FAKE, FAKE + 4, 16, None, None) == M.api.MRX_E_ARGUMENT
    assert lib.mrx_set_findall_strided_dev(s._h, FAKE, 64, None, 65, 10, FAKE, FAKE, FAKE, 16, None, None) == \
        M.api.MRX_E_ARGUMENT
    assert lib.mrx_set_findall_batch(s._h, None, None, 1, None, None, None, 16, None) == M.api.MRX_E_ARGUMENT
    assert tot.value == -7   # nothing was written


def test_member_refusal_is_reported_before_anything_is_enqueued():
    # member 1's search is refused (its '$' LazyDFA cache exceeds what is tracked): the call fails before it touches a
    # device, which is why this runs without one
    s = M.compile_set([b"[a-z]+\\d+", b"(a|b)*a(a|b){5}$"])
    lib = M.load_library()
    tot = M.api.C.c_int64(-7)
    for rc in (lib.mrx_set_findall_dev(s._h, FAKE, FAKE, 10, FAKE, FAKE, FAKE, 16, M.api.C.byref(tot), None),
               lib.mrx_set_findall_known_dev(s._h, FAKE, FAKE, 10, 100, 10, FAKE, FAKE, FAKE, 16, M.api.C.byref(tot), None),
               lib.mrx_set_findall_strided_dev(s._h, FAKE, 64, None, 64, 10, FAKE, FAKE, FAKE, 16, M.api.C.byref(tot),
                                               None)):
        assert rc == M.api.MRX_E_UNSUPPORTED, rc
        assert lib.mrx_last_error().startswith(b"member 1: "), lib.mrx_last_error()
    assert tot.value == -7
    data, off = M.pack_texts([b"abc1", b"zz9"])
    prefix = np.full(3, -5, np.int64)
    rc = lib.mrx_set_findall_batch(s._h, data.ctypes.data, off.ctypes.data, 2, prefix.ctypes.data, FAKE, FAKE, 16, None)
    assert rc == M.api.MRX_E_UNSUPPORTED and lib.mrx_last_error().startswith(b"member 1: ")
    assert prefix.tolist() == [-5, -5, -5]
