"""distinct without a GPU: the expectation helper (tests/distinct_expect.py) on hand-traced cases, the C ABI's symbols and
its argument errors, all of which return before any device call."""
from collections import Counter

import numpy as np

import mojo_regex_amd as M
import distinct_expect as D

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C


def _five(got):
    return got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3].tolist(), got[4].tobytes()


def test_groups_are_numbered_by_first_occurrence():
    got = D.expected([b"b", b"a", b"b", b"c", b"a", b"b"])
    assert _five(got) == ([0, 1, 0, 2, 1, 0], [0, 1, 3], [3, 2, 1], [0, 1, 2, 3], b"bac")
    assert D.values(got) == [b"b", b"a", b"c"]


def test_the_empty_text_is_a_value_and_a_trailing_nul_is_a_byte():
    texts = [b"a", b"", b"a\0", b"", b"a", b"\0", b"ab"]
    got = D.expected(texts)
    assert _five(got) == ([0, 1, 2, 1, 0, 3, 4], [0, 1, 2, 5, 6], [2, 2, 1, 1, 1], [0, 1, 1, 3, 4, 6], b"aa\0\0ab")
    assert D.value_counts(texts) == list(Counter(texts).items())
    assert D.values(got) == list(dict.fromkeys(texts))


def test_no_text_and_one_text():
    assert _five(D.expected([])) == ([], [], [], [0], b"")
    assert _five(D.expected([b"xyz"])) == ([0], [0], [1], [0, 3], b"xyz")
    assert _five(D.expected([b""])) == ([0], [0], [1], [0, 0], b"")


def test_counts_add_up_and_first_increases():
    rng = np.random.default_rng(5)
    texts = [bytes(rng.integers(97, 100, size=int(rng.integers(0, 4))).tolist()) for _ in range(500)]
    group_of, first, counts, off, data = D.expected(texts)
    assert counts.sum() == len(texts) and np.all(np.diff(first) > 0) and off[-1] == len(data)
    assert [texts[i] for i in first] == D.values((group_of, first, counts, off, data))
    assert all(texts[i] == texts[first[g]] for i, g in enumerate(group_of))


SYMBOLS = ("mrx_distinct_dev", "mrx_distinct_known_dev", "mrx_distinct_strided_dev", "mrx_distinct_batch")
HOOKS = ("mrx_debug_distinct_hash_mask", "mrx_debug_distinct_grid")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    for name in HOOKS:
        assert name in M.api.TESTING_SYMBOLS
        assert getattr(lib, name) is not None
    assert callable(M.distinct) and callable(M.value_counts)
    assert callable(M.DeviceBatch.distinct) and callable(M.DeviceBatch.distinct_async)
    assert callable(M.CompiledRegex.value_counts)


def _tot():
    tot = (C.c_int64 * 2)(-7, -7)
    return tot, C.cast(tot, C.c_void_p)


def _entry_points(lib):
    """(csr, known, strided) callables taking (n, group_of, first, counts, out_offsets, out_data, out_cap, d_totals,
    totals) with a well-formed fake batch in front."""
    return (lambda n, *t: lib.mrx_distinct_dev(FAKE, FAKE, n, *t, None),
            lambda n, *t: lib.mrx_distinct_known_dev(FAKE, FAKE, n, 100, 10, *t, None),
            lambda n, *t: lib.mrx_distinct_strided_dev(FAKE, 64, None, 64, n, *t, None))


def test_device_entry_points_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    tot, tp = _tot()
    good = (FAKE, FAKE, FAKE, FAKE, FAKE, 16, FAKE, tp)
    for call in _entry_points(lib):
        assert call(-1, *good) == A                                               # negative n
        assert call(10, FAKE, FAKE, FAKE, FAKE, FAKE, -1, FAKE, tp) == A          # negative out_cap
        assert call(10, None, FAKE, FAKE, FAKE, FAKE, 16, FAKE, tp) == A          # null d_group_of
        assert call(10, FAKE, None, FAKE, FAKE, FAKE, 16, FAKE, tp) == A          # null d_first
        assert call(10, FAKE, FAKE, None, FAKE, FAKE, 16, FAKE, tp) == A          # null d_counts
        assert call(10, FAKE, FAKE, FAKE, None, FAKE, 16, FAKE, tp) == A          # null d_out_offsets
        assert call(10, FAKE, FAKE, FAKE, FAKE, None, 16, FAKE, tp) == A          # null d_out_data with a capacity
        assert call(10, FAKE, FAKE, FAKE, FAKE, FAKE, 16, None, tp) == A          # null d_totals
        assert call(0, FAKE, FAKE, FAKE, None, FAKE, 16, FAKE, tp) == A           # ... for no text too
        assert call(0, FAKE, FAKE, FAKE, FAKE, FAKE, 16, None, tp) == A
        assert call(1 << 31, *good) == A                                          # an index needs 32 bits
        assert b"2^31" in lib.mrx_last_error()
        assert call((1 << 31) + 5, *good) == A
    assert lib.mrx_distinct_dev(FAKE, None, 10, *good, None) == A                 # null d_offsets
    assert lib.mrx_distinct_known_dev(FAKE, None, 10, 100, 10, *good, None) == A
    assert lib.mrx_distinct_known_dev(FAKE, FAKE, 10, -1, 10, *good, None) == A   # negative known bounds
    assert lib.mrx_distinct_known_dev(FAKE, FAKE, 10, 100, -1, *good, None) == A
    assert lib.mrx_distinct_strided_dev(FAKE, 64, None, 65, 10, *good, None) == A  # a length beyond the pitch
    assert lib.mrx_distinct_strided_dev(FAKE, 64, None, -1, 10, *good, None) == A
    assert lib.mrx_distinct_strided_dev(FAKE, 0, None, 0, 10, *good, None) == A    # a non-positive pitch
    assert lib.mrx_distinct_strided_dev(FAKE, -8, None, 0, 10, *good, None) == A
    assert list(tot) == [-7, -7]


def test_host_entry_point_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    tot, tp = _tot()
    data, off = M.pack_texts([b"abc1", b"zz9"])
    group_of, first, counts = (np.full(2, -5, np.int64) for _ in range(3))
    out_off = np.full(3, -5, np.int64)
    out = np.full(8, 0xEE, np.uint8)
    batch = lib.mrx_distinct_batch
    d, o = data.ctypes.data, off.ctypes.data
    g, f, c, oo, od = (a.ctypes.data for a in (group_of, first, counts, out_off, out))
    assert batch(d, o, -1, g, f, c, oo, od, 8, tp) == A
    assert batch(d, o, 2, g, f, c, oo, od, -1, tp) == A
    assert batch(d, None, 2, g, f, c, oo, od, 8, tp) == A
    assert batch(d, o, 2, None, f, c, oo, od, 8, tp) == A
    assert batch(d, o, 2, g, None, c, oo, od, 8, tp) == A
    assert batch(d, o, 2, g, f, None, oo, od, 8, tp) == A
    assert batch(d, o, 2, g, f, c, None, od, 8, tp) == A
    assert batch(d, o, 2, g, f, c, oo, None, 8, tp) == A
    assert batch(None, o, 2, g, f, c, oo, od, 8, tp) == A                          # null data of a batch with bytes
    assert batch(d, o, 1 << 31, g, f, c, oo, od, 8, tp) == A                       # refused before the offsets are read
    assert b"2^31" in lib.mrx_last_error()
    bad = np.array([4, 2, 0], np.int64)
    assert batch(d, bad.ctypes.data, 2, g, f, c, oo, od, 8, tp) == A               # offsets that decrease
    assert list(tot) == [-7, -7]
    for a in (group_of, first, counts, out_off):
        assert a.tolist() == [-5] * len(a)
    assert out.tolist() == [0xEE] * 8
