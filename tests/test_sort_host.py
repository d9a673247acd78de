"""sort and take without a GPU: the expectation helper (tests/sort_expect.py) on hand-traced cases, the C ABI's symbols
and its argument errors, all of which return before any device call."""
from collections import Counter

import numpy as np

import mojo_regex_amd as M
import sort_expect as S

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C


def test_order_is_bytewise_unsigned_prefix_first_and_stable():
    texts = [b"b", b"", b"a\0", b"a", b"\x80", b"a", b"\x7f"]
    order, rank, u = S.expected(texts)
    assert order.tolist() == [1, 3, 5, 2, 0, 6, 4]
    assert rank.tolist() == [3, 0, 2, 1, 5, 1, 4] and u == 6
    assert [texts[i] for i in order] == sorted(texts)
    assert S.order([b"", b"a", b"a\0", b"a\0\0", b"aa"]).tolist() == [0, 1, 2, 3, 4]
    assert S.order([b"aa", b"a\0\0", b"a\0", b"a", b""]).tolist() == [4, 3, 2, 1, 0]


def test_rank_is_numpy_unique_inverse():
    rng = np.random.default_rng(7)
    texts = [bytes(rng.integers(97, 100, size=int(rng.integers(0, 4))).tolist()) for _ in range(300)]
    order, rank, u = S.expected(texts)
    uniq, inverse = np.unique(np.array(texts, dtype=object), return_inverse=True)
    assert u == len(uniq) and np.array_equal(rank, inverse)
    assert sorted(order.tolist()) == list(range(300))
    assert all(texts[a] < texts[b] or (texts[a] == texts[b] and a < b) for a, b in zip(order[:-1], order[1:]))


def test_no_text_and_one_text():
    order, rank, u = S.expected([])
    assert order.tolist() == [] and rank.tolist() == [] and u == 0 and order.dtype == np.int64
    assert [a.tolist() for a in S.expected([b"x"])[:2]] == [[0], [0]]
    off, data = S.packed([])
    assert off.tolist() == [0] and data.size == 0


def test_take_and_count_order():
    texts = [b"b", b"", b"ab", b"b"]
    assert S.take(texts, [3, 0, 0, 2, 1]) == [b"b", b"b", b"b", b"ab", b""]
    off, data = S.packed(S.take(texts, [2, 2, 1, 0]))
    assert off.tolist() == [0, 2, 4, 4, 5] and data.tobytes() == b"ababb"
    pieces = [b"x", b"b", b"a", b"b", b"a", b"c", b"b"]
    assert S.value_counts(pieces) == [(b"x", 1), (b"b", 3), (b"a", 2), (b"c", 1)]
    assert S.value_counts(pieces, "value") == [(b"a", 2), (b"b", 3), (b"c", 1), (b"x", 1)]
    assert S.value_counts(pieces, "count") == [(b"b", 3), (b"a", 2), (b"x", 1), (b"c", 1)] == Counter(pieces).most_common()
    assert S.value_counts(pieces, "count", top=2) == Counter(pieces).most_common(2)
    assert S.value_counts(pieces, "value", top=0) == [] and len(S.value_counts(pieces, None, top=10 ** 9)) == 4


SYMBOLS = ("mrx_sort_dev", "mrx_sort_known_dev", "mrx_sort_strided_dev", "mrx_sort_batch",
           "mrx_take_dev", "mrx_take_known_dev", "mrx_take_strided_dev", "mrx_take_batch")
HOOKS = ("mrx_debug_sort_small", "mrx_debug_sort_grid", "mrx_debug_sort_rounds")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    for name in HOOKS:
        assert name in M.api.TESTING_SYMBOLS
        assert getattr(lib, name) is not None
    assert callable(M.sort_texts) and callable(M.distinct) and callable(M.value_counts)
    for name in ("argsort", "take", "take_async", "sort"):
        assert callable(getattr(M.DeviceBatch, name))


def _tot():
    tot = (C.c_int64 * 2)(-7, -7)
    return tot, C.cast(tot, C.c_void_p)


def test_sort_device_entry_points_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    calls = (lambda n, *t: lib.mrx_sort_dev(FAKE, FAKE, n, *t, None),
             lambda n, *t: lib.mrx_sort_known_dev(FAKE, FAKE, n, 100, 10, *t, None),
             lambda n, *t: lib.mrx_sort_strided_dev(FAKE, 64, None, 64, n, *t, None))
    for call in calls:
        assert call(-1, FAKE, FAKE, FAKE) == A                       # negative n
        assert call(10, None, FAKE, FAKE) == A                       # null d_order
        assert call(10, None, None, None) == A
        assert call(1 << 31, FAKE, FAKE, FAKE) == A                  # an index needs 32 bits
        assert b"2^31" in lib.mrx_last_error()
        assert call((1 << 31) + 5, FAKE, None, None) == A
    assert lib.mrx_sort_dev(FAKE, None, 10, FAKE, FAKE, FAKE, None) == A                    # null d_offsets
    assert lib.mrx_sort_known_dev(FAKE, None, 10, 100, 10, FAKE, FAKE, FAKE, None) == A
    assert lib.mrx_sort_known_dev(FAKE, FAKE, 10, -1, 10, FAKE, FAKE, FAKE, None) == A      # negative known bounds
    assert lib.mrx_sort_known_dev(FAKE, FAKE, 10, 100, -1, FAKE, FAKE, FAKE, None) == A
    assert lib.mrx_sort_strided_dev(FAKE, 64, None, 65, 10, FAKE, FAKE, FAKE, None) == A    # a length beyond the pitch
    assert lib.mrx_sort_strided_dev(FAKE, 64, None, -1, 10, FAKE, FAKE, FAKE, None) == A
    assert lib.mrx_sort_strided_dev(FAKE, 0, None, 0, 10, FAKE, FAKE, FAKE, None) == A      # a non-positive pitch
    assert lib.mrx_sort_strided_dev(FAKE, -8, None, 0, 10, FAKE, FAKE, FAKE, None) == A
    assert lib.mrx_debug_scratch_in_use() == 0


def test_take_device_entry_points_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    tot, tp = _tot()
    calls = (lambda n, *t: lib.mrx_take_dev(FAKE, FAKE, n, *t, None),
             lambda n, *t: lib.mrx_take_known_dev(FAKE, FAKE, n, 100, 10, *t, None),
             lambda n, *t: lib.mrx_take_strided_dev(FAKE, 64, None, 64, n, *t, None))
    # (d_index, k, d_out_offsets, d_out_data, out_cap, d_totals, totals)
    for call in calls:
        assert call(-1, FAKE, 5, FAKE, FAKE, 16, FAKE, tp) == A      # negative n
        assert call(10, FAKE, -1, FAKE, FAKE, 16, FAKE, tp) == A     # negative k
        assert call(10, FAKE, 5, FAKE, FAKE, -1, FAKE, tp) == A      # negative out_cap
        assert call(10, None, 5, FAKE, FAKE, 16, FAKE, tp) == A      # null d_index
        assert call(10, FAKE, 5, None, FAKE, 16, FAKE, tp) == A      # null d_out_offsets
        assert call(10, FAKE, 5, FAKE, None, 16, FAKE, tp) == A      # null d_out_data with a capacity
        assert call(10, FAKE, 5, FAKE, FAKE, 16, None, tp) == A      # null d_totals
        assert call(10, None, 0, None, FAKE, 16, FAKE, tp) == A      # ... for no index too
        assert call(10, None, 0, FAKE, FAKE, 16, None, tp) == A
    good = (FAKE, 5, FAKE, FAKE, 16, FAKE, tp)
    assert lib.mrx_take_dev(FAKE, None, 10, *good, None) == A                          # null d_offsets
    assert lib.mrx_take_known_dev(FAKE, None, 10, 100, 10, *good, None) == A
    assert lib.mrx_take_known_dev(FAKE, FAKE, 10, -1, 10, *good, None) == A            # negative known bounds
    assert lib.mrx_take_known_dev(FAKE, FAKE, 10, 100, -1, *good, None) == A
    assert lib.mrx_take_strided_dev(FAKE, 64, None, 65, 10, *good, None) == A          # a length beyond the pitch
    assert lib.mrx_take_strided_dev(FAKE, 0, None, 0, 10, *good, None) == A            # a non-positive pitch
    assert list(tot) == [-7, -7]
    assert lib.mrx_debug_scratch_in_use() == 0


def test_host_entry_points_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    tot, tp = _tot()
    data, off = M.pack_texts([b"abc1", b"zz9"])
    order, rank = np.full(2, -5, np.int64), np.full(2, -5, np.int64)
    d, o = data.ctypes.data, off.ctypes.data
    bad = np.array([4, 2, 0], np.int64)
    sort = lib.mrx_sort_batch
    assert sort(d, o, -1, order.ctypes.data, rank.ctypes.data, tp) == A
    assert sort(d, None, 2, order.ctypes.data, rank.ctypes.data, tp) == A
    assert sort(d, o, 2, None, rank.ctypes.data, tp) == A
    assert sort(None, o, 2, order.ctypes.data, rank.ctypes.data, tp) == A              # null data of a batch with bytes
    assert sort(d, o, 1 << 31, order.ctypes.data, rank.ctypes.data, tp) == A           # refused before the offsets are read
    assert b"2^31" in lib.mrx_last_error()
    assert sort(d, bad.ctypes.data, 2, order.ctypes.data, rank.ctypes.data, tp) == A   # offsets that decrease
    index = np.array([1, 0, 1], np.int64)
    out_off = np.full(4, -5, np.int64)
    out = np.full(16, 0xEE, np.uint8)
    take = lib.mrx_take_batch
    i, oo, od = index.ctypes.data, out_off.ctypes.data, out.ctypes.data
    assert take(d, o, -1, i, 3, oo, od, 16, tp) == A
    assert take(d, o, 2, i, -1, oo, od, 16, tp) == A
    assert take(d, o, 2, i, 3, oo, od, -1, tp) == A
    assert take(d, None, 2, i, 3, oo, od, 16, tp) == A
    assert take(d, o, 2, None, 3, oo, od, 16, tp) == A
    assert take(d, o, 2, i, 3, None, od, 16, tp) == A
    assert take(d, o, 2, i, 3, oo, None, 16, tp) == A
    assert take(None, o, 2, i, 3, oo, od, 16, tp) == A
    assert take(d, bad.ctypes.data, 2, i, 3, oo, od, 16, tp) == A
    assert list(tot) == [-7, -7]
    assert order.tolist() == [-5, -5] and rank.tolist() == [-5, -5] and out_off.tolist() == [-5] * 4
    assert out.tolist() == [0xEE] * 16
