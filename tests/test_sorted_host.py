"""The sorted index without a GPU: the expectation helper (tests/sorted_expect.py) on hand-traced cases, the C ABI's
symbols and its argument errors, all of which return before any device call."""
import numpy as np

import mojo_regex_amd as M
import sorted_expect as SX

FAKE = 1 << 40   # a device pointer, or a handle, that is never dereferenced
C = M.api.C


def test_order_is_bytewise_unsigned_and_prefix_first():
    entries = [b"aa", b"a\0", b"", b"a"]
    assert SX.order(entries).tolist() == [2, 3, 1, 0]                     # b"" < b"a" < b"a\0" < b"aa"
    lo, hi = SX.search(entries, [b"", b"a", b"a\0", b"aa", b"a\0\0", b"ab", b"\0"], SX.EQUAL)
    assert lo.tolist() == [0, 1, 2, 3, 3, 4, 1] and hi.tolist() == [1, 2, 3, 4, 3, 4, 1]
    high = [b"\x80", b"\x7f", b"\x7f\xff"]                                # 0x80 above 0x7f
    assert SX.order(high).tolist() == [1, 2, 0]
    lo, hi = SX.search(high, [b"\x7f", b"\x80", b"\x7f\x80", b"\xff"], SX.EQUAL)
    assert lo.tolist() == [0, 2, 1, 3] and hi.tolist() == [1, 3, 1, 3]


def test_duplicates_stand_in_index_order():
    entries = [b"b", b"a", b"b", b"a", b"b"]
    assert SX.order(entries).tolist() == [1, 3, 0, 2, 4]
    lo, hi = SX.search(entries, [b"a", b"b", b"ab", b"c"], SX.EQUAL)
    assert lo.tolist() == [0, 2, 2, 5] and hi.tolist() == [2, 5, 2, 5]
    assert SX.index(entries, [b"a", b"b", b"ab"]) == [1, 0, -1]
    lo, hi = SX.search(entries, [b"b", b"bb", b""], SX.LONGEST)
    assert lo.tolist() == [2, 2, -1] and hi.tolist() == [1, 1, -1]       # the lowest position of the equal entries


def test_prefix_ranges_and_longest_prefix():
    entries = [b"/img/", b"/", b"/img/png/", b"/api", b"/img/", b"zzz"]
    srt = sorted(entries)
    assert srt == [b"/", b"/api", b"/img/", b"/img/", b"/img/png/", b"zzz"]
    lo, hi = SX.search(entries, [b"/img", b"/img/", b"/img/p", b"/x", b"", b"zzzz", b"/"], SX.PREFIX)
    assert lo.tolist() == [2, 2, 4, 5, 0, 6, 0] and hi.tolist() == [5, 5, 5, 5, 6, 6, 5]
    lo, hi = SX.search(entries, [b"/img/png/a.png", b"/img/jpg", b"/api", b"/ap", b"img", b"zzzz", b""], SX.LONGEST)
    assert lo.tolist() == [4, 2, 1, 0, -1, 5, -1] and hi.tolist() == [9, 5, 4, 1, -1, 3, -1]
    with_empty = entries + [b""]                                          # the empty entry is a prefix of every text
    lo, hi = SX.search(with_empty, [b"img", b"", b"/q"], SX.LONGEST)
    assert lo.tolist() == [0, 0, 1] and hi.tolist() == [0, 0, 1]


def test_empty_index_and_empty_probe():
    for mode, want in ((SX.EQUAL, (0, 0)), (SX.PREFIX, (0, 0)), (SX.LONGEST, (-1, -1))):
        lo, hi = SX.search([], [b"", b"abc"], mode)
        assert lo.tolist() == [want[0]] * 2 and hi.tolist() == [want[1]] * 2 and lo.dtype == np.int64
    assert SX.order([]).tolist() == [] and SX.order([]).dtype == np.int64
    entries = [b"b", b"", b"a", b""]
    lo, hi = SX.search(entries, [b""], SX.EQUAL)
    assert (lo.tolist(), hi.tolist()) == ([0], [2])
    lo, hi = SX.search(entries, [b""], SX.PREFIX)                         # every entry begins with the empty text
    assert (lo.tolist(), hi.tolist()) == ([0], [4])
    lo, hi = SX.search([b"b", b"a"], [b""], SX.PREFIX)
    assert (lo.tolist(), hi.tolist()) == ([0], [2])
    lo, hi = SX.search(entries, [], SX.EQUAL)
    assert lo.size == 0 and hi.size == 0


SYMBOLS = ("mrx_sorted_build_dev", "mrx_sorted_build_strided_dev", "mrx_sorted_free", "mrx_sorted_size",
           "mrx_sorted_distinct", "mrx_sorted_order_dev", "mrx_sorted_search_dev", "mrx_sorted_search_strided_dev",
           "mrx_sorted_search_batch")
HOOKS = ("mrx_debug_sorted_grid", "mrx_debug_sorted_aids")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    for name in HOOKS:
        assert name in M.api.TESTING_SYMBOLS
        assert getattr(lib, name) is not None
    assert callable(M.SortedIndex) and callable(M.build_sorted_index) and callable(M.searchsorted)
    for name in ("searchsorted", "equal_range", "prefix_range", "longest_prefix", "index", "search_async"):
        assert callable(getattr(M.SortedIndex, name))
    assert (M.api.MRX_SORTED_EQUAL, M.api.MRX_SORTED_PREFIX, M.api.MRX_SORTED_LONGEST) == (SX.EQUAL, SX.PREFIX, SX.LONGEST)
    lib.mrx_sorted_free(None)                                             # NULL is a no-op
    assert lib.mrx_sorted_size(None) == 0 and lib.mrx_sorted_distinct(None) == 0


def test_aid_switch_keeps_its_mask():
    lib = M.load_library()
    default = lib.mrx_debug_sorted_aids(-1)
    try:
        assert lib.mrx_debug_sorted_aids(0) == 0
        assert lib.mrx_debug_sorted_aids(1) == 1 and lib.mrx_debug_sorted_aids(3) == 3
        assert lib.mrx_debug_sorted_aids(-5) == 3                         # any other negative value changes nothing
    finally:
        assert lib.mrx_debug_sorted_aids(-1) == default


def test_build_argument_errors_leave_out_alone():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    out = C.c_void_p(12345)
    ref = C.byref(out)
    assert lib.mrx_sorted_build_dev(FAKE, FAKE, -1, None, ref) == A                     # negative m
    assert lib.mrx_sorted_build_dev(FAKE, None, 10, None, ref) == A                     # null d_offsets
    assert lib.mrx_sorted_build_dev(FAKE, FAKE, 10, None, None) == A                    # null out
    assert lib.mrx_sorted_build_dev(FAKE, FAKE, 1 << 31, None, ref) == A                # an index needs 32 bits
    assert b"2^31" in lib.mrx_last_error()
    assert lib.mrx_sorted_build_strided_dev(FAKE, 64, None, 64, -1, None, ref) == A
    assert lib.mrx_sorted_build_strided_dev(FAKE, 64, None, 64, 10, None, None) == A
    assert lib.mrx_sorted_build_strided_dev(FAKE, 64, None, 65, 10, None, ref) == A     # a length beyond the pitch
    assert lib.mrx_sorted_build_strided_dev(FAKE, 64, None, -1, 10, None, ref) == A
    assert lib.mrx_sorted_build_strided_dev(FAKE, 0, None, 0, 10, None, ref) == A       # a non-positive pitch
    assert lib.mrx_sorted_build_strided_dev(FAKE, -8, None, 0, 10, None, ref) == A
    assert lib.mrx_sorted_build_strided_dev(FAKE, 64, None, 64, (1 << 31) + 3, None, ref) == A
    assert out.value == 12345
    assert lib.mrx_debug_scratch_in_use() == 0


def test_search_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    calls = (lambda h, mode, n, *t: lib.mrx_sorted_search_dev(h, mode, FAKE, FAKE, n, *t, None),
             lambda h, mode, n, *t: lib.mrx_sorted_search_strided_dev(h, mode, FAKE, 64, None, 64, n, *t, None))
    for call in calls:
        assert call(None, SX.EQUAL, 10, FAKE, FAKE) == A                  # null handle
        assert call(FAKE, 3, 10, FAKE, FAKE) == A                         # an unknown mode
        assert call(FAKE, 0xFFFFFFFF, 10, FAKE, FAKE) == A
        for mode in (SX.EQUAL, SX.PREFIX, SX.LONGEST):
            assert call(FAKE, mode, -1, FAKE, FAKE) == A                  # negative n
            assert call(FAKE, mode, 10, None, None) == A                  # both outputs null
    assert lib.mrx_sorted_search_dev(FAKE, SX.EQUAL, FAKE, None, 10, FAKE, FAKE, None) == A          # null d_offsets
    assert lib.mrx_sorted_search_strided_dev(FAKE, SX.EQUAL, FAKE, 64, None, 65, 10, FAKE, FAKE, None) == A
    assert lib.mrx_sorted_search_strided_dev(FAKE, SX.EQUAL, FAKE, 0, None, 0, 10, FAKE, FAKE, None) == A
    assert lib.mrx_sorted_search_strided_dev(FAKE, SX.EQUAL, FAKE, -8, None, 0, 10, FAKE, FAKE, None) == A
    assert lib.mrx_sorted_order_dev(None, FAKE, None) == A                # null handle
    assert lib.mrx_debug_scratch_in_use() == 0


def test_host_entry_point_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    edata, eoff = M.pack_texts([b"b", b"a"])
    data, off = M.pack_texts([b"abc1", b"zz9"])
    lo, hi = np.full(2, -5, np.int64), np.full(2, -5, np.int64)
    bad = np.array([4, 2, 0], np.int64)
    e, eo, d, o, pl, ph = edata.ctypes.data, eoff.ctypes.data, data.ctypes.data, off.ctypes.data, lo.ctypes.data, hi.ctypes.data
    search = lib.mrx_sorted_search_batch
    assert search(e, eo, -1, SX.EQUAL, d, o, 2, pl, ph) == A
    assert search(e, eo, 2, SX.EQUAL, d, o, -1, pl, ph) == A
    assert search(e, eo, 2, 7, d, o, 2, pl, ph) == A                      # an unknown mode
    assert search(e, None, 2, SX.EQUAL, d, o, 2, pl, ph) == A
    assert search(e, eo, 2, SX.EQUAL, d, None, 2, pl, ph) == A
    assert search(e, eo, 2, SX.EQUAL, d, o, 2, None, None) == A
    assert search(None, eo, 2, SX.EQUAL, d, o, 2, pl, ph) == A            # null data of a batch with bytes
    assert search(e, eo, 2, SX.EQUAL, None, o, 2, pl, ph) == A
    assert search(e, eo, 1 << 31, SX.EQUAL, d, o, 2, pl, ph) == A         # refused before the offsets are read
    assert b"2^31" in lib.mrx_last_error()
    assert search(e, bad.ctypes.data, 2, SX.EQUAL, d, o, 2, pl, ph) == A  # offsets that decrease
    assert search(e, eo, 2, SX.EQUAL, d, bad.ctypes.data, 2, pl, ph) == A
    assert lo.tolist() == [-5, -5] and hi.tolist() == [-5, -5]
