"""Dictionaries without a GPU: the expectation helper (tests/lookup_expect.py) on hand-traced cases, the C ABI's symbols
and its argument errors, all of which return before any device call."""
import numpy as np

import mojo_regex_amd as M
import lookup_expect as LE

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C


def _three(got):
    return got[0].tolist(), got[1].tolist(), got[2].tobytes()


def test_duplicates_among_the_entries_give_the_lowest_index():
    entries = [b"x", b"y", b"x", b"x", b"z", b"y"]
    assert LE.expected(entries, [b"x", b"z", b"y", b"w", b"x"]).tolist() == [0, 4, 1, -1, 0]
    assert _three(LE.filtered(entries, [b"x", b"z", b"y", b"w", b"x"])) == ([0, 1, 2, 4], [0, 1, 2, 3, 4], b"xzyx")
    assert _three(LE.filtered(entries, [b"x", b"z", b"y", b"w", b"x"], invert=True)) == ([3], [0, 1], b"w")


def test_the_empty_text_is_an_entry_and_a_trailing_nul_is_a_byte():
    entries = [b"a\0", b"", b"a"]
    texts = [b"a", b"a\0", b"\0", b"", b"a\0\0", b""]
    assert LE.expected(entries, texts).tolist() == [2, 0, -1, 1, -1, 1]
    assert _three(LE.filtered(entries, texts)) == ([0, 1, 3, 5], [0, 1, 3, 3, 3], b"aa\0")
    assert _three(LE.filtered(entries, texts, invert=True)) == ([2, 4], [0, 1, 4], b"\0a\0\0")
    assert LE.expected([b"\0"], texts).tolist() == [-1, -1, 0, -1, -1, -1]
    assert LE.expected([b"a"], [b""]).tolist() == [-1]   # the empty text is found only where it is an entry


def test_no_entries_and_no_texts():
    got = LE.expected([], [b"a", b""])
    assert got.dtype == np.int64 and got.tolist() == [-1, -1]
    assert _three(LE.filtered([], [b"a", b""])) == ([], [0], b"")
    assert _three(LE.filtered([], [b"a", b""], invert=True)) == ([0, 1], [0, 1, 1], b"a")
    got = LE.expected([b"a"], [])
    assert got.dtype == np.int64 and got.shape == (0,)
    assert _three(LE.filtered([b"a"], [])) == ([], [0], b"")


SYMBOLS = ("mrx_dict_build_dev", "mrx_dict_build_strided_dev", "mrx_dict_free", "mrx_dict_size", "mrx_dict_distinct",
           "mrx_dict_lookup_dev", "mrx_dict_lookup_strided_dev", "mrx_dict_filter_dev", "mrx_dict_filter_known_dev",
           "mrx_dict_filter_strided_dev", "mrx_dict_lookup_batch")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert callable(M.build_dictionary) and callable(M.lookup)
    for name in ("lookup", "isin", "filter", "lookup_async", "filter_async", "__len__", "__del__"):
        assert callable(getattr(M.Dictionary, name))
    assert isinstance(M.Dictionary.distinct_count, property)
    lib.mrx_dict_free(None)   # a no-op
    assert lib.mrx_dict_size(None) == 0 and lib.mrx_dict_distinct(None) == 0


def _tot():
    tot = (C.c_int64 * 2)(-7, -7)
    return tot, C.cast(tot, C.c_void_p)


def test_build_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    out = C.c_void_p(0x5A5A)
    ref = C.byref(out)
    assert lib.mrx_dict_build_dev(FAKE, FAKE, -1, None, ref) == A                  # negative m
    assert lib.mrx_dict_build_dev(FAKE, None, 10, None, ref) == A                  # null d_offsets
    assert lib.mrx_dict_build_dev(FAKE, FAKE, 10, None, None) == A                 # null out
    assert lib.mrx_dict_build_dev(FAKE, FAKE, 1 << 31, None, ref) == A             # an index needs 32 bits
    assert b"n must be below 2^31: a table slot keeps a text's index in 32 bits" in lib.mrx_last_error()
    assert lib.mrx_dict_build_dev(FAKE, FAKE, (1 << 31) + 5, None, ref) == A
    assert lib.mrx_dict_build_strided_dev(FAKE, 64, None, 64, -1, None, ref) == A
    assert lib.mrx_dict_build_strided_dev(FAKE, 64, None, 64, 10, None, None) == A
    assert lib.mrx_dict_build_strided_dev(FAKE, 64, None, 64, 1 << 31, None, ref) == A
    assert b"2^31" in lib.mrx_last_error()
    assert lib.mrx_dict_build_strided_dev(FAKE, 64, None, 65, 10, None, ref) == A  # a length beyond the pitch
    assert lib.mrx_dict_build_strided_dev(FAKE, 64, None, -1, 10, None, ref) == A
    assert lib.mrx_dict_build_strided_dev(FAKE, 0, None, 0, 10, None, ref) == A    # a non-positive pitch
    assert lib.mrx_dict_build_strided_dev(FAKE, -8, None, 0, 10, None, ref) == A
    assert out.value == 0x5A5A                                                     # no handle came back


def test_lookup_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    H = FAKE + 64   # a handle that is never dereferenced
    assert lib.mrx_dict_lookup_dev(None, FAKE, FAKE, 10, FAKE, None) == A          # null handle
    assert lib.mrx_dict_lookup_dev(None, FAKE, FAKE, 0, FAKE, None) == A           # ... for no text too
    assert lib.mrx_dict_lookup_dev(H, FAKE, FAKE, -1, FAKE, None) == A             # negative n
    assert lib.mrx_dict_lookup_dev(H, FAKE, None, 10, FAKE, None) == A             # null d_offsets
    assert lib.mrx_dict_lookup_dev(H, FAKE, FAKE, 10, None, None) == A             # null d_index
    assert lib.mrx_dict_lookup_strided_dev(None, FAKE, 64, None, 64, 10, FAKE, None) == A
    assert lib.mrx_dict_lookup_strided_dev(H, FAKE, 64, None, 64, -1, FAKE, None) == A
    assert lib.mrx_dict_lookup_strided_dev(H, FAKE, 64, None, 64, 10, None, None) == A
    assert lib.mrx_dict_lookup_strided_dev(H, FAKE, 64, None, 65, 10, FAKE, None) == A
    assert lib.mrx_dict_lookup_strided_dev(H, FAKE, 64, None, -1, 10, FAKE, None) == A
    assert lib.mrx_dict_lookup_strided_dev(H, FAKE, 0, None, 0, 10, FAKE, None) == A
    assert lib.mrx_dict_lookup_strided_dev(H, FAKE, -8, None, 0, 10, FAKE, None) == A


def _filter_entry_points(lib):
    """(csr, known, strided) callables taking (handle, flags, n, index, kept_idx, out_offsets, out_data, out_cap, d_totals,
    totals) with a well-formed fake batch between flags and n."""
    return (lambda h, f, n, *t: lib.mrx_dict_filter_dev(h, f, FAKE, FAKE, n, *t, None),
            lambda h, f, n, *t: lib.mrx_dict_filter_known_dev(h, f, FAKE, FAKE, n, 100, 10, *t, None),
            lambda h, f, n, *t: lib.mrx_dict_filter_strided_dev(h, f, FAKE, 64, None, 64, n, *t, None))


def test_filter_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    H = FAKE + 64
    tot, tp = _tot()
    good = (FAKE, FAKE, FAKE, FAKE, 16, FAKE, tp)
    for call in _filter_entry_points(lib):
        assert call(None, 0, 10, *good) == A                                      # null handle
        assert call(None, 0, 0, *good) == A
        assert call(H, 4, 10, *good) == A                                         # unknown flag bits
        assert call(H, 1 | 8, 10, *good) == A
        assert call(H, 0, -1, *good) == A                                         # negative n
        assert call(H, 0, 10, FAKE, FAKE, FAKE, FAKE, -1, FAKE, tp) == A          # negative out_cap
        assert call(H, 0, 10, FAKE, None, FAKE, FAKE, 16, FAKE, tp) == A          # null d_kept_idx
        assert call(H, 0, 10, FAKE, FAKE, None, FAKE, 16, FAKE, tp) == A          # null d_out_offsets
        assert call(H, 0, 10, FAKE, FAKE, FAKE, None, 16, FAKE, tp) == A          # null d_out_data with a capacity
        assert call(H, 0, 10, FAKE, FAKE, FAKE, FAKE, 16, None, tp) == A          # null d_totals
        assert call(H, 0, 0, FAKE, FAKE, None, FAKE, 16, FAKE, tp) == A           # ... for no text too
        assert call(H, 0, 0, FAKE, FAKE, FAKE, FAKE, 16, None, tp) == A
    assert lib.mrx_dict_filter_dev(H, 0, FAKE, None, 10, *good, None) == A        # null d_offsets
    assert lib.mrx_dict_filter_known_dev(H, 0, FAKE, None, 10, 100, 10, *good, None) == A
    assert lib.mrx_dict_filter_known_dev(H, 0, FAKE, FAKE, 10, -1, 10, *good, None) == A   # negative known bounds
    assert lib.mrx_dict_filter_known_dev(H, 0, FAKE, FAKE, 10, 100, -1, *good, None) == A
    assert lib.mrx_dict_filter_strided_dev(H, 0, FAKE, 64, None, 65, 10, *good, None) == A  # a length beyond the pitch
    assert lib.mrx_dict_filter_strided_dev(H, 0, FAKE, 64, None, -1, 10, *good, None) == A
    assert lib.mrx_dict_filter_strided_dev(H, 0, FAKE, 0, None, 0, 10, *good, None) == A    # a non-positive pitch
    assert lib.mrx_dict_filter_strided_dev(H, 0, FAKE, -8, None, 0, 10, *good, None) == A
    assert list(tot) == [-7, -7]


def test_host_entry_point_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    edata, eoff = M.pack_texts([b"abc1", b"zz9"])
    data, off = M.pack_texts([b"zz9", b"q", b"abc1"])
    index = np.full(3 + 4, -5, np.int64)
    batch = lib.mrx_dict_lookup_batch
    ed, eo, d, o, ix = (a.ctypes.data for a in (edata, eoff, data, off, index))
    assert batch(ed, eo, -1, d, o, 3, ix) == A
    assert batch(ed, eo, 2, d, o, -1, ix) == A
    assert batch(ed, None, 2, d, o, 3, ix) == A
    assert batch(ed, eo, 2, d, None, 3, ix) == A
    assert batch(ed, eo, 2, d, o, 3, None) == A
    assert batch(None, eo, 2, d, o, 3, ix) == A                                    # null data of entries with bytes
    assert batch(ed, eo, 2, None, o, 3, ix) == A                                   # ... and of texts with bytes
    assert batch(ed, eo, 1 << 31, d, o, 3, ix) == A                                # refused before the offsets are read
    assert b"2^31" in lib.mrx_last_error()
    bad = np.array([4, 2, 0], np.int64)
    assert batch(ed, bad.ctypes.data, 2, d, o, 3, ix) == A                         # offsets that decrease
    assert batch(ed, eo, 2, d, bad.ctypes.data, 2, ix) == A
    assert index.tolist() == [-5] * 7
