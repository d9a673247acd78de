"""Fields without a GPU: the table of the contract, the expectation helper (tests/fields_expect.py) pinned against
bytes.split itself, the walk of the kernel on the CPU (mrx_debug_fields_host: the same groups, the same rounds) against
the helper on the batches of the GPU tests, the C ABI's symbols and its argument errors, all of which return before any
device call."""
import numpy as np
import pytest

import mojo_regex_amd as M
import fields_cases as FC
import fields_expect as FE

FAKE = 1 << 40   # a device pointer that is never dereferenced
A = M.api.MRX_E_ARGUMENT
W, R = M.api.MRX_FIELDS_WHITESPACE, M.api.MRX_FIELDS_REST

# (text, delim, rest, columns, row, nf): include/mrx.h, "fields"
TABLE = (
    (b"", b",", False, [1, -1], [(0, 0), (0, 0)], 1),
    (b"", None, False, [1, -1], [(-1, -1), (-1, -1)], 0),
    (b" a  b c ", None, False, [1, 2, 3, -1], [(1, 2), (4, 5), (6, 7), (6, 7)], 3),
    (b" a  b c ", None, True, [2], [(4, 8)], 2),
    (b"a,b,,c", b",", False, [3, 4, 5, -4, -5], [(4, 4), (5, 6), (-1, -1), (0, 1), (-1, -1)], 4),
    (b"a,b,,c", b",", True, [2], [(2, 6)], 2),
)


def _host(texts, columns, delim=None, rest=False, skew=0, counts=True, prefix=True):
    """mrx_debug_fields_host -> (rc, rows, nf, prefix), canaries behind all three checked."""
    lib = M.load_library()
    flags, delim_byte, cols = M.api._fields_args(columns, delim, rest)
    d, o = M.pack_texts(texts)
    if skew:   # the texts at another alignment, delimiter bytes in front of them
        d = np.concatenate([np.full(skew, delim_byte or 32, np.uint8), d])
        o = o + skew
    n, f = len(texts), len(cols)
    rows = np.full(n * f * 2 + 4, -7, np.int32)
    nf = np.full(n + 2, -7, np.int32)
    pre = np.full(n + 1 + 2, -7, np.int64)
    rc = lib.mrx_debug_fields_host(flags, delim_byte, cols.ctypes.data, f, d.ctypes.data, o.ctypes.data, n, rows.ctypes.data,
                                   nf.ctypes.data if counts else None, pre.ctypes.data if prefix else None)
    assert rows[n * f * 2:].tolist() == [-7] * 4 and nf[n:].tolist() == [-7, -7] and pre[n + 1:].tolist() == [-7, -7]
    if not counts:
        assert np.all(nf == -7)
    if not prefix:
        assert np.all(pre == -7)
    return rc, rows[:n * f * 2].reshape(n, f, 2), nf[:n], pre[:n + 1]


def _assert_host(texts, columns, delim, rest, where, **kw):
    want = FE.expected(texts, columns, delim, rest)
    rc, rows, nf, pre = _host(texts, columns, delim, rest, **kw)
    assert rc == 0, where
    assert np.array_equal(rows, want[0]), (where, rows.tolist(), want[0].tolist())
    if kw.get("counts", True):
        assert np.array_equal(nf, want[1]), where
    if kw.get("prefix", True):
        assert np.array_equal(pre, want[2]), where


def test_the_table_of_the_contract():
    for t, delim, rest, cols, want_row, want_nf in TABLE:
        assert FE.row(t, cols, delim, rest) == (want_row, want_nf), (t, cols)
        rc, rows, nf, pre = _host([t], cols, delim, rest)
        assert rc == 0
        assert [tuple(p) for p in rows[0].tolist()] == want_row, (t, cols)
        assert nf.tolist() == [want_nf] and pre.tolist() == [0, 1]


def test_the_expectation_is_bytes_split_itself():
    assert bytes(b for b in range(256) if bytes([b]).isspace()) == FE.WHITESPACE
    rng = np.random.default_rng(11)
    al = np.frombuffer(b"ab,, \t\n1;", np.uint8)
    for rep in range(600):
        t = al[rng.integers(0, len(al), size=int(rng.integers(0, 61)))].tobytes()
        for delim in (b",", None):
            for maxsplit in (-1, 0, 1, 3):
                assert [t[s:e] for s, e in FE.parts(t, delim, maxsplit)] == t.split(delim, maxsplit), (t, delim, maxsplit)
    for b in range(256):   # one byte between two letters: a separator exactly when Python says so
        t = b"a" + bytes([b]) + b"c"
        assert len(FE.parts(t)) == len(t.split()) == (2 if bytes([b]).isspace() else 1)


def test_the_host_walk_knows_the_same_six_whitespace_bytes():
    texts = [b"a" + bytes([b]) + b"c" for b in range(256)]
    _assert_host(texts, [1, -1, 2], None, False, "every byte value")


@pytest.mark.parametrize("G", FC.GROUPS)
def test_the_host_walk_on_the_edges_of_a_group(G):
    lib = M.load_library()
    try:
        assert lib.mrx_debug_fields_group(G) == G
        for delim in FC.MODES:
            sep = delim[0] if delim else 32
            cases = FC.edges(G, sep)
            texts = list(cases.values())
            for k, (cols, rest) in enumerate(FC.REQUESTS + ((FC.WIDE, False),)):
                _assert_host(texts, cols, delim, rest, (G, delim, cols, rest), skew=(0, 1, 7, 15)[k % 4], counts=k % 3 != 1)
            for name, t in cases.items():   # REST with cmax equal to 1, nf and nf + 1
                for cols, rest in FC.rest_requests(FE.row(t, [1], delim)[1]):
                    _assert_host([t], cols, delim, rest, (G, delim, name, cols))
    finally:
        assert lib.mrx_debug_fields_group(0) == 0


@pytest.mark.parametrize("skew", [0, 1, 7, 15])
def test_the_host_walk_on_generated_batches(skew):
    lib = M.load_library()
    try:
        for G in FC.GROUPS + (0,):
            assert lib.mrx_debug_fields_group(G) == G
            texts = FC.short_texts(65, seed=G) + FC.log_lines(20, seed=G)
            for delim in (b",", None, b" "):
                for cols, rest in FC.REQUESTS:
                    _assert_host(texts, cols, delim, rest, (G, delim, cols, rest), skew=skew)
                _assert_host(texts, [1, 3], delim, False, (G, delim, "no nf"), skew=skew, counts=False)   # the early stop
                _assert_host(texts, [2, -1], delim, False, (G, delim, "no nf, no prefix"), skew=skew, counts=False, prefix=False)
    finally:
        assert lib.mrx_debug_fields_group(0) == 0


def test_the_group_hook():
    lib = M.load_library()
    try:
        assert lib.mrx_debug_fields_group(0) == 0
        for g in (1, 2, 4, 8, 16, 32, 64):
            assert lib.mrx_debug_fields_group(g) == g
        for bad in (3, 65, 128, -1):   # changes nothing
            assert lib.mrx_debug_fields_group(bad) == 64
    finally:
        assert lib.mrx_debug_fields_group(0) == 0


def test_no_text_writes_nothing():
    rc, rows, nf, pre = _host([], [1, -1], b",")
    assert rc == 0 and pre.tolist() == [-7]   # n == 0: not even prefix[0]


SYMBOLS = ("mrx_fields_dev", "mrx_fields_known_dev", "mrx_fields_strided_dev", "mrx_fields_batch")
HOOKS = ("mrx_debug_fields_group", "mrx_debug_fields_grid", "mrx_debug_fields_host")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    for name in HOOKS:
        assert name in M.api.TESTING_SYMBOLS
        assert getattr(lib, name) is not None
    assert callable(M.fields_of)
    for name in ("fields", "fields_async", "cut"):
        assert callable(getattr(M.DeviceBatch, name))
    assert (W, R, M.api.MRX_FIELDS_MAX_COLUMNS) == (1, 2, 32)


def test_argument_errors_come_before_any_device_work():
    lib = M.load_library()

    def arr(cols):
        return np.array(cols, np.int32)

    def csr(flags, cols, n=1, data=FAKE, off=FAKE, rows=FAKE, f=None, colp=True):
        c = arr(cols)
        return lib.mrx_fields_dev(flags, 44, c.ctypes.data if colp else None, len(c) if f is None else f, data, off, n, rows,
                                  FAKE, FAKE, None)

    def known(flags, cols, n=1, end=4, longest=4, rows=FAKE, off=FAKE, f=None, colp=True):
        c = arr(cols)
        return lib.mrx_fields_known_dev(flags, 44, c.ctypes.data if colp else None, len(c) if f is None else f, FAKE, off, n,
                                        end, longest, rows, FAKE, FAKE, None)

    def pitch(flags, cols, n=1, stride=8, length=8, rows=FAKE, f=None, colp=True, off=None):
        c = arr(cols)
        return lib.mrx_fields_strided_dev(flags, 44, c.ctypes.data if colp else None, len(c) if f is None else f, FAKE, stride,
                                          None, length, n, rows, FAKE, FAKE, None)

    def host(flags, cols, n=1, f=None, colp=True, rows=True, off=True):
        c = arr(cols)
        d, o = M.pack_texts([b"a,b"])
        r = np.zeros(2 * max(len(c), 1), np.int32)
        args = (flags, 44, c.ctypes.data if colp else None, len(c) if f is None else f, d.ctypes.data,
                o.ctypes.data if off else None, n, r.ctypes.data if rows else None, None, None)
        return lib.mrx_fields_batch(*args), lib.mrx_debug_fields_host(*args)

    for call in (csr, known, pitch):
        assert call(4, [1]) == A and b"unknown flag" in lib.mrx_last_error()
        assert call(W | R | 8, [1]) == A
        assert call(0, [1], f=0) == A and call(0, [1] * 33) == A and b"MRX_FIELDS_MAX_COLUMNS" in lib.mrx_last_error()
        assert call(0, [1, 0, 2]) == A and b"must not be 0" in lib.mrx_last_error()
        assert call(R, [2, -1]) == A and b"MRX_FIELDS_REST" in lib.mrx_last_error()
        assert call(W | R, [-1]) == A
        assert call(0, [1], n=-1) == A
        assert call(0, [1], rows=None) == A and call(0, [1], colp=False) == A
        assert call(0, [1], rows=FAKE + 4) == A   # a misaligned row block
    assert csr(0, [1], off=None) == A and known(0, [1], off=None) == A
    assert known(0, [1], end=-1) == A and known(0, [1], longest=-1) == A
    assert pitch(0, [1], stride=0) == A and pitch(0, [1], stride=8, length=9) == A
    for bad in ((4, [1]), (0, [0]), (R, [-1]), (0, [1] * 33)):
        assert host(*bad) == (A, A)
    assert host(0, [1], f=0) == (A, A) and host(0, [1], n=-1) == (A, A)
    assert host(0, [1], colp=False) == (A, A) and host(0, [1], rows=False) == (A, A) and host(0, [1], off=False) == (A, A)
    # n == 0 with good arguments: nothing to do, on any form
    assert csr(0, [1], n=0) == 0 and known(W, [1, -1], n=0) == 0 and pitch(R, [2], n=0) == 0
    with pytest.raises(M.MrxError):
        M.api._fields_args([1], b",,", False)   # one byte only
    with pytest.raises(M.MrxError):
        M.api._fields_args([1], b"", False)
    with pytest.raises(M.MrxError):
        M.DeviceBatch.cut(None, list(range(1, 11)))   # expand's limit, said before anything else is looked at
