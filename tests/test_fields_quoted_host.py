"""Quoted fields without a GPU (include/mrx.h, "quoted fields"): the expectation helper (tests/fields_quoted_expect.py)
pinned against the table of the contract, against csv.reader on rows that csv.writer wrote and against
tests/fields_expect.py on texts without a quote; then the walk of the kernel on the CPU (mrx_debug_fields_quoted_host:
the same groups, rounds, ballots and carried parity) against the helper, the C ABI's symbols and its argument errors,
all of which return before any device call."""
import csv

import numpy as np
import pytest

import mojo_regex_amd as M
import fields_cases as FC
import fields_expect as FE
import fields_quoted_cases as QC
import fields_quoted_expect as QE

FAKE = 1 << 40   # a device pointer that is never dereferenced
A = M.api.MRX_E_ARGUMENT
W, R = M.api.MRX_FIELDS_WHITESPACE, M.api.MRX_FIELDS_REST
Q = QC.Q


def _host(texts, columns, delim=None, rest=False, skew=0, counts=True, prefix=True, quoted=True, quote=Q):
    """mrx_debug_fields_quoted_host -> (rc, rows, nf, prefix, quoted), canaries behind all four checked."""
    lib = M.load_library()
    flags, delim_byte, cols = M.api._fields_args(columns, delim, rest)
    d, o = M.pack_texts(texts)
    if skew:   # the texts at another alignment, an odd number of quote bytes in front of them
        d = np.concatenate([np.full(skew, quote[0], np.uint8), d])
        o = o + skew
    n, f = len(texts), len(cols)
    rows = np.full(n * f * 2 + 4, -7, np.int32)
    nf = np.full(n + 2, -7, np.int32)
    pre = np.full(n + 1 + 2, -7, np.int64)
    qd = np.full(n * f + 3, 0xEE, np.uint8)
    rc = lib.mrx_debug_fields_quoted_host(flags, delim_byte, quote[0], cols.ctypes.data, f, d.ctypes.data, o.ctypes.data, n,
                                          rows.ctypes.data, nf.ctypes.data if counts else None,
                                          qd.ctypes.data if quoted else None, pre.ctypes.data if prefix else None)
    assert rows[n * f * 2:].tolist() == [-7] * 4 and nf[n:].tolist() == [-7, -7] and pre[n + 1:].tolist() == [-7, -7]
    assert qd[n * f:].tolist() == [0xEE] * 3
    if not counts:
        assert np.all(nf == -7)
    if not prefix:
        assert np.all(pre == -7)
    if not quoted:
        assert np.all(qd == 0xEE)
    return rc, rows[:n * f * 2].reshape(n, f, 2), nf[:n], pre[:n + 1], qd[:n * f].reshape(n, f)


def _assert_host(texts, columns, delim, rest, where, **kw):
    want = QE.expected(texts, columns, kw.get("quote", Q), delim, rest)
    rc, rows, nf, pre, qd = _host(texts, columns, delim, rest, **kw)
    assert rc == 0, where
    assert np.array_equal(rows, want[0]), (where, [(texts[i], rows[i].tolist(), want[0][i].tolist())
                                                   for i in np.nonzero((rows != want[0]).any(axis=(1, 2)))[0][:3]])
    if kw.get("counts", True):
        assert np.array_equal(nf, want[1]), where
    if kw.get("prefix", True):
        assert np.array_equal(pre, want[2]), where
    if kw.get("quoted", True):
        assert np.array_equal(qd, want[3]), where


@pytest.fixture
def pin():
    lib = M.load_library()

    def set_group(G):
        assert lib.mrx_debug_fields_group(G) == G

    yield set_group
    assert lib.mrx_debug_fields_group(0) == 0


# ---- the expectation itself --------------------------------------------------------------------------------------------

def test_the_expectation_gives_the_table_of_the_contract():
    for t, delim, rest, cols, want_row, want_quoted in QC.TABLE:
        pairs, nf, quoted = QE.row(t, cols, Q, delim, rest)
        assert (pairs, quoted) == (want_row, want_quoted), (t, cols)
    assert QE.decoded(b'a,"b""c",d', Q, 3, 7) == b'b"c'
    assert QE.row(b'a,"b,c",d', [1], Q, b",")[1] == 3 and QE.row(b'a "b c"  d', [1], Q)[1] == 3
    assert QE.row(b'a,"b,c",d', [2], Q, b",", True)[1] == 2


def test_the_expectation_agrees_with_csv_reader():
    lines, cells = QC.csv_rows()
    assert len(lines) == 2000
    read = list(csv.reader([l.decode() for l in lines]))
    assert len(read) == len(lines)
    for line, wrote, back in zip(lines, cells, read):   # every row, none left out
        assert [c.encode() for c in back] == wrote, line
        assert QE.cells(line) == wrote, line
    assert sum(b'""' in l[1:-1] for l in lines) > 200 and sum(b'",' in l for l in lines) > 500   # quotes are common


def test_without_a_quote_byte_the_expectation_is_plain_fields():
    texts = [t for t in FC.short_texts(200, seed=2) + FC.log_lines(40, seed=2) + list(FC.edges(4, 44).values()) if Q not in t]
    assert len(texts) > 200
    for delim in (b",", None, b" "):
        for cols, rest in FC.REQUESTS:
            want = FE.expected(texts, cols, delim, rest)
            got = QE.expected(texts, cols, Q, delim, rest)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not got[3].any()


# ---- the walk on the CPU ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", QC.GROUPS + (0,))
def test_the_host_walk_gives_the_table(G, pin):
    pin(G)
    for t, delim, rest, cols, want_row, want_quoted in QC.TABLE:
        rc, rows, nf, pre, qd = _host([t], cols, delim, rest)
        assert rc == 0
        assert [tuple(p) for p in rows[0].tolist()] == want_row, (t, cols)
        assert qd[0].tolist() == want_quoted and pre.tolist() == [0, 1]
        assert nf.tolist() == [QE.row(t, cols, Q, delim, rest)[1]]


@pytest.mark.parametrize("G", QC.GROUPS + (0,))
def test_the_host_walk_on_the_edges_of_a_group(G, pin):
    pin(G)
    for delim in QC.MODES:
        cases = QC.edges(G or 2, delim[0] if delim else 32)
        texts = list(cases.values())
        for k, (cols, rest) in enumerate(QC.REQUESTS + ((QC.WIDE, False),)):
            for skew in QC.SKEWS:
                _assert_host(texts, cols, delim, rest, (G, delim, cols, rest, skew), skew=skew, counts=k % 3 != 1,
                             quoted=k % 4 != 2)


@pytest.mark.parametrize("skew", QC.SKEWS)
def test_the_host_walk_on_generated_batches(skew, pin):
    lines, _ = QC.csv_rows(300, seed=5)
    for G in QC.GROUPS + (0,):
        pin(G)
        texts = QC.generated_texts(65, seed=G) + QC.combined_log_lines(10, seed=G) + lines[:60]
        for delim in (b",", None, b" "):
            for cols, rest in QC.REQUESTS:
                _assert_host(texts, cols, delim, rest, (G, delim, cols, rest), skew=skew)
            _assert_host(texts, [1, 3], delim, False, (G, delim, "no nf"), skew=skew, counts=False)   # the early stop
            _assert_host(texts, [2, -1], delim, False, (G, delim, "rows alone"), skew=skew, counts=False, prefix=False, quoted=False)
        _assert_host(texts, [1, 2, -1], b",", False, (G, "another quote"), skew=skew, quote=b"'")
        _assert_host(texts, [1, 2, -1], b"a", False, (G, "a letter for a delimiter"), skew=skew, quote=b"b")


def test_the_host_walk_agrees_with_csv_reader(pin):
    lines, cells = QC.csv_rows()
    for G in (1, 4, 0):
        pin(G)
        rc, rows, nf, pre, qd = _host(lines, [1, 2, 3, 4, 5, 6], b",")
        assert rc == 0 and nf.tolist() == [len(c) for c in cells]
        for i, (line, wrote) in enumerate(zip(lines, cells)):
            got = [QE.decoded(line, Q, int(s), int(e)) for s, e in rows[i][:len(wrote)]]
            assert got == wrote and rows[i][len(wrote):].tolist() == [[-1, -1]] * (6 - len(wrote)), line


def test_plain_fields_are_what_they_were_on_texts_with_quotes():
    """mrx_debug_fields_host knows no quote: the quoted texts split at every delimiter, as before."""
    lib = M.load_library()
    texts = QC.generated_texts(80, seed=1)
    flags, delim_byte, cols = M.api._fields_args([1, 2, -1], b",", False)
    d, o = M.pack_texts(texts)
    rows, nf = np.zeros((len(texts), 3, 2), np.int32), np.zeros(len(texts), np.int32)
    assert lib.mrx_debug_fields_host(flags, delim_byte, cols.ctypes.data, 3, d.ctypes.data, o.ctypes.data, len(texts),
                                     rows.ctypes.data, nf.ctypes.data, None) == 0
    want = FE.expected(texts, [1, 2, -1], b",")
    assert np.array_equal(rows, want[0]) and np.array_equal(nf, want[1])


def test_no_text_writes_nothing():
    rc, rows, nf, pre, qd = _host([], [1, -1], b",")
    assert rc == 0 and pre.tolist() == [-7]   # n == 0: not even prefix[0]


SYMBOLS = ("mrx_fields_quoted_dev", "mrx_fields_quoted_strided_dev", "mrx_fields_quoted_batch")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "mrx_debug_fields_quoted_host" in M.api.TESTING_SYMBOLS and lib.mrx_debug_fields_quoted_host is not None
    assert callable(M.csv_of) and callable(M.csv_columns)
    import inspect
    for fn in (M.DeviceBatch.fields, M.DeviceBatch.fields_async, M.DeviceBatch.cut, M.fields_of):
        assert inspect.signature(fn).parameters["quote"].default is None


def test_argument_errors_come_before_any_device_work():
    lib = M.load_library()

    def arr(cols):
        return np.array(cols, np.int32)

    def csr(flags, cols, n=1, off=FAKE, rows=FAKE, f=None, colp=True, delim=44, quote=34, quoted=FAKE):
        c = arr(cols)
        return lib.mrx_fields_quoted_dev(flags, delim, quote, c.ctypes.data if colp else None, len(c) if f is None else f, FAKE,
                                         off, n, rows, FAKE, quoted, FAKE, None)

    def pitch(flags, cols, n=1, stride=8, length=8, rows=FAKE, f=None, colp=True, delim=44, quote=34, quoted=FAKE, off=None):
        c = arr(cols)
        return lib.mrx_fields_quoted_strided_dev(flags, delim, quote, c.ctypes.data if colp else None,
                                                 len(c) if f is None else f, FAKE, stride, None, length, n, rows, FAKE, quoted,
                                                 FAKE, None)

    def host(flags, cols, n=1, f=None, colp=True, rows=True, off=True, delim=44, quote=34, quoted=False):
        c = arr(cols)
        d, o = M.pack_texts([b"a,b"])
        r = np.zeros(2 * max(len(c), 1), np.int32)
        qd = np.zeros(max(len(c), 1), np.uint8)
        args = (flags, delim, quote, c.ctypes.data if colp else None, len(c) if f is None else f, d.ctypes.data,
                o.ctypes.data if off else None, n, r.ctypes.data if rows else None, None, qd.ctypes.data if quoted else None, None)
        return lib.mrx_fields_quoted_batch(*args), lib.mrx_debug_fields_quoted_host(*args)

    for call in (csr, pitch):
        # everything that fields refuses
        assert call(4, [1]) == A and b"unknown flag" in lib.mrx_last_error()
        assert call(W | R | 8, [1]) == A
        assert call(0, [1], f=0) == A and call(0, [1] * 33) == A and b"MRX_FIELDS_MAX_COLUMNS" in lib.mrx_last_error()
        assert call(0, [1, 0, 2]) == A and b"must not be 0" in lib.mrx_last_error()
        assert call(R, [2, -1]) == A and b"MRX_FIELDS_REST" in lib.mrx_last_error()
        assert call(0, [1], n=-1) == A
        assert call(0, [1], rows=None, quoted=None) == A and b"null argument" in lib.mrx_last_error()
        assert call(0, [1], colp=False) == A
        assert call(0, [1], rows=FAKE + 4) == A
        # and the quote's own
        assert call(0, [1], delim=44, quote=44) == A and b"quote must differ from delim" in lib.mrx_last_error()
        assert call(R, [2], delim=34, quote=34) == A
        for ws in FE.WHITESPACE:
            assert call(W, [1], quote=ws) == A and b"whitespace byte" in lib.mrx_last_error()
            assert call(0, [1], quote=ws, n=0) == 0   # a delimiter mode's quote may be any other byte
        assert call(W, [1], delim=34, quote=34, n=0) == 0   # whitespace mode ignores delim
        assert call(0, [1], rows=None) == A and b"d_quoted needs d_rows" in lib.mrx_last_error()
    assert csr(0, [1], off=None) == A
    assert pitch(0, [1], stride=0) == A and pitch(0, [1], stride=8, length=9) == A
    for bad in ((4, [1]), (0, [0]), (R, [-1]), (0, [1] * 33)):
        assert host(*bad) == (A, A)
    assert host(0, [1], quote=44) == (A, A) and host(W, [1], quote=32) == (A, A)
    assert host(0, [1], rows=False, quoted=True) == (A, A) and b"d_quoted needs d_rows" in lib.mrx_last_error()
    assert host(0, [1], f=0) == (A, A) and host(0, [1], n=-1) == (A, A)
    assert host(0, [1], colp=False) == (A, A) and host(0, [1], rows=False) == (A, A) and host(0, [1], off=False) == (A, A)
    # n == 0 with good arguments: nothing to do, on any form
    assert csr(0, [1], n=0) == 0 and csr(W, [1, -1], n=0) == 0 and pitch(R, [2], n=0) == 0
    # plain fields still refuses flag value 4: no quote flag hides there
    c = arr([1])
    assert lib.mrx_fields_dev(4, 44, c.ctypes.data, 1, FAKE, FAKE, 1, FAKE, FAKE, FAKE, None) == A
    for bad in (b"", b'""'):
        with pytest.raises(M.MrxError, match="single byte"):
            M.api._quote_byte(bad)
    with pytest.raises(M.MrxError):
        M.fields_of([b"a"], [1], delim=b",", quote=b",,")
