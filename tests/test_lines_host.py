"""Lines without a GPU: the expectation helper (tests/lines_expect.py) pinned against Python's own splitlines and the
oracle's split, the block walk of the kernels on the CPU (mrx_debug_lines_host: the same pieces, the same passes) against
the helper on every batch of the GPU tests, the C ABI's symbols and its argument errors, all of which return before any
device call."""
import numpy as np
import pytest

import mojo_regex_amd as M
import lines_cases as LC
import lines_expect as LE
from mrx_ref import hybrid as O

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C
A = M.api.MRX_E_ARGUMENT


def test_the_table_of_the_contract():
    for t, want in ((b"", []), (b"\n", [b""]), (b"a", [b"a"]), (b"a\nb", [b"a", b"b"]), (b"a\nb\n", [b"a", b"b"]),
                    (b"\n\na", [b"", b"", b"a"])):
        assert LE.lines(t)[0] == want
    assert LE.lines(b"a\r\nb\r", crlf=True) == ([b"a", b"b\r"], 2)
    assert LE.lines(b"a\r\r\n\rb\n", crlf=True)[0] == [b"a\r", b"\rb"]
    assert LE.lines(b"a\nb", partial=False) == ([b"a"], 1)
    assert LE.lines(b"a\nb\n", keepends=True, partial=False) == ([b"a\n", b"b\n"], 0)
    assert LE.lines(b"a;b;;c", sep=b";")[0] == [b"a", b"b", b"", b"c"]


def test_the_expectation_is_pythons_splitlines_and_the_oracles_split():
    rng = np.random.default_rng(5)
    plain = np.frombuffer(b"ab c\n\n", np.uint8)            # splitlines also cuts at \r, \v, \f, \x1c-\x1e, \x85
    paired = [b"a", b"b", b" ", b"\r\n", b"\n", b"\r\n"]
    for rep in range(300):
        t = plain[rng.integers(0, len(plain), size=int(rng.integers(0, 60)))].tobytes()
        assert LE.lines(t)[0] == t.splitlines()
        assert LE.lines(t, keepends=True)[0] == t.splitlines(keepends=True)
        # (the pattern is the newline byte itself: this dialect knows no \n escape, a backslash in front of an n gives
        # the letter n, as the lexer of the reference has it)
        pieces = O.split(b"\n", t)
        assert LE.lines(t)[0] == (pieces[:-1] if pieces and pieces[-1] == b"" else pieces)
        u = b"".join(paired[int(k)] for k in rng.integers(0, len(paired), size=int(rng.integers(0, 40))))
        assert LE.lines(u, crlf=True)[0] == u.splitlines()


def _host(texts, piece_cap=None, out_cap=None, skew=0, sep=b"\n", **opts):
    """mrx_debug_lines_host -> (rc, prefix, owner, offsets, data, totals) with canaries checked."""
    lib = M.load_library()
    flags, sep_byte = M.api._lines_flags(sep, opts.get("keepends", False), opts.get("crlf", False), opts.get("partial", True))
    d, o = M.pack_texts(texts)
    if skew:   # the texts at another alignment, separators in front of them
        d = np.concatenate([np.full(skew, 10, np.uint8), d])
        o = o + skew
    want = LE.expected(texts, sep=sep, **opts)
    pcap = want[4][0] if piece_cap is None else piece_cap
    ocap = want[4][1] if out_cap is None else out_cap
    n = len(texts)
    prefix = np.full(n + 1 + 2, -7, np.int64)
    owner = np.full(pcap + 2, -7, np.int64)
    off = np.full(pcap + 1 + 2, -7, np.int64)
    out = np.full(ocap + 16, 0xEE, np.uint8)
    tot = (C.c_int64 * 4)(-1, -1, -1, -1)
    rc = lib.mrx_debug_lines_host(flags, sep_byte, d.ctypes.data, o.ctypes.data, n, prefix.ctypes.data, owner.ctypes.data,
                                  off.ctypes.data, pcap, out.ctypes.data, ocap, C.cast(tot, C.c_void_p))
    assert prefix[n + 1:].tolist() == [-7, -7] and owner[pcap:].tolist() == [-7, -7] and off[pcap + 1:].tolist() == [-7, -7]
    assert np.all(out[ocap:] == 0xEE)   # nothing behind a capacity
    return rc, prefix[:n + 1], owner[:pcap], off[:pcap + 1], out[:ocap], list(tot), want


def _assert_equal(got, where):
    rc, prefix, owner, off, out, tot, want = got
    assert rc == 0, where
    assert tot == want[4], (where, tot, want[4])
    assert np.array_equal(prefix, want[0]), where
    assert np.array_equal(owner, want[1]), where
    assert np.array_equal(off, want[2]), where
    assert np.array_equal(out, want[3]), where


def test_the_host_walk_on_every_case_of_the_gpu_tests():
    P = LC.piece_length()
    for name, texts in LC.all_cases(P).items():
        for k, opts in enumerate(LE.OPTION_SETS):
            _assert_equal(_host(texts, skew=(3 * k + len(name)) % 16, **opts), (name, opts))


@pytest.mark.parametrize("piece", [1024, 3000, 0])
def test_the_host_walk_at_other_piece_lengths(piece):
    lib = M.load_library()
    try:
        P = lib.mrx_debug_lines_piece(piece)
        assert P % 1024 == 0 and P >= max(piece, 1024)
        for name, texts in LC.piece_edges(P).items():
            for opts in LE.OPTION_SETS + (dict(keepends=True, partial=False), dict(crlf=True, partial=False)):
                _assert_equal(_host(texts, **opts), (name, opts, P))
    finally:
        assert lib.mrx_debug_lines_piece(0) == LC.piece_length()


def test_another_separator():
    texts = [b"a;b;;c", b";", b"", b"x\ny;", b"no separator"]
    for opts in (dict(), dict(keepends=True), dict(partial=False)):
        _assert_equal(_host(texts, sep=b";", **opts), opts)


def test_capacity_on_the_host_walk():
    texts = LC.log_texts(40, 3)
    want = LE.expected(texts)
    lines, nbytes = want[4][0], want[4][1]
    rc, prefix, owner, off, out, tot, _ = _host(texts, piece_cap=lines - 1)
    assert rc == M.api.MRX_E_CAPACITY and tot[0] == lines and tot[1] == nbytes and tot[3] == want[4][3]
    assert np.array_equal(prefix, want[0]) and np.all(out == 0xEE) and np.all(owner == -7) and np.all(off == -7)
    rc, prefix, owner, off, out, tot, _ = _host(texts, out_cap=nbytes - 1)
    assert rc == M.api.MRX_E_CAPACITY and tot == want[4]
    assert np.array_equal(prefix, want[0]) and np.array_equal(owner, want[1]) and np.array_equal(off, want[2])
    assert np.all(out == 0xEE)   # no byte at all


SYMBOLS = ("mrx_lines_dev", "mrx_lines_known_dev", "mrx_lines_strided_dev", "mrx_lines_batch")
HOOKS = ("mrx_debug_lines_piece", "mrx_debug_lines_syncs", "mrx_debug_lines_host")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    for name in HOOKS:
        assert name in M.api.TESTING_SYMBOLS
        assert getattr(lib, name) is not None
    assert callable(M.lines_of)
    for name in ("lines", "from_lines", "lines_async"):
        assert callable(getattr(M.DeviceBatch, name))
    assert (M.api.MRX_LINES_KEEPENDS, M.api.MRX_LINES_CRLF, M.api.MRX_LINES_DROP_PARTIAL) == (1, 2, 4)


def test_argument_errors_come_before_any_device_work():
    lib = M.load_library()
    syncs = lib.mrx_debug_lines_syncs()
    nl, K, CR, DP = 10, M.api.MRX_LINES_KEEPENDS, M.api.MRX_LINES_CRLF, M.api.MRX_LINES_DROP_PARTIAL

    def csr(flags, sep, n=1, pcap=4, ocap=4, data=FAKE, off=FAKE, prefix=FAKE, owner=FAKE, out_off=FAKE, out=FAKE, tot=FAKE):
        return lib.mrx_lines_dev(flags, sep, data, off, n, prefix, owner, out_off, pcap, out, ocap, tot, None, None)

    def known(flags, sep, n=1, end=4, longest=4):
        return lib.mrx_lines_known_dev(flags, sep, FAKE, FAKE, n, end, longest, FAKE, FAKE, FAKE, 4, FAKE, 4, FAKE, None, None)

    def pitch(flags, sep, stride=8, length=8, n=1):
        return lib.mrx_lines_strided_dev(flags, sep, FAKE, stride, None, length, n, FAKE, FAKE, FAKE, 4, FAKE, 4, FAKE, None, None)

    def host(flags, sep):
        d, o = M.pack_texts([b"a\nb"])
        pre, ow, oo, out = np.zeros(2, np.int64), np.zeros(4, np.int64), np.zeros(5, np.int64), np.zeros(4, np.uint8)
        args = (flags, sep, d.ctypes.data, o.ctypes.data, 1, pre.ctypes.data, ow.ctypes.data, oo.ctypes.data, 4, out.ctypes.data, 4, None)
        return lib.mrx_lines_batch(*args), lib.mrx_debug_lines_host(*args)

    for call in (csr, known, pitch):
        assert call(8, nl) == A and b"unknown flag" in lib.mrx_last_error()        # a flag bit that does not exist
        assert call(K | CR | DP | 16, nl) == A
        assert call(CR, ord(";")) == A and b"MRX_LINES_CRLF" in lib.mrx_last_error()   # crlf with another separator
        assert call(CR | K, nl) == A                                                # crlf with keepends
        assert call(CR | K | DP, nl) == A
        assert call(0, nl, n=-1) == A
    assert host(8, nl) == (A, A) and host(CR, ord(";")) == (A, A) and host(CR | K, nl) == (A, A)
    assert csr(0, nl, pcap=-1) == A and csr(0, nl, ocap=-1) == A
    assert csr(0, nl, off=None) == A and csr(0, nl, prefix=None) == A and csr(0, nl, out_off=None) == A
    assert csr(0, nl, tot=None) == A and csr(0, nl, owner=None) == A and csr(0, nl, out=None) == A
    assert known(0, nl, end=-1) == A and known(0, nl, longest=-1) == A
    assert pitch(0, nl, stride=0) == A and pitch(0, nl, stride=8, length=9) == A
    assert lib.mrx_debug_lines_syncs() == syncs   # nothing reached the device
    with pytest.raises(M.MrxError):
        M.api._lines_flags(b"\r\n", False, False, True)   # one byte only
    with pytest.raises(M.MrxError):
        M.api._lines_flags(b"", False, False, True)
