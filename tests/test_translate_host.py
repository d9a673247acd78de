"""Translate and strip without a GPU: the expectation helper (tests/translate_expect.py) pinned against Python's own
bytes methods and a squeeze written twice more, the block walks of the kernels on the CPU (mrx_debug_translate_host,
mrx_debug_strip_host: the same pieces, the same passes) against the helper on every batch of the GPU
tests, the C ABI's symbols and its argument errors, all of which return before any device call."""
import itertools
import re

import numpy as np
import pytest

import mojo_regex_amd as M
import translate_cases as TC
import translate_expect as TE

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C
A, CAPACITY = M.api.MRX_E_ARGUMENT, M.api.MRX_E_CAPACITY
L, R = M.api.MRX_STRIP_LEFT, M.api.MRX_STRIP_RIGHT


def test_the_table_of_the_contract():
    assert TE.translate(b"GET /A b", TE.LOWER) == b"get /a b"
    assert TE.translate(b"a\r\n", delete=b"\r") == b"a\n"
    assert TE.translate(b"a  b   c", squeeze=b" ") == b"a b c"
    assert TE.translate(b"a\t b", TE.TAB_TO_SPACE, squeeze=b" ") == b"a b"
    assert TE.translate(b"aab", squeeze=b" ") == b"aab"
    for t, flags, want in ((b"  42 ", (True, True), (2, 4)), (b"  42 ", (True, False), (2, 5)), (b"  42 ", (False, True), (0, 4)),
                           (b"   ", (True, False), (3, 3)), (b"   ", (True, True), (3, 3)), (b"   ", (False, True), (0, 0)),
                           (b"", (True, True), (0, 0))):
        assert TE.strip(t, None, *flags) == want


def test_the_expectation_is_pythons_own():
    rng = np.random.default_rng(5)
    for rep in range(300):
        t = TC._mixed(int(rng.integers(0, 80)), rep)
        assert TE.translate(t, TE.LOWER) == t.lower() and TE.translate(t, TE.UPPER) == t.upper()
        assert TE.translate(t, None, b"\r a") == t.replace(b"\r", b"").replace(b" ", b"").replace(b"a", b"")
        for sq in (b" ", b" \t-ab"):   # tr -s twice more: runs collapsed by a regex, and group by group
            by_regex = re.sub(b"([" + re.escape(sq) + b"])\\1+", b"\\1", t)
            by_group = b"".join(bytes([c]) * (1 if c in sq else len(list(g))) for c, g in itertools.groupby(t))
            assert TE.translate(t, squeeze=sq) == by_regex == by_group
        for chars in (None, b" \t\"'", b"ab", b""):
            for left, right, py in ((True, True, t.strip), (True, False, t.lstrip), (False, True, t.rstrip)):
                a, b = TE.strip(t, chars, left, right)
                assert t[a:b] == (py(chars) if chars != b"" else t), (t, chars, left, right)
                assert (a == 0 or left) and (b == len(t) or right)
    # a text of set bytes alone: where the empty result lies
    assert TE.strip(b"    ", None, True, True) == (4, 4) and TE.strip(b"    ", None, False, True) == (0, 0)


_WANT = {}


def _want(name, texts, params):
    key = (name, len(texts), sum(len(t) for t in texts), tuple(sorted(params.items())))
    if key not in _WANT:
        _WANT[key] = TE.expected(texts, **params)
    return _WANT[key]


def _host(texts, params, out_cap=None, skew=0, want=None):
    """mrx_debug_translate_host -> (rc, offsets, data, totals, want) with canaries checked."""
    lib = M.load_library()
    table, dele, sq = M.api._translate_args(**params)
    d, o = M.pack_texts(texts)
    if skew:   # the texts at another alignment, members of the sets in front of them
        d = np.concatenate([np.frombuffer((b" \r" * 8)[:skew], np.uint8), d])
        o = o + skew
    want = TE.expected(texts, **params) if want is None else want
    ocap = want[2][0] if out_cap is None else out_cap
    n = len(texts)
    off = np.full(n + 1 + 2, -7, np.int64)
    out = np.full(ocap + 16, 0xEE, np.uint8)
    tot = (C.c_int64 * 2)(-1, -1)
    rc = lib.mrx_debug_translate_host(table, dele, sq, d.ctypes.data, o.ctypes.data, n, off.ctypes.data, out.ctypes.data, ocap,
                                      C.cast(tot, C.c_void_p))
    assert off[n + 1:].tolist() == [-7, -7] and np.all(out[ocap:] == 0xEE)   # nothing behind a capacity
    return rc, off[:n + 1], out[:ocap], list(tot), want


def _assert_equal(got, where):
    rc, off, out, tot, want = got
    assert rc == 0, where
    assert tot == want[2], (where, tot, want[2])
    assert np.array_equal(off, want[0]), where
    assert np.array_equal(out, want[1]), where


def test_the_host_walk_on_every_case_of_the_gpu_tests():
    P = TC.piece_length()
    for name, texts in TC.all_cases(P).items():
        for k, params in enumerate(TE.PARAMETER_SETS):
            _assert_equal(_host(texts, params, skew=(3 * k + len(name)) % 16, want=_want(name, texts, params)), (name, params))


def test_the_host_walk_at_every_alignment():
    P = TC.piece_length()
    edges = TC.piece_edges(P)
    names = ["runs_over_block_round_and_piece_edges_space", "runs_over_block_round_and_piece_edges_cr", "a_run_only_behind_the_map"]
    batches = [(name, edges[name]) for name in names] + [("mixed", TC.mixed_texts(20, 3, longest=70))]
    for name, texts in batches:
        for params in TE.PARAMETER_SETS:
            for skew in range(16):
                _assert_equal(_host(texts, params, skew=skew, want=_want(name, texts, params)), (name, params, skew))


@pytest.mark.parametrize("piece", [1024, 3000])
def test_the_host_walk_at_other_piece_lengths(piece):
    lib = M.load_library()
    try:
        P = lib.mrx_debug_translate_piece(piece)
        assert P % 1024 == 0 and P >= piece
        for name, texts in TC.piece_edges(P).items():
            for k, params in enumerate(TE.PACKED):
                _assert_equal(_host(texts, params, skew=(5 * k + len(name)) % 16), (name, params, P))
    finally:
        assert lib.mrx_debug_translate_piece(0) == TC.piece_length()


def test_capacity_on_the_host_walk():
    texts = TC.mixed_texts(40, 3)
    for params in (dict(delete=b"\r"), dict(squeeze=b" "), dict(table=TE.LOWER)):
        want = TE.expected(texts, **params)
        rc, off, out, tot, _ = _host(texts, params, out_cap=want[2][0] - 1)
        assert rc == CAPACITY and tot == want[2] and np.array_equal(off, want[0])
        assert np.all(out == 0xEE)   # no byte at all


def _strip_host(texts, opts, skew=0):
    lib = M.load_library()
    d, o = M.pack_texts(texts)
    if skew:
        d = np.concatenate([np.frombuffer((b" Z" * 8)[:skew], np.uint8), d])
        o = o + skew
    n = len(texts)
    rows = np.full(2 * n + 2, -7, np.int32)
    prefix = np.full(n + 1 + 2, -7, np.int64)
    chars = opts.get("chars")
    flags = M.api._strip_flags(opts.get("left", True), opts.get("right", True))
    rc = lib.mrx_debug_strip_host(None if chars is None else M.api._byte_set(chars), flags, d.ctypes.data, o.ctypes.data, n,
                                  rows.ctypes.data, prefix.ctypes.data)
    assert rc == 0 and rows[2 * n:].tolist() == [-7, -7] and prefix[n + 1:].tolist() == [-7, -7]
    assert prefix[:n + 1].tolist() == list(range(n + 1))
    return rows[:2 * n].reshape(n, 1, 2)


def _strip_batches(opts):
    chars = opts.get("chars")
    s = b" " if not chars else chars[:1]
    return [TC.strip_texts(s), TC.mixed_texts(60, 9, longest=60), TC.strip_texts(s, b"\n" if chars else b"Z")[::-1]]


def test_the_strip_walk_on_every_case():
    for opts in TE.STRIPS:
        for k, texts in enumerate(_strip_batches(opts)):
            for skew in range(16):
                assert np.array_equal(_strip_host(texts, opts, skew), TE.strip_rows(texts, **opts)), (opts, k, skew)
    assert _strip_host([], {}).shape == (0, 1, 2)


SYMBOLS = ("mrx_translate_dev", "mrx_translate_known_dev", "mrx_translate_strided_dev", "mrx_translate_batch",
           "mrx_strip_dev", "mrx_strip_known_dev", "mrx_strip_strided_dev", "mrx_strip_batch")
HOOKS = ("mrx_debug_translate_piece", "mrx_debug_translate_syncs", "mrx_debug_translate_host",
         "mrx_debug_strip_host")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    for name in HOOKS:
        assert name in M.api.TESTING_SYMBOLS
        assert getattr(lib, name) is not None
    assert callable(M.translate_texts) and callable(M.strip_texts)
    for name in ("translate", "translate_async", "lower", "upper", "strip", "strip_async"):
        assert callable(getattr(M.DeviceBatch, name))
    assert (L, R) == (1, 2)
    assert M.api._LOWER == bytes(range(256)).lower() and M.api._UPPER == bytes(range(256)).upper()


def test_argument_errors_come_before_any_device_work():
    lib = M.load_library()
    syncs = lib.mrx_debug_translate_syncs()
    cr, sp = M.api._byte_set(b"\r"), M.api._byte_set(b" ")

    def csr(dele=None, sq=None, n=1, ocap=4, data=FAKE, off=FAKE, out=FAKE, out_off=FAKE, tot=FAKE):
        return lib.mrx_translate_dev(None, dele, sq, data, off, n, out, ocap, out_off, tot, None, None)

    def known(dele=None, sq=None, n=1, end=4, longest=4, ocap=4):
        return lib.mrx_translate_known_dev(None, dele, sq, FAKE, FAKE, n, end, longest, FAKE, ocap, FAKE, FAKE, None, None)

    def pitch(dele=None, sq=None, stride=8, length=8, n=1, ocap=8):
        return lib.mrx_translate_strided_dev(None, dele, sq, FAKE, stride, None, length, n, FAKE, ocap, FAKE, FAKE, None, None)

    def host(dele, sq, n=1, ocap=4):
        d, o = M.pack_texts([b"a  b"])
        oo, out = np.zeros(2, np.int64), np.zeros(4, np.uint8)
        args = (None, dele, sq, d.ctypes.data, o.ctypes.data, n, oo.ctypes.data, out.ctypes.data, ocap, None)
        return lib.mrx_translate_batch(*args), lib.mrx_debug_translate_host(*args)

    for call in (csr, known, pitch):
        assert call(cr, sp) == A and b"delete and squeeze" in lib.mrx_last_error()
        assert call(cr, None, n=-1) == A and call(None, None, n=-1) == A
        assert call(cr, None, ocap=-1) == A and call(None, None, ocap=-1) == A
    assert host(cr, sp) == (A, A) and host(cr, None, n=-1) == (A, A) and host(None, sp, ocap=-1) == (A, A)
    assert csr(cr, off=None) == A and csr(off=None) == A and csr(cr, out=None) == A and csr(out=None) == A
    assert csr(cr, out_off=None) == A and csr(sp, tot=None) == A
    assert known(cr, end=-1) == A and known(longest=-1) == A
    assert pitch(cr, stride=0) == A and pitch(stride=8, length=9) == A
    # the same-length form of a batch whose region the host knows: a capacity that is too small is refused at once
    assert known(end=5, ocap=4) == CAPACITY and pitch(stride=8, length=8, n=2, ocap=15) == CAPACITY

    def s_csr(flags, n=1, off=FAKE, rows=FAKE):
        return lib.mrx_strip_dev(None, flags, FAKE, off, n, rows, FAKE, None)

    def s_known(flags, n=1, end=4, longest=4):
        return lib.mrx_strip_known_dev(None, flags, FAKE, FAKE, n, end, longest, FAKE, FAKE, None)

    def s_pitch(flags, n=1, stride=8, length=8):
        return lib.mrx_strip_strided_dev(None, flags, FAKE, stride, None, length, n, FAKE, FAKE, None)

    def s_host(flags, n=1):
        d, o = M.pack_texts([b" a "])
        rows = np.zeros(2, np.int32)
        args = (None, flags, d.ctypes.data, o.ctypes.data, n, rows.ctypes.data, None)
        return lib.mrx_strip_batch(*args), lib.mrx_debug_strip_host(*args)

    for call in (s_csr, s_known, s_pitch):
        assert call(0) == A and b"MRX_STRIP_LEFT" in lib.mrx_last_error()   # neither side
        assert call(4) == A and call(L | R | 8) == A                        # a flag bit that does not exist
        assert call(L, n=-1) == A
    assert s_host(0) == (A, A) and s_host(4) == (A, A) and s_host(L, n=-1) == (A, A)
    assert s_csr(L, off=None) == A and s_csr(L, rows=None) == A and s_csr(R, rows=FAKE + 4) == A
    assert s_known(L, end=-1) == A and s_known(R, longest=-1) == A
    assert s_pitch(L, stride=0) == A and s_pitch(L, stride=8, length=9) == A
    assert lib.mrx_debug_translate_syncs() == syncs   # nothing reached the device
    with pytest.raises(M.MrxError):
        M.api._translate_args(b"abc", b"", b"")       # a table that is not 256 bytes
    with pytest.raises(M.MrxError):
        M.api._translate_args(None, b"\r", b" ")
    with pytest.raises(M.MrxError):
        M.translate_texts([b"a"], delete=b"a", squeeze=b"b")
    with pytest.raises(M.MrxError):
        M.strip_texts([b"a"], left=False, right=False)
