"""numbers without a GPU: the expectation helper (tests/parse_expect.py) against Python's own float() and on the listed
edges, the new names, and the C ABI's argument errors, all of which return before any device call."""
import struct

import numpy as np

import mojo_regex_amd as M
import parse_expect as P

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C


def _float_strings(n=20000, seed=5):
    rng = np.random.default_rng(seed)

    def digits(k):
        return bytes(rng.integers(48, 58, size=k).tolist())

    out = []
    for j in range(n):
        t = (b"", b"+", b"-")[int(rng.integers(0, 3))]
        ip, fp = digits(int(rng.integers(0, 9 if j % 16 else 25))), digits(int(rng.integers(0, 9 if j % 16 != 1 else 25)))
        if rng.random() < 0.3:
            ip = b"0" * int(rng.integers(0, 4)) + ip
        if rng.random() < 0.3:
            fp += b"0" * int(rng.integers(0, 25))
        if rng.random() < 0.2:
            ip += b"0" * int(rng.integers(0, 25))
        t += ip + (b"." + fp if rng.random() < 0.8 else b"")
        if rng.random() < 0.5:
            t += (b"e", b"E")[int(rng.integers(0, 2))] + (b"", b"+", b"-")[int(rng.integers(0, 3))] + str(int(rng.integers(0, 30))).encode()
        out.append(t)
    return out


def test_every_float_the_rule_answers_is_pythons_float_in_all_64_bits():
    answered = refused = 0
    for t in _float_strings() + list(P.edge_pieces()):
        st, bits = P.expect(t, "float")
        if st == P.OK:
            assert bits == P.float_bits(float(t)), t
            answered += 1
        elif st == P.RANGE:
            float(t)   # well-formed for Python too
            refused += 1
    assert answered > 8000 and refused > 1000
    assert P.expect(b"-0.0e999", "float") == (P.OK, -(1 << 63))                      # the sign bit of a zero is kept
    assert P.expect(b"0e99999999999999999999", "float") == (P.OK, 0)
    assert P.expect(b"1.5" + b"0" * 22, "float") == (P.OK, P.float_bits(1.5))
    assert P.expect(b"9007199254740992e22", "float")[0] == P.OK and P.expect(b"9007199254740992e23", "float")[0] == P.RANGE
    assert P.expect(b"0." + b"0" * 21 + b"1", "float") == (P.OK, P.float_bits(1e-22))
    assert P.expect(b"0." + b"0" * 22 + b"1", "float")[0] == P.RANGE


def test_listed_edges_have_the_listed_statuses():
    for piece, want in P.LISTED.items():
        for kind, st in zip(P.KINDS, want):
            assert P.expect(piece, kind)[0] == st, (piece, kind)
    assert P.expect(b"-0", "int") == (P.OK, 0) and P.expect(b"-0", "float") == (P.OK, -(1 << 63))
    assert P.expect(b"9223372036854775807", "int") == (P.OK, (1 << 63) - 1)
    assert P.expect(b"-9223372036854775808", "int") == (P.OK, -(1 << 63))
    assert P.expect(b"0" * 100 + b"1", "hex") == (P.OK, 1)
    assert P.expect(b"0X1f", "hex") == (P.OK, 31) and P.expect(b"-0xff", "hex") == (P.OK, -255)
    assert P.expect(b"7fffffffffffffff", "hex") == (P.OK, (1 << 63) - 1)
    assert P.expect(b"-8000000000000000", "hex") == (P.OK, -(1 << 63))
    assert P.expect(b"1e22", "float") == (P.OK, P.float_bits(1e22)) and P.expect(b"1e22", "hex") == (P.OK, 0x1e22)
    assert P.expect(b"1e-22", "float") == (P.OK, P.float_bits(1e-22))
    assert P.expect(b"9007199254740992", "float") == (P.OK, P.float_bits(2.0 ** 53))
    # a row that is not a number holds the fill word, for a float the bits of the fill
    assert P.expect(b"x", "int", fill=-7) == (P.MALFORMED, -7)
    assert P.expect(b"", "hex", fill=5) == (P.EMPTY, 5)
    assert P.expect(b"1e23", "float", fill=float("nan")) == (P.RANGE, P.float_bits(float("nan")))
    pieces = P.edge_pieces()
    assert 280 <= len(pieces) <= 330 and {len(p) for p in pieces} >= set(range(41))
    assert P.clamp_piece(b"abcdef", -3, 2) == b"ab" and P.clamp_piece(b"abcdef", 4, 99) == b"ef"
    assert P.clamp_piece(b"abcdef", 5, 2) == b"" and P.clamp_piece(b"abcdef", -1, -1) == b""
    assert P.python_value(b"12", "int") == 12 and P.python_value(b"1.5", "float") == 1.5 and P.python_value(b"", "int") is None


SYMBOLS = ("mrx_parse_dev", "mrx_parse_strided_dev", "mrx_parse_spans_dev", "mrx_parse_spans_strided_dev", "mrx_parse_batch")


def test_names_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "mrx_debug_parse_grid" in M.api.TESTING_SYMBOLS and lib.mrx_debug_parse_grid is not None
    assert callable(M.numbers) and callable(M.parse_numbers) and callable(M.CompiledRegex.numbers)
    assert callable(M.DeviceBatch.parse) and callable(M.DeviceBatch.parse_spans)
    assert (M.api.MRX_NUM_INT10, M.api.MRX_NUM_INT16, M.api.MRX_NUM_FLOAT) == (0, 1, 2)
    assert (M.api.MRX_NUM_OK, M.api.MRX_NUM_EMPTY, M.api.MRX_NUM_MALFORMED, M.api.MRX_NUM_RANGE) == (P.OK, P.EMPTY, P.MALFORMED, P.RANGE)
    hdr = open(M.api.os.path.join(M.api.os.path.dirname(M.api._HERE), "include", "mrx.h")).read()
    for word in ("MRX_NUM_INT10 = 0", "MRX_NUM_INT16 = 1", "MRX_NUM_FLOAT = 2", "MRX_NUM_OK = 0", "MRX_NUM_EMPTY = 1",
                 "MRX_NUM_MALFORMED = 2", "MRX_NUM_RANGE = 3"):
        assert word in hdr


def test_python_argument_errors():
    for call in (lambda: M.parse_numbers([b"1"], kind="octal"), lambda: M.api._num_kind("INT"),
                 lambda: M.api._num_fill("int", 1 << 63), lambda: M.api._num_fill("hex", -(1 << 63) - 1)):
        try:
            call()
        except M.MrxError:
            continue
        raise AssertionError("no MrxError")
    assert M.api._num_fill("int", -1) == -1 and M.api._num_fill("float", -0.0) == -(1 << 63)
    assert M.api._num_fill("float", 1.5) == struct.unpack("<q", struct.pack("<d", 1.5))[0]


def test_whole_text_entry_points_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    calls = (lambda n, *t: lib.mrx_parse_dev(FAKE, FAKE, n, *t, None),
             lambda n, *t: lib.mrx_parse_strided_dev(FAKE, 64, None, 64, n, *t, None))
    # (kind, fill, d_values, d_status)
    for call in calls:
        assert call(-1, 0, 0, FAKE, FAKE) == A        # negative n
        assert call(10, 3, 0, FAKE, FAKE) == A        # a kind that is none of the three
        assert b"kind" in lib.mrx_last_error()
        assert call(10, -1, 0, FAKE, FAKE) == A
        assert call(10, 0, 0, None, FAKE) == A        # null d_values
        assert call(10, 2, 0, FAKE, None) == A        # null d_status
    assert lib.mrx_parse_dev(FAKE, None, 10, 0, 0, FAKE, FAKE, None) == A                     # null d_offsets
    assert lib.mrx_parse_strided_dev(FAKE, 64, None, 65, 10, 0, 0, FAKE, FAKE, None) == A     # a length beyond the pitch
    assert lib.mrx_parse_strided_dev(FAKE, 64, None, -1, 10, 0, 0, FAKE, FAKE, None) == A
    assert lib.mrx_parse_strided_dev(FAKE, 0, None, 0, 10, 0, 0, FAKE, FAKE, None) == A       # a non-positive pitch
    assert lib.mrx_parse_strided_dev(FAKE, -8, None, 0, 10, 0, 0, FAKE, FAKE, None) == A
    assert lib.mrx_debug_scratch_in_use() == 0


def test_spans_entry_points_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    tot = (C.c_int64 * 1)(-7)
    tp = C.cast(tot, C.c_void_p)
    calls = (lambda n, *t: lib.mrx_parse_spans_dev(FAKE, FAKE, n, *t, None),
             lambda n, *t: lib.mrx_parse_spans_strided_dev(FAKE, 64, None, 64, n, *t, None))
    # (d_prefix, d_spans, row_pairs, pair, kind, fill, row_cap, d_values, d_status, d_owner, d_totals, totals)
    for call in calls:
        assert call(-1, FAKE, FAKE, 1, 0, 0, 0, 8, FAKE, FAKE, FAKE, FAKE, tp) == A     # negative n
        assert call(10, FAKE, FAKE, 1, 0, 0, 0, -1, FAKE, FAKE, FAKE, FAKE, tp) == A    # negative row_cap
        assert call(10, FAKE, FAKE, 1, 0, 3, 0, 8, FAKE, FAKE, FAKE, FAKE, tp) == A     # a bad kind
        assert call(10, FAKE, FAKE, 1, 0, -1, 0, 8, FAKE, FAKE, FAKE, FAKE, tp) == A
        assert call(10, FAKE, FAKE, 0, 0, 0, 0, 8, FAKE, FAKE, FAKE, FAKE, tp) == A     # row_pairs < 1
        assert call(10, FAKE, FAKE, 3, 3, 0, 0, 8, FAKE, FAKE, FAKE, FAKE, tp) == A     # pair outside the rows
        assert call(10, FAKE, FAKE, 3, -1, 0, 0, 8, FAKE, FAKE, FAKE, FAKE, tp) == A
        assert call(10, FAKE, FAKE + 4, 1, 0, 0, 0, 8, FAKE, FAKE, FAKE, FAKE, tp) == A  # a misaligned d_spans
        assert b"aligned" in lib.mrx_last_error()
        assert call(10, None, FAKE, 1, 0, 0, 0, 8, FAKE, FAKE, FAKE, FAKE, tp) == A     # null d_prefix
        assert call(10, FAKE, None, 1, 0, 0, 0, 8, FAKE, FAKE, FAKE, FAKE, tp) == A     # null d_spans with a capacity
        assert call(10, FAKE, FAKE, 1, 0, 0, 0, 8, None, FAKE, FAKE, FAKE, tp) == A     # null d_values
        assert call(10, FAKE, FAKE, 1, 0, 0, 0, 8, FAKE, None, FAKE, FAKE, tp) == A     # null d_status
        assert call(10, FAKE, FAKE, 1, 0, 0, 0, 8, FAKE, FAKE, None, None, tp) == A     # null d_totals (d_owner may be)
        assert call(10, FAKE, None, 1, 0, 0, 0, 0, None, None, None, None, tp) == A     # ... for no capacity too
    good = (FAKE, FAKE, 1, 0, 0, 0, 8, FAKE, FAKE, FAKE, FAKE, tp)
    assert lib.mrx_parse_spans_dev(FAKE, None, 10, *good, None) == A                          # null d_offsets
    assert lib.mrx_parse_spans_strided_dev(FAKE, 64, None, 65, 10, *good, None) == A          # a length beyond the pitch
    assert lib.mrx_parse_spans_strided_dev(FAKE, 0, None, 0, 10, *good, None) == A            # a non-positive pitch
    assert list(tot) == [-7]
    assert lib.mrx_debug_scratch_in_use() == 0


def test_host_entry_point_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    data, off = M.pack_texts([b"12", b"-7"])
    values, status = np.full(2, -5, np.int64), np.full(2, 9, np.uint8)
    d, o, v, s = data.ctypes.data, off.ctypes.data, values.ctypes.data, status.ctypes.data
    bad = np.array([4, 2, 0], np.int64)
    parse = lib.mrx_parse_batch
    assert parse(d, o, -1, 0, 0, v, s) == A
    assert parse(d, o, 2, 3, 0, v, s) == A
    assert parse(d, o, 2, -1, 0, v, s) == A
    assert parse(d, None, 2, 0, 0, v, s) == A
    assert parse(d, o, 2, 0, 0, None, s) == A
    assert parse(d, o, 2, 0, 0, v, None) == A
    assert parse(None, o, 2, 0, 0, v, s) == A                 # null data of a batch with bytes
    assert parse(d, bad.ctypes.data, 2, 0, 0, v, s) == A      # offsets that decrease
    assert values.tolist() == [-5, -5] and status.tolist() == [9, 9]
