"""format without a GPU: the per-cell formatter of the library (mrx_testing_format_one, the code the kernels run) against
the expectation helper (tests/format_expect.py) on the listed edges and on generated doubles, the helper itself against
Python's own % wherever it answers, the new names, the C ABI's argument errors, all of which return before any device
call, and the Python wrapper's spec errors."""
import ctypes as C

import numpy as np
import pytest

import mojo_regex_amd as M
import format_expect as F

FAKE = 1 << 40   # a device pointer that is never dereferenced
A = M.api.MRX_E_ARGUMENT


def _one(lib, out, kind, arg, word):
    r = lib.mrx_testing_format_one(kind, arg, word, C.cast(out, C.c_void_p))
    return bytes(out[:r]) if r >= 0 else r


def test_integer_cells_are_pythons_on_every_edge():
    lib, out = M.load_library(), (C.c_uint8 * 32)()
    cells = 0
    for spec in F.INT_SPECS:
        kind, arg = F.spec_kind(spec)
        for v in F.int_edges():
            want = (b"%" + spec.encode()) % v
            assert F.cell(spec, v) == want
            assert _one(lib, out, kind, arg, v) == want, (spec, v)
            cells += 1
    assert cells > 2000
    assert _one(lib, out, F.INT10, 0, F.INT64_MIN) == b"-9223372036854775808"
    assert _one(lib, out, F.INT10, 20, F.INT64_MIN) == b"-09223372036854775808" and len(b"-09223372036854775808") == 21
    assert _one(lib, out, F.INT16, 0, -255) == b"-ff" and _one(lib, out, F.INT16, 0, F.INT64_MIN) == b"-8000000000000000"
    assert _one(lib, out, F.INT16, 20, F.INT64_MAX) == b"00007fffffffffffffff"
    assert _one(lib, out, F.INT10, 0, 0) == b"0" and _one(lib, out, F.INT10, 1, 0) == b"0"   # K = 0 is read as 1
    # what the entry point refuses, the hook refuses
    for kind, arg in ((F.TEXT, 0), (4, 0), (-1, 0), (F.INT10, 21), (F.INT10, -1), (F.INT16, 21), (F.FIXED, 10), (F.FIXED, -1)):
        assert _one(lib, out, kind, arg, 5) == -F.MALFORMED
    assert lib.mrx_testing_format_one(F.INT10, 0, 5, None) == -F.MALFORMED


def test_fixed_cells_are_the_rules_on_edges_and_generated_doubles():
    lib, out = M.load_library(), (C.c_uint8 * 32)()
    values = F.fixed_edges() + F.fixed_random(12000, 11)
    answered = refused = 0
    for P in F.FIXED_PRECISIONS:
        spec = ".%df" % P
        for v in values:
            want = F.cell(spec, v)
            got = _one(lib, out, F.FIXED, P, F.float_bits(v))
            if want is None:
                assert got == -F.RANGE, (P, v, got)
                refused += 1
            else:
                assert got == want, (P, v, got, want)
                assert want == (b"%" + spec.encode()) % v, (P, v)      # the expectation itself is Python's
                assert len(want) <= 21
                answered += 1
    assert answered + refused >= 100000 and answered > 50000 and refused > 10000
    for spec, v, want in ((".0f", 0.5, b"0"), (".0f", 2.5, b"2"), (".0f", 1.5, b"2"), (".2f", 0.125, b"0.12"), (".3f", -0.0, b"-0.000"),
                          (".1f", -0.04, b"-0.0"), (".0f", 7.0, b"7"), (".9f", 5e-324, b"0.000000000"), (".0f", 2.0 ** 53, b"9007199254740992")):
        assert F.cell(spec, v) == want and _one(lib, out, F.FIXED, int(spec[1]), F.float_bits(v)) == want
    for v in (float("nan"), float("inf"), float("-inf"), 1e19, -1e19, 1e300):
        assert F.cell(".0f", v) is None and _one(lib, out, F.FIXED, 0, F.float_bits(v)) == -F.RANGE
    # the doubles around 10^19 / 10^P: the last one below is answered with 19 digits, the bound itself is not
    for P in F.FIXED_PRECISIONS:
        bound = 10.0 ** (19 - P)
        below = F.bits_float(F.float_bits(bound) - 1)
        assert F.cell(".%df" % P, bound) is None
        got = F.cell(".%df" % P, below)
        assert got is not None and len(got) == 19 + (P > 0) and got == b"%.*f" % (P, below)


def test_the_expectation_of_records():
    recs, st = F.records(rb"\2 \1" + b"\n", [[b"ab", b"", b"c"], ([7, -1, 0], "d")])
    assert recs == [b"7 ab\n", b"-1 \n", b"0 c\n"] and st.tolist() == [0, 0, 0]
    recs, st = F.records(rb"\1|\1|\3|\9\0\\", [([1.5, float("nan")], ".0f"), [b"x", b"y"], ([3, 4], ".2x", [F.MALFORMED, F.OK])])
    assert recs == [b"2|2||\\0\\\\", b"||04|\\0\\\\"] and st.tolist() == [F.MALFORMED, F.RANGE]
    assert F.records(b"", [[b"a"]])[0] == [b""] and F.records(b"lit\\", [[b"a"]])[0] == [b"lit\\"]
    assert F.packed([b"ab", b"", b"c"])[1].tolist() == [0, 2, 2, 3]


SYMBOLS = ("mrx_format_dev", "mrx_format_batch")


def test_names_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    for name in ("mrx_debug_format_grid", "mrx_testing_format_one"):
        assert name in M.api.TESTING_SYMBOLS and getattr(lib, name) is not None
    assert callable(M.format_records) and callable(M.format_numbers) and callable(M.format_records_async)
    assert (M.api.MRX_COL_TEXT, M.api.MRX_COL_INT10, M.api.MRX_COL_INT16, M.api.MRX_COL_FIXED) == (F.TEXT, F.INT10, F.INT16, F.FIXED)
    hdr = open(M.api.os.path.join(M.api.os.path.dirname(M.api._HERE), "include", "mrx.h")).read()
    for word in ("MRX_COL_TEXT = 0", "MRX_COL_INT10 = 1", "MRX_COL_INT16 = 2", "MRX_COL_FIXED = 3", "typedef struct mrx_column"):
        assert word in hdr
    assert C.sizeof(M.api._Column) == 56


def _cols(*specs):
    """An mrx_column array with fake device pointers: "t" = a CSR text column, "s" = one at a fixed pitch of 64, else a
    number spec."""
    arr = (M.api._Column * max(len(specs), 1))()
    for c, spec in zip(arr, specs):
        c.d_values = FAKE
        if spec == "t":
            c.kind, c.d_offsets = F.TEXT, FAKE
        elif spec == "s":
            c.kind, c.stride, c.len = F.TEXT, 64, 64
        else:
            c.kind, c.arg = F.spec_kind(spec)
    return arr


def test_device_entry_point_argument_errors():
    lib = M.load_library()
    tot = (C.c_int64 * 2)(-7, -7)
    tp = C.cast(tot, C.c_void_p)

    def call(arr, ncols=None, tpl=rb"\1", tpl_len=None, n=10, off=FAKE, data=FAKE, cap=100, rs=FAKE, dt=FAKE):
        return lib.mrx_format_dev(tpl, len(tpl or b"") if tpl_len is None else tpl_len, C.cast(arr, C.c_void_p) if arr is not None else None,
                                  len(arr) if ncols is None else ncols, n, off, data, cap, rs, dt, tp, None)
    good = _cols("t", "d", ".3f", "s")
    assert call(good, n=-1) == A and call(good, cap=-1) == A                         # negative n, out_cap
    assert call(good, ncols=0) == A and call(_cols(*["d"] * 10), ncols=10) == A      # ncols outside 1..9
    assert b"ncols" in lib.mrx_last_error()
    assert call(None, ncols=1) == A                                                  # null cols
    assert call(good, tpl=None, tpl_len=3) == A                                      # null template of nonzero length
    assert call(good, off=None) == A and call(good, dt=None) == A and call(good, data=None) == A
    for kind in (4, -1, 99):                                                         # an unknown kind
        bad = _cols("d")
        bad[0].kind = kind
        assert call(bad) == A
        assert b"kind" in lib.mrx_last_error()
    for spec, arg in (("d", 21), ("d", -1), ("x", 21), ("x", -1), (".0f", 10), (".0f", -1)):   # K, P out of range
        bad = _cols("t", spec)
        bad[1].arg = arg
        assert call(bad) == A
    for fix in (dict(stride=0), dict(stride=-8), dict(len=65), dict(len=-1)):        # a text column with a bad pitch
        bad = _cols("d", "s")
        for k, v in fix.items():
            setattr(bad[1], k, v)
        assert call(bad) == A
    for j in range(4):                                                               # a column's values or data, n > 0
        bad = _cols("t", "d", ".3f", "s")
        bad[j].d_values = None
        assert call(bad) == A
        assert b"null" in lib.mrx_last_error()
    # a column that the template does not name is checked all the same
    bad = _cols("d", "d")
    bad[1].arg = 30
    assert call(bad, tpl=rb"\1") == A
    assert list(tot) == [-7, -7]
    assert lib.mrx_debug_scratch_in_use() == 0


def test_host_entry_point_argument_errors():
    lib = M.load_library()
    data, off = M.pack_texts([b"ab", b"c"])
    vals, st = np.array([1, 2], np.int64), np.zeros(2, np.uint8)
    out_off, out, rs, tot = np.full(3, -5, np.int64), np.full(64, 0xEE, np.uint8), np.full(2, 9, np.uint8), np.full(2, -7, np.int64)

    def cols(data_p=data.ctypes.data, off_p=off.ctypes.data, vals_p=vals.ctypes.data, arg=0, kind=F.INT10):
        arr = (M.api._Column * 2)()
        arr[0].kind, arr[0].d_values, arr[0].d_offsets = F.TEXT, data_p, off_p
        arr[1].kind, arr[1].arg, arr[1].d_values, arr[1].d_status = kind, arg, vals_p, st.ctypes.data
        return arr

    def call(arr, ncols=2, n=2, tpl=rb"\1 \2", oo=out_off.ctypes.data, od=out.ctypes.data, cap=64):
        return lib.mrx_format_batch(tpl, len(tpl), C.cast(arr, C.c_void_p) if arr is not None else None, ncols, n, oo, od, cap,
                                    rs.ctypes.data, tot.ctypes.data)
    assert call(cols(), n=-1) == A and call(cols(), cap=-1) == A
    assert call(cols(), ncols=0) == A and call(cols(), ncols=10) == A and call(None) == A
    assert call(cols(), oo=None) == A and call(cols(), od=None) == A
    assert call(cols(kind=7)) == A and call(cols(arg=21)) == A and call(cols(kind=F.FIXED, arg=10)) == A
    assert call(cols(data_p=None)) == A and call(cols(vals_p=None)) == A
    bad = np.array([4, 2, 0], np.int64)
    assert call(cols(off_p=bad.ctypes.data)) == A                                    # offsets that decrease
    assert b"decrease" in lib.mrx_last_error()
    assert out_off.tolist() == [-5] * 3 and np.all(out == 0xEE) and rs.tolist() == [9, 9] and tot.tolist() == [-7, -7]


def test_python_spec_errors():
    import torch
    i64, f64 = torch.arange(3, dtype=torch.int64), torch.zeros(3, dtype=torch.float64)
    st = torch.zeros(3, dtype=torch.uint8)
    bad = [
        lambda: M.format_records(rb"\1", [(i64, "q")]),                    # an unknown letter
        lambda: M.format_records(rb"\1", [(i64, "f")]),
        lambda: M.format_records(rb"\1", [(i64, "%d")]),
        lambda: M.format_records(rb"\1", [(i64, ".21d")]),                 # K, P out of range
        lambda: M.format_records(rb"\1", [(i64, ".21x")]),
        lambda: M.format_records(rb"\1", [(f64, ".10f")]),
        lambda: M.format_records(rb"\1", [(i64, ".2f")]),                  # a dtype that does not fit the spec
        lambda: M.format_records(rb"\1", [(f64, "d")]),
        lambda: M.format_records(rb"\1", [f64]),                           # float64 needs a spec
        lambda: M.format_records(rb"\1", [i64.to(torch.int32)]),
        lambda: M.format_records(rb"\1", [i64, (torch.arange(4, dtype=torch.int64), "x")]),   # different row counts
        lambda: M.format_records(rb"\1", [(i64, "d", st[:2])]),
        lambda: M.format_records(rb"\1", [(i64, "d", st.to(torch.int32))]),
        lambda: M.format_records(rb"\1", []),                              # 1 to 9 columns
        lambda: M.format_records(rb"\1", [i64] * 10),
        lambda: M.format_records(rb"\1", [i64, [1, 2, 3]]),                # device and host columns mixed
        lambda: M.format_records(rb"\1", [[1, 2], [b"a"]]),                # host lists of different lengths
        lambda: M.format_records(rb"\1", [([1.5], "d")]),
        lambda: M.format_records(rb"\1", [[1.5]]),
        lambda: M.format_records(rb"\1", [([1], ".99d")]),
        lambda: M.format_records(rb"\1", [([1 << 64], "d")]),
        lambda: M.format_numbers([1, 2], spec="g"),
        lambda: M.format_numbers(f64, spec="x"),
        lambda: M.format_records_async(rb"\1", [(i64, "z")], None),
    ]
    for call in bad:
        with pytest.raises(M.MrxError):
            call()
    assert M.api._fmt_spec("d") == (F.INT10, 0) and M.api._fmt_spec(".20x") == (F.INT16, 20) and M.api._fmt_spec(".0f") == (F.FIXED, 0)
    assert M.api._template_ref_list(rb"\2 \1\0\\9\9" + b"\\") == [2, 1, 9, 9] and M.api._template_refs(rb"a\1\1") == 2
