"""format on the GPU against tests/format_expect.py, bit for bit and with nothing left out: text columns on every layout of
tests/layouts.py with digits, '-' and '.' directly around every text; row counts around a wavefront and several rounds per
wavefront; the output at every alignment between canaries; records of every length against block boundaries, number
cells cut at each of their bytes, repeated and missing references, nine columns; the host test's edge values under
every spec, status columns and the row status; the edges of the C contract in include/mrx.h (capacity, optional
pointers, scratch); and the round trips with parse, numbers, value_counts, distinct and Dictionary."""
import collections
import ctypes as C

import numpy as np
import pytest

import mojo_regex_amd as M
import format_expect as F
import layouts as LY
import parse_expect as P

pytestmark = pytest.mark.gpu

OK, CAPACITY = M.api.MRX_OK, M.api.MRX_E_CAPACITY
LENGTHS = (0, 1, 15, 16, 17, 33)


def _np(t):
    return t.cpu().numpy()


def _poison(seed=0):
    """Bytes around the texts that would change a record if they were read as part of a cell: digits, '-' and '.'."""
    rng = np.random.default_rng(4000 + seed)
    alphabet = np.frombuffer(b"0123456789-.", dtype=np.uint8)
    turn = [0]

    def pz(i, t, k):
        if k <= 0:
            return b""
        turn[0] += 1
        return bytes([alphabet[turn[0] % len(alphabet)]]) + alphabet[rng.integers(0, len(alphabet), size=k - 1)].tobytes()
    return pz


def _texts(n, seed=0, lengths=LENGTHS):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(97, 123, size=lengths[int(rng.integers(0, len(lengths)))]).tolist()) for _ in range(n)]


def _device(col):
    """A column of the expectation (a list of bytes, or (values, spec[, status])) as a device column."""
    import torch
    if not isinstance(col, tuple):
        return M.DeviceBatch.from_texts(col)
    kind = F.spec_kind(col[1])[0]
    values = torch.from_numpy(np.array(col[0], np.float64 if kind == F.FIXED else np.int64)).cuda()
    if len(col) > 2 and col[2] is not None:
        return values, col[1], torch.from_numpy(np.array(col[2], np.uint8)).cuda()
    return values, col[1]


def _check(res, want, what=None):
    """(records DeviceBatch, row status) against (records, status) of the expectation."""
    import torch
    torch.cuda.synchronize()
    records, status = res
    data, off = F.packed(want[0])
    assert np.array_equal(_np(records.offsets), off), what
    assert _np(records.data)[:len(data)].tobytes() == data and records.data.numel() == len(data), what
    assert np.array_equal(_np(status), want[1]), what
    lib = M.load_library()
    assert lib.mrx_last_kernel_name() == b"k_format_gather"
    assert lib.mrx_debug_scratch_in_use() == 0
    if records._max_len is not None:
        assert records._end_offset == len(data) and int(np.diff(off).max(initial=0)) <= records._max_len


def _both(tpl, cols, what=None):
    """format_records on device columns made from `cols`, checked against the expectation; returns the records."""
    res = M.format_records(tpl, [_device(c) for c in cols], status=True)
    _check(res, F.records(tpl, cols), what or tpl)
    return res[0]


def _raw(tpl, cols, cap, skew=0, totals=True, status=True, null_out=False, pad=4):
    """mrx_format_dev on the caller's own buffers: the output begins `skew` bytes behind a 16-byte boundary and has 48
    canary bytes behind its capacity, out_offsets and row_status have `pad` canary elements.  Returns (rc, out_offsets,
    the whole output buffer, row_status, d_totals, host totals)."""
    import torch
    arr, n, _, _, _, keep = M.api._fmt_device_columns(tpl, cols)
    buf = torch.full((16 + skew + cap + 48,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    off = torch.full((n + 1 + pad,), -9, dtype=torch.int64, device="cuda")
    rs = torch.full((n + pad,), 0xEE, dtype=torch.uint8, device="cuda")
    dt = torch.full((2,), -9, dtype=torch.int64, device="cuda")
    ht = (C.c_int64 * 2)(-7, -7)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = M.load_library().mrx_format_dev(tpl, len(tpl), C.cast(arr, C.c_void_p), len(arr), n, off.data_ptr(),
                                         None if null_out else buf[16 + skew:].data_ptr(), cap, rs.data_ptr() if status else None,
                                         dt.data_ptr(), C.cast(ht, C.c_void_p) if totals else None, stream)
    torch.cuda.synchronize()
    assert M.load_library().mrx_debug_scratch_in_use() == 0
    del keep
    return rc, _np(off), _np(buf), _np(rs), _np(dt).tolist(), list(ht)


# ---- text columns ------------------------------------------------------------------------------------------------------

def test_text_columns_on_every_layout():
    texts = _texts(70, 1) + [b""] * 3 + [b"x" * k for k in LENGTHS]
    counts = [(-1) ** i * 10 ** (i % 8) + i for i in range(len(texts))]
    tpl = rb"\1|\2;\1" + b"\n"
    names = set()
    for lay in LY.layouts_for(texts, _poison()):
        names.add(lay.name)
        batch = lay.device()
        want = F.records(tpl, [lay.texts, (counts, "d")])
        res = M.format_records(tpl, [batch, _device((counts, "d"))[0]], status=True)
        _check(res, want, lay.name)
        longest = batch.longest()
        if longest is None:
            assert res[0]._max_len is None
        else:
            assert res[0]._max_len == len(tpl) + 2 * longest + 21
    assert {"csr_packed", "csr_shift1", "csr_shift7", "csr_shift15", "rows48", "rows1001", "fixed64_len45"} <= names
    assert {len(t) for t in texts} >= set(LENGTHS)


def test_two_text_columns_of_different_layouts():
    a, b = _texts(40, 2), _texts(40, 3)
    la, lb = LY.csr_shifted(a, 7, _poison(1)), LY.ragged_rows(b, False, _poison(2))
    res = M.format_records(rb"\2=\1,\2", [la.device(), lb.device()], status=True)
    _check(res, F.records(rb"\2=\1,\2", [a, b]))


# ---- row counts ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130, 255, 257])
def test_row_counts(n):
    texts = _texts(n, 10 + n)
    vals = [(7919 * i * i - 50000) * (1 if i % 3 else -1) for i in range(n)]
    _both(rb"\2 \1" + b"\n", [texts, (vals, "d")], n)
    assert M.format_records(rb"\2 \1" + b"\n", [texts, vals]) == [b"%d %s\n" % (v, t) for t, v in zip(texts, vals)]


def test_one_wavefront_runs_several_rounds():
    lib = M.load_library()
    n = 700
    texts = _texts(n, 5)
    vals = [i * 104729 - 3 for i in range(n)]
    fl = [i / 8.0 - 20 for i in range(n)]
    lib.mrx_debug_format_grid(1)
    try:
        rec = _both(rb"\1 \2 \3 \2" + b"\n", [texts, (vals, ".3x"), (fl, ".2f")])
        assert rec.data.numel() > 4 * 64 * 16 * 2      # more than two rounds of 64 blocks for each of the 4 wavefronts
    finally:
        lib.mrx_debug_format_grid(0)
    _both(rb"\1 \2 \3 \2" + b"\n", [texts, (vals, ".3x"), (fl, ".2f")])


# ---- output alignment ------------------------------------------------------------------------------------------------------

def test_output_at_every_alignment_between_canaries():
    n = 90
    texts = _texts(n, 6)
    vals = [(-3) ** (i % 39) for i in range(n)]
    st = [F.OK if i % 11 else F.MALFORMED for i in range(n)]
    tpl = rb"<\1:\2>"
    cols = [texts, (vals, ".4d", st)]
    dcols = [_device(c) for c in cols]
    recs, status = F.records(tpl, cols)
    data, off = F.packed(recs)
    nbytes = len(data)
    for skew in range(16):
        for cap in (nbytes, nbytes + 29):
            rc, goff, buf, rs, dt, ht = _raw(tpl, dcols, cap, skew)
            assert rc == OK and dt == [n, nbytes] and ht == dt, (skew, cap)
            assert np.all(buf[:16 + skew] == 0xA5) and np.all(buf[16 + skew + nbytes:] == 0xA5), (skew, cap)
            assert buf[16 + skew:16 + skew + nbytes].tobytes() == data, (skew, cap)
            assert np.array_equal(goff[:n + 1], off) and np.all(goff[n + 1:] == -9)
            assert np.array_equal(rs[:n], status) and np.all(rs[n:] == 0xEE)


# ---- records -----------------------------------------------------------------------------------------------------------------

def test_record_lengths_and_runs_of_empty_records():
    rng = np.random.default_rng(7)
    lens = [0, 1, 15, 16, 17, 40] * 6 + [0] * 70 + [40, 1] + [0] * 130 + [16, 0, 0, 17] + [0] * 65
    texts = [bytes(rng.integers(97, 123, size=k).tolist()) for k in lens]
    rec = _both(rb"\1", [texts])
    assert sorted(set(np.diff(_np(rec.offsets)).tolist())) == [0, 1, 15, 16, 17, 40]
    # the same lengths from a literal, a number and a text: 40 = 3 + 21 + 16
    vals = [F.INT64_MIN + i for i in range(len(texts))]
    st = [F.OK if k == 40 else F.EMPTY for k in lens]
    cut = [t[:16] if k == 40 else t for t, k in zip(texts, lens)]
    mixed = F.records(rb"\3\2\1", [cut, (vals, ".20d", st), [b"abc" if k == 40 else b"" for k in lens]])
    assert sorted(set(len(r) for r in mixed[0])) == [0, 1, 15, 16, 17, 40]
    _both(rb"\3\2\1", [cut, (vals, ".20d", st), [b"abc" if k == 40 else b"" for k in lens]])


def test_number_cells_cut_by_a_block_boundary_at_each_byte():
    n = 400
    texts = [b"t" * (i % 16) for i in range(n)]
    ints = [-(10 ** 18) - i for i in range(n)]
    hexs = [-(1 << 62) - i for i in range(n)]
    fl = [-(10.0 ** 9) - i - 0.5 for i in range(n)]
    for tpl, col, width in ((rb"\1\2", (ints, ".20d"), 21), (rb"\1\2", (hexs, ".20x"), 21), (rb"\1\2", (fl, ".9f"), 21)):
        recs, _ = F.records(tpl, [texts, col])
        _, off = F.packed(recs)
        assert all(len(r) == len(t) + width for r, t in zip(recs, texts))
        starts = {int(off[i] + len(texts[i])) % 16 for i in range(n)}
        assert starts == set(range(16))      # so a boundary falls behind each of the cell's first 20 bytes
        _both(tpl, [texts, col], tpl)
    _both(rb"\2\1\3|\4", [texts, (ints, "d"), (hexs, "x"), (fl, ".3f")])


def test_references_repeated_missing_and_none():
    n = 150
    texts, vals = _texts(n, 8), [i * i * 31 - 999 for i in range(n)]
    cols = [texts, (vals, "d")]
    for tpl in (rb"\2\2 \1 \2", rb"\1\7\9x", rb"\3\4", b"", b"lit", rb"\0\\" + b"\\", rb"a\\1b", b"no reference at all, forty bytes long.."):
        rec = _both(tpl, cols, tpl)
        if tpl in (b"", rb"\3\4"):
            assert rec.data.numel() == 0 and not _np(rec.offsets).any()
    assert M.format_records(rb"\2\2 \1", [[b"a", b"b"], [1, None]], status=True)[0] == [b"11 a", b" b"]


def test_nine_columns():
    n = 120
    rng = np.random.default_rng(9)
    cols = [_texts(n, 20), (rng.integers(-10 ** 6, 10 ** 6, size=n).tolist(), "d"), (rng.integers(0, 1 << 40, size=n).tolist(), ".12x"),
            (rng.normal(0, 1000, size=n).tolist(), ".3f"), _texts(n, 21, (0, 2, 5)), (rng.integers(-99, 99, size=n).tolist(), ".5d"),
            ((rng.integers(-10 ** 9, 10 ** 9, size=n) / 4.0).tolist(), ".0f"), _texts(n, 22, (1, 16)),
            (rng.integers(-(1 << 62), 1 << 62, size=n).tolist(), "x")]
    _both(rb"\9\8\7\6\5\4\3\2\1|\5", cols)
    _both(rb"\1,\2,\3,\4,\5,\6,\7,\8,\9" + b"\n", cols)


# ---- number columns --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", F.INT_SPECS)
def test_integer_edges(spec):
    vals = F.int_edges()
    rec = _both(rb"\1,", [(vals, spec)], spec)
    assert _np(rec.data).tobytes() == b"".join((b"%" + spec.encode()) % v + b"," for v in vals)


@pytest.mark.parametrize("P", F.FIXED_PRECISIONS)
def test_fixed_edges(P):
    import torch
    vals = F.fixed_edges() + F.fixed_random(600, 30 + P)
    spec = ".%df" % P
    bits = torch.from_numpy(np.array([F.float_bits(v) for v in vals], np.int64)).cuda()      # (NaN payloads as they are)
    res = M.format_records(rb"\1;", [(bits.view(torch.float64), spec)], status=True)
    want = F.records(rb"\1;", [(vals, spec)])
    _check(res, want, spec)
    assert {F.OK, F.RANGE} == set(want[1].tolist())
    answered = [v for v, s in zip(vals, want[1]) if s == F.OK]
    assert b"".join(want[0]) == b"".join(((b"%" + spec.encode()) % v + b";") if s == F.OK else b";" for v, s in zip(vals, want[1]))
    assert len(answered) > 300


def test_status_columns_and_the_row_status():
    n = 200
    rng = np.random.default_rng(12)
    a, b, c = (rng.integers(-1000, 1000, size=n).tolist() for _ in range(3))
    fl = [1e19 if i % 5 == 0 else i / 4.0 for i in range(n)]
    sa = rng.choice([F.OK, F.EMPTY, F.MALFORMED, F.RANGE], size=n, p=[0.55, 0.15, 0.15, 0.15]).tolist()
    sb = rng.choice([F.OK, F.EMPTY, F.MALFORMED, F.RANGE], size=n, p=[0.55, 0.15, 0.15, 0.15]).tolist()
    sc = rng.choice([F.OK, 7, 255], size=n, p=[0.6, 0.2, 0.2]).tolist()      # any byte that is not OK, passed on as it is
    a = [-77777 if s else v for v, s in zip(a, sa)]                           # (a fill word: never printed)
    cols = [(a, "d", sa), (b, ".3x", sb), (fl, ".1f"), (c, "d", sc)]
    for tpl in (rb"\1 \2 \3 \4", rb"\4|\3|\2", rb"\3\3", rb"\2", rb"x\4\1", b"none"):
        want = F.records(tpl, cols)
        _both(tpl, cols, tpl)
        if tpl == rb"\1 \2 \3 \4":
            assert set(want[1].tolist()) >= {F.OK, F.EMPTY, F.MALFORMED, F.RANGE}
            both = [i for i in range(n) if sa[i] and sb[i] and sa[i] != sb[i]]
            assert both and all(want[1][i] == sa[i] for i in both)       # several failing columns: the lowest-numbered one
        if tpl == rb"\4|\3|\2":
            assert {7, 255} <= set(want[1].tolist())
            late = [i for i in range(n) if sb[i] and sc[i]]
            assert late and all(want[1][i] == sb[i] for i in late)       # ... by column number, not by place in the template
    assert b"77777" not in b"".join(F.records(rb"\1", cols)[0])


# ---- the contract ------------------------------------------------------------------------------------------------------------

def test_capacity_totals_and_optional_pointers():
    n = 130
    texts, vals = _texts(n, 13), [i * 1000003 for i in range(n)]
    tpl = rb"\1\2" + b"\n"
    cols = [texts, (vals, "d")]
    dcols = [_device(c) for c in cols]
    recs, status = F.records(tpl, cols)
    data, off = F.packed(recs)
    nbytes = len(data)
    # one byte short: offsets, status and totals complete, no byte written, MRX_E_CAPACITY
    rc, goff, buf, rs, dt, ht = _raw(tpl, dcols, nbytes - 1, 5)
    assert rc == CAPACITY and dt == [n, nbytes] and ht == dt
    assert np.all(buf == 0xA5) and np.array_equal(goff[:n + 1], off) and np.array_equal(rs[:n], status)
    assert b"need %d" % nbytes in M.load_library().mrx_last_error()
    # ... and without totals the call cannot know: MRX_OK, the same device state
    rc, goff, buf, rs, dt, ht = _raw(tpl, dcols, nbytes - 1, 5, totals=False)
    assert rc == OK and dt == [n, nbytes] and ht == [-7, -7] and np.all(buf == 0xA5) and np.array_equal(goff[:n + 1], off)
    # totals == NULL with room
    rc, goff, buf, rs, dt, ht = _raw(tpl, dcols, nbytes, 3, totals=False)
    assert rc == OK and dt == [n, nbytes] and ht == [-7, -7] and buf[19:19 + nbytes].tobytes() == data
    # out_cap == 0 with a null d_out_data
    rc, goff, buf, rs, dt, ht = _raw(tpl, dcols, 0, 0, null_out=True)
    assert rc == CAPACITY and dt == [n, nbytes] and np.array_equal(goff[:n + 1], off) and np.all(buf == 0xA5)
    rc, goff, buf, rs, dt, ht = _raw(b"", dcols, 0, 0, null_out=True)
    assert rc == OK and dt == [n, 0] and not goff[:n + 1].any() and np.all(goff[n + 1:] == -9)
    # d_row_status == NULL
    rc, goff, buf, rs, dt, ht = _raw(tpl, dcols, nbytes, 9, status=False)
    assert rc == OK and np.all(rs == 0xEE) and buf[25:25 + nbytes].tobytes() == data
    # no rows
    rc, goff, buf, rs, dt, ht = _raw(tpl, [_device([]), _device(([], "d"))], 8, 0)
    assert rc == OK and dt == [0, 0] and ht == [0, 0] and goff[0] == 0 and np.all(goff[1:] == -9) and np.all(buf == 0xA5)
    assert M.load_library().mrx_last_kernel_name() == b"k_format_gather"


def test_python_capacities_and_the_async_form():
    import torch
    n = 300
    texts, vals = _texts(n, 14), [i - 150 for i in range(n)]
    tpl = rb"\2:\1"
    cols = [texts, (vals, "d")]
    recs, _ = F.records(tpl, cols)
    data, off = F.packed(recs)
    dcols = [_device(c) for c in cols]
    with pytest.raises(M.MrxError):
        M.format_records(tpl, dcols, out_cap=len(data) - 1)
    assert M.load_library().mrx_debug_scratch_in_use() == 0
    rec = M.format_records(tpl, dcols, out_cap=len(data))
    assert _np(rec.data).tobytes() == data
    # a text column that does not know its longest text: the first capacity is an estimate (12 bytes a number), and the
    # call grows to what the 21-byte cells need
    plain = M.DeviceBatch(dcols[0].data, dcols[0].offsets)
    wide = F.records(rb"\1\2\2\2", [texts, (vals, ".20d")])[0]
    rec = M.format_records(rb"\1\2\2\2", [plain, (dcols[1][0], ".20d")])
    assert rec._max_len is None and _np(rec.data).tobytes() == b"".join(wide)
    assert len(b"".join(wide)) > 8 * n + len(b"".join(texts)) + 3 * 12 * n      # (the estimate)
    out = (torch.full((n + 1,), -9, dtype=torch.int64, device="cuda"), torch.full((len(data) + 7,), 0xA5, dtype=torch.uint8, device="cuda"),
           torch.full((2,), -9, dtype=torch.int64, device="cuda"), torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda"))
    M.format_records_async(tpl, dcols, out)
    torch.cuda.synchronize()
    assert _np(out[2]).tolist() == [n, len(data)] and np.array_equal(_np(out[0]), off) and not _np(out[3]).any()
    assert _np(out[1])[:len(data)].tobytes() == data and np.all(_np(out[1])[len(data):] == 0xA5)
    M.format_records_async(tpl, dcols, out[:3])


def test_host_buffer_entry_point():
    lib = M.load_library()
    texts, vals, fl = [b"ab", b"", b"xyz" * 9], np.array([5, -17, 1 << 40], np.int64), np.array([0.125, float("inf"), -2.5])
    st = np.array([F.OK, F.MALFORMED, F.OK], np.uint8)
    data, off = M.pack_texts(texts)
    arr = (M.api._Column * 3)()
    arr[0].kind, arr[0].d_values, arr[0].d_offsets = F.TEXT, data.ctypes.data, off.ctypes.data
    arr[1].kind, arr[1].arg, arr[1].d_values, arr[1].d_status = F.INT10, 3, vals.ctypes.data, st.ctypes.data
    arr[2].kind, arr[2].arg, arr[2].d_values = F.FIXED, 2, fl.ctypes.data
    tpl = rb"\1 \2 \3" + b"\n"
    want = F.records(tpl, [texts, (vals.tolist(), ".3d", st.tolist()), (fl.tolist(), ".2f")])
    wdata, woff = F.packed(want[0])
    for cap in (len(wdata), len(wdata) - 1):
        out_off, out, rs, tot = np.full(4, -5, np.int64), np.full(len(wdata) + 8, 0xEE, np.uint8), np.full(3, 9, np.uint8), np.zeros(2, np.int64)
        rc = lib.mrx_format_batch(tpl, len(tpl), C.cast(arr, C.c_void_p), 3, 3, out_off.ctypes.data, out.ctypes.data, cap,
                                  rs.ctypes.data, tot.ctypes.data)
        assert rc == (OK if cap == len(wdata) else CAPACITY)
        assert tot.tolist() == [3, len(wdata)] and np.array_equal(out_off, woff) and np.array_equal(rs, want[1])
        assert out[:len(wdata)].tobytes() == (wdata if rc == OK else b"\xee" * len(wdata)) and np.all(out[len(wdata):] == 0xEE)
    assert lib.mrx_debug_scratch_in_use() == 0


# ---- round trips and the pipeline ----------------------------------------------------------------------------------------------

def test_parse_of_format_is_the_identity():
    import torch
    vals = F.int_edges()
    v = torch.from_numpy(np.array(vals, np.int64)).cuda()
    for spec, kind in (("d", "int"), (".20d", "int"), ("x", "hex"), (".17x", "hex")):
        texts = M.format_numbers(v, spec)
        back, status = texts.parse(kind)
        torch.cuda.synchronize()
        assert torch.equal(back, v) and not _np(status).any(), spec
    assert M.format_numbers(vals[:50], "x") == [b"%x" % x for x in vals[:50]]
    assert M.format_numbers([1.5, None, -0.0], ".1f") == [b"1.5", b"", b"-0.0"]


def test_numbers_then_format_prints_the_ok_pieces_again():
    import torch
    pieces = P.edge_pieces()
    batch = M.DeviceBatch.from_texts(pieces)
    values, status = batch.parse("int", fill=-7)
    rec, row = M.format_records(rb"\1" + b"\n", [(values, "d", status)], status=True)
    torch.cuda.synchronize()
    want = []
    for p in pieces:
        st, val = P.expect(p, "int", fill=-7)
        want.append(b"%d\n" % val if st == P.OK else b"\n")
    assert _np(rec.data).tobytes() == b"".join(want)
    assert np.array_equal(_np(row), _np(status)) and len(set(_np(row).tolist())) == 4
    assert sum(w != b"\n" for w in want) > 20


def test_value_counts_report_and_the_records_as_a_batch():
    import torch
    rng = np.random.default_rng(15)
    words = [b"alpha", b"be", b"gamma", b"d", b"epsilon", b"zeta", b"eta", b"theta"]
    texts = [b" ".join(words[int(k)] for k in rng.zipf(1.6, size=int(rng.integers(0, 9))) % len(words)) for _ in range(400)]
    batch = M.DeviceBatch.from_texts(texts)
    rx = M.compile_regex(rb"[a-z]+")
    values, counts = rx.value_counts(batch, sort="count", top=5)
    report = M.format_records(rb"\2 \1" + b"\n", [values, counts])
    torch.cuda.synchronize()
    counter = collections.Counter(w for t in texts for w in t.split())
    assert _np(report.data).tobytes() == b"".join(b"%d %s\n" % (c, w) for w, c in counter.most_common(5))
    # composite keys: the records are a batch like any other
    keys = M.format_records(rb"\1/\2", [M.DeviceBatch.from_texts([t[:3] for t in texts]), torch.arange(len(texts), device="cuda") % 3])
    host = [b"%s/%d" % (t[:3], i % 3) for i, t in enumerate(texts)]
    uniq, cnt, _, _ = keys.distinct()
    torch.cuda.synchronize()
    want = collections.Counter(host)
    raw, off = _np(uniq.data).tobytes(), _np(uniq.offsets)
    assert [(raw[off[g]:off[g + 1]], int(c)) for g, c in enumerate(_np(cnt))] == list(want.items())
    d = M.Dictionary(keys)
    assert len(d) == len(host)
    probe = d.lookup(M.DeviceBatch.from_texts([host[7], b"nothing/9", host[0]]))
    assert _np(probe).tolist() == [host.index(host[7]), -1, 0]
    assert M.load_library().mrx_debug_scratch_in_use() == 0
