"""numbers on the GPU against tests/parse_expect.py, bit for bit and with nothing left out: the edge pieces under all three
kinds on every layout of tests/layouts.py, with digits, signs, '.', 'e', 'x' and 'f' directly around every text; spans
built in numpy (sub-ranges, spans that leave their text, reversed and unset ones, every pair of rows of 1 and 3 pairs,
texts without rows, row counts around a wavefront, several rounds per wavefront); the edges of the C contract in
include/mrx.h (canaries, capacities, optional pointers, no text, the fill word, scratch); and CompiledRegex.numbers
against the oracle's spans.  Float values are compared as int64 views, so the sign of a zero is checked."""
import ctypes as C

import numpy as np
import pytest

import mojo_regex_amd as M
import captures_all_expect as CA
import extract_expect as X
import layouts as LY
import parse_expect as P

pytestmark = pytest.mark.gpu

FILL = {"int": -7, "hex": 1 << 62, "float": float("nan")}
KIND_CODE = {"int": 0, "hex": 1, "float": 2}


def _np(t):
    return t.cpu().numpy()


def _bits(values):
    """values as an int64 numpy array, whatever the kind."""
    import torch
    return _np(values.view(torch.int64))


def _poison(seed=0):
    """Bytes around the texts that would change an answer if they were read as part of one: digits, signs, '.', 'e', 'x'
    and 'f', each of them in turn directly behind a text (and so in front of the next one)."""
    rng = np.random.default_rng(3000 + seed)
    alphabet = np.frombuffer(b"0123456789+-.exf", dtype=np.uint8)
    turn = [0]

    def pz(i, t, k):
        if k <= 0:
            return b""
        turn[0] += 1
        return bytes([alphabet[turn[0] % len(alphabet)]]) + alphabet[rng.integers(0, len(alphabet), size=k - 1)].tobytes()
    return pz


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def edge_layouts():
    texts = P.edge_pieces()
    lays = LY.layouts_for(texts, _poison())
    return [(lay, {k: P.expect_many(lay.texts, k, FILL[k]) for k in P.KINDS}) for lay in lays]


def _raw_parse(batch, kind, fill_word, pad=4):
    """The C call of the whole-text form on the caller's own buffers with `pad` canary elements behind each."""
    import torch
    dev, n = batch.data.device, batch.n
    values = torch.full((n + pad,), -9, dtype=torch.int64, device=dev)
    status = torch.full((n + pad,), 0xEE, dtype=torch.uint8, device=dev)
    rc = batch.call(M.load_library(), "mrx_parse", (), (KIND_CODE[kind], fill_word, values.data_ptr(), status.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return rc, _np(values), _np(status)


def test_edge_pieces_on_every_layout(edge_layouts):
    import torch
    lib = M.load_library()
    names, seen = set(), {k: set() for k in P.KINDS}
    for lay, want in edge_layouts:
        names.add(lay.name)
        batch = lay.device()
        for kind in P.KINDS:
            st, val = want[kind]
            values, status = batch.parse(kind, FILL[kind])
            torch.cuda.synchronize()
            assert values.dtype == (torch.float64 if kind == "float" else torch.int64) and status.dtype == torch.uint8
            assert np.array_equal(_np(status), st), (lay.name, kind, [lay.texts[i] for i in np.nonzero(_np(status) != st)[0][:5]])
            assert np.array_equal(_bits(values), val), (lay.name, kind, [lay.texts[i] for i in np.nonzero(_bits(values) != val)[0][:5]])
            assert lib.mrx_last_kernel_name() == b"k_parse"
            assert lib.mrx_debug_scratch_in_use() == 0
            seen[kind] |= set(st.tolist())
            rc, rv, rs = _raw_parse(batch, kind, P.fill_word(kind, FILL[kind]))
            assert rc == M.api.MRX_OK
            assert np.array_equal(rv[:batch.n], val) and np.all(rv[batch.n:] == -9) and len(rv) == batch.n + 4
            assert np.array_equal(rs[:batch.n], st) and np.all(rs[batch.n:] == 0xEE)
    assert {"csr_packed", "csr_shift1", "csr_shift7", "csr_shift15", "rows48", "rows1001", "fixed64_len45"} <= names
    assert all(s == {P.OK, P.EMPTY, P.MALFORMED, P.RANGE} for s in seen.values())


def test_list_form_of_whole_texts():
    pieces = P.edge_pieces()
    for kind in P.KINDS:
        got = M.parse_numbers(pieces, kind)
        want = [P.python_value(p, kind) for p in pieces]
        assert [type(v) for v in got] == [type(v) for v in want]
        assert [repr(v) for v in got] == [repr(v) for v in want], kind   # (repr: -0.0 is not 0.0)
    assert M.parse_numbers([], "int") == []
    assert M.parse_numbers(["12", b"-0x10", "1.5"], "hex") == [0x12, -16, None]


# ---- spans -------------------------------------------------------------------------------------------------------------

TOKENS = [b"12", b"-7", b"+300", b"3.5e2", b"0x1f", b"99999999999999999999", b"0", b"-0", b"1e22", b"1e23", b".5", b"7.",
          b"ff", b"9223372036854775807", b"-9223372036854775808", b"0.000001", b"1_0", b"e", b"-", b"0123456789012345678"]


def _number_texts(rng, n):
    """Texts of a few tokens separated by single bytes, some texts empty; (texts, token ranges per text)."""
    texts, ranges = [], []
    for i in range(n):
        t, rs = b"", []
        for _ in range(int(rng.integers(0, 6)) if i % 7 else 0):
            tok = TOKENS[int(rng.integers(0, len(TOKENS)))]
            rs.append((len(t), len(t) + len(tok)))
            t += tok + (b" ", b",", b"5", b"-")[int(rng.integers(0, 4))]
        texts.append(t)
        ranges.append(rs)
    return texts, ranges


def _random_rows(rng, texts, ranges, counts, row_pairs):
    """prefix int64[n + 1] and spans int32[rows, row_pairs, 2]: token ranges, random sub-ranges, spans that start before
    0 or end behind the text, reversed ones and (-1, -1)."""
    prefix = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum(counts, out=prefix[1:])
    spans = np.zeros((int(prefix[-1]), row_pairs, 2), dtype=np.int32)
    for i, t in enumerate(texts):
        L = len(t)
        for r in range(int(prefix[i]), int(prefix[i + 1])):
            for p in range(row_pairs):
                how = int(rng.integers(0, 8))
                if how <= 2 and ranges[i]:
                    s, e = ranges[i][int(rng.integers(0, len(ranges[i])))]
                elif how == 3:
                    s, e = -1, -1
                elif how == 4:
                    s, e = int(rng.integers(-5, 1)), int(rng.integers(0, L + 6))      # starts before 0, may end behind
                elif how == 5:
                    s = int(rng.integers(0, L + 1))
                    e = s + int(rng.integers(0, 40))                                  # may end behind the text
                elif how == 6:
                    e = int(rng.integers(0, L + 1))
                    s = e + int(rng.integers(1, 5))                                   # start > end
                else:
                    s = int(rng.integers(0, L + 1))
                    e = int(rng.integers(s, L + 1))
                spans[r, p] = (s, e)
    return prefix, spans


def _counts_for(rng, n, rows):
    """n row counts that add up to `rows`, with texts without rows among them."""
    counts = np.zeros(n, dtype=np.int64)
    if rows:
        at = rng.integers(0, n, size=rows)
        at[at % 5 == 0] = (at[at % 5 == 0] + 1) % n    # every fifth text stays without rows ...
        at[at % 5 == 0] = (at[at % 5 == 0] + 1) % n
        np.add.at(counts, at, 1)
    return counts


def _want_rows(texts, prefix, spans, pair, kind, fill):
    owner = np.repeat(np.arange(len(texts), dtype=np.int64), np.diff(prefix))
    pieces = [P.clamp_piece(texts[int(i)], *spans[r, pair]) for r, i in enumerate(owner)]
    st, val = P.expect_many(pieces, kind, fill)
    return st, val, owner


def _device_rows(prefix, spans, row_pairs):
    import torch
    sp = torch.from_numpy(spans.reshape(-1, 2).copy() if row_pairs == 1 else spans.copy()).cuda()
    if row_pairs == 1:
        sp = sp.reshape(-1, 2)
    return torch.from_numpy(prefix.copy()).cuda(), sp


def _assert_spans(batch, texts, prefix, spans, row_pairs, kinds=P.KINDS, where=""):
    import torch
    d_prefix, d_spans = _device_rows(prefix, spans, row_pairs)
    for pair in range(row_pairs):
        for kind in kinds:
            st, val, owner = _want_rows(texts, prefix, spans, pair, kind, FILL[kind])
            values, status, own = batch.parse_spans(d_prefix, d_spans, pair, kind, FILL[kind])
            torch.cuda.synchronize()
            assert values.numel() == len(st) == status.numel() == own.numel(), where
            assert np.array_equal(_np(status), st), (where, pair, kind)
            assert np.array_equal(_bits(values), val), (where, pair, kind)
            assert np.array_equal(_np(own), owner), (where, pair, kind)
    assert M.load_library().mrx_debug_scratch_in_use() == 0


def test_spans_of_rows_of_one_and_three_pairs_on_csr_and_fixed_pitch():
    rng = np.random.default_rng(11)
    texts, ranges = _number_texts(rng, 90)
    seen = set()
    for row_pairs in (1, 3):
        counts = rng.integers(0, 5, size=len(texts))
        counts[::9] = 0                                                   # texts without rows, the first one too
        prefix, spans = _random_rows(rng, texts, ranges, counts, row_pairs)
        seen |= set(_want_rows(texts, prefix, spans, 0, "float", 0.0)[0].tolist())
        for lay in (LY.csr_shifted(texts, 7, _poison(1)), LY.ragged_rows(texts, False, _poison(2))):
            _assert_spans(lay.device(), texts, prefix, spans, row_pairs, where=(lay.name, row_pairs))
    assert seen == {P.OK, P.EMPTY, P.MALFORMED, P.RANGE}


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65])
def test_row_counts_around_a_wavefront(rows):
    rng = np.random.default_rng(100 + rows)
    texts, ranges = _number_texts(rng, 23)
    prefix, spans = _random_rows(rng, texts, ranges, _counts_for(rng, len(texts), rows), 1)
    assert prefix[-1] == rows and (np.diff(prefix) == 0).any()
    _assert_spans(M.DeviceBatch.from_texts(texts), texts, prefix, spans, 1, where=rows)


def test_several_rounds_per_wavefront():
    lib = M.load_library()
    rng = np.random.default_rng(300)
    texts, ranges = _number_texts(rng, 70)
    prefix, spans = _random_rows(rng, texts, ranges, _counts_for(rng, len(texts), 300), 3)
    whole = P.edge_pieces()
    lib.mrx_debug_parse_grid(1)   # one workgroup: four wavefronts of 128, 128, 44 and no rows
    try:
        _assert_spans(M.DeviceBatch.from_texts(texts), texts, prefix, spans, 3, kinds=("int", "float"), where="one workgroup")
        values, status = M.DeviceBatch.from_texts(whole).parse("float", 0.0)
        st, val = P.expect_many(whole, "float", 0.0)
        assert np.array_equal(_np(status), st) and np.array_equal(_bits(values), val)
    finally:
        lib.mrx_debug_parse_grid(0)


# ---- the C contract ----------------------------------------------------------------------------------------------------

def _raw_spans(batch, d_prefix, d_spans, row_pairs, pair, kind, fill, row_cap, owner=True, totals=True, pad=4):
    """The C call on the caller's own buffers with `pad` canary elements behind each: (rc, values, status, owner,
    d_totals, host totals)."""
    import torch
    dev = batch.data.device
    values = torch.full((row_cap + pad,), -9, dtype=torch.int64, device=dev)
    status = torch.full((row_cap + pad,), 0xEE, dtype=torch.uint8, device=dev)
    own = torch.full((row_cap + pad,), -9, dtype=torch.int64, device=dev)
    dt = torch.full((1 + pad,), -9, dtype=torch.int64, device=dev)
    tot = (C.c_int64 * 2)(-7, -7)
    rc = batch.call(M.load_library(), "mrx_parse_spans", (),
                    (d_prefix.data_ptr(), d_spans.data_ptr(), row_pairs, pair, KIND_CODE[kind], fill, row_cap,
                     values.data_ptr(), status.data_ptr(), own.data_ptr() if owner else None, dt.data_ptr(),
                     C.cast(tot, C.c_void_p) if totals else None, _stream()))
    torch.cuda.synchronize()
    return rc, _np(values), _np(status), _np(own), _np(dt), list(tot)


def test_c_contract_capacities_canaries_and_optional_pointers():
    import torch
    lib = M.load_library()
    rng = np.random.default_rng(77)
    texts, ranges = _number_texts(rng, 40)
    prefix, spans = _random_rows(rng, texts, ranges, _counts_for(rng, len(texts), 150), 3)
    rows = 150
    d_prefix, d_spans = _device_rows(prefix, spans, 3)
    for lay in (LY.csr_packed(texts), LY.ragged_rows(texts, True, _poison(3))):
        batch = lay.device()
        st, val, owner = _want_rows(texts, prefix, spans, 1, "int", -7)
        assert (st != P.OK).sum() > 20 and (st == P.OK).sum() > 20
        for cap in (rows, rows + 7):                       # row_cap equal to rows, and larger
            rc, v, s, o, dt, tot = _raw_spans(batch, d_prefix, d_spans, 3, 1, "int", -7, cap)
            assert rc == M.api.MRX_OK and tot == [rows, -7] and dt.tolist() == [rows, -9, -9, -9, -9]
            assert np.array_equal(v[:rows], val) and np.all(v[rows:] == -9)
            assert np.all(v[:rows][st != P.OK] == -7)      # the fill word in every row that is not a number
            assert np.array_equal(s[:rows], st) and np.all(s[rows:] == 0xEE)
            assert np.array_equal(o[:rows], owner) and np.all(o[rows:] == -9)
        # one short: only d_totals[0] is written
        rc, v, s, o, dt, tot = _raw_spans(batch, d_prefix, d_spans, 3, 1, "int", -7, rows - 1)
        assert rc == M.api.MRX_E_CAPACITY and tot == [rows, -7] and dt.tolist() == [rows, -9, -9, -9, -9]
        assert np.all(v == -9) and np.all(s == 0xEE) and np.all(o == -9)
        rc, v, s, o, dt, tot = _raw_spans(batch, d_prefix, d_spans, 3, 1, "int", -7, rows - 1, totals=False)
        assert rc == M.api.MRX_OK and tot == [-7, -7] and dt.tolist() == [rows, -9, -9, -9, -9]
        assert np.all(v == -9) and np.all(s == 0xEE) and np.all(o == -9)
        rc, v, s, o, dt, tot = _raw_spans(batch, d_prefix, d_spans, 3, 1, "int", -7, 0)
        assert rc == M.api.MRX_E_CAPACITY and tot[0] == rows and dt[0] == rows and np.all(v == -9) and np.all(s == 0xEE)
        # d_owner NULL, totals NULL
        rc, v, s, o, dt, tot = _raw_spans(batch, d_prefix, d_spans, 3, 1, "int", -7, rows, owner=False, totals=False)
        assert rc == M.api.MRX_OK and tot == [-7, -7] and dt.tolist() == [rows, -9, -9, -9, -9]
        assert np.array_equal(v[:rows], val) and np.array_equal(s[:rows], st) and np.all(o == -9)
        # a float fill is stored verbatim
        nan = P.fill_word("float", float("nan"))
        st, val, _ = _want_rows(texts, prefix, spans, 2, "float", float("nan"))
        rc, v, s, o, dt, tot = _raw_spans(batch, d_prefix, d_spans, 3, 2, "float", nan, rows)
        assert rc == M.api.MRX_OK and np.array_equal(v[:rows], val) and np.array_equal(s[:rows], st)
        assert np.all(v[:rows][st != P.OK] == nan) and (st != P.OK).any()
        assert lib.mrx_debug_scratch_in_use() == 0
    # n == 0
    empty = M.DeviceBatch(torch.zeros(16, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc, v, s, o, dt, tot = _raw_spans(empty, zero, d_spans, 3, 1, "int", -7, 5)
    assert rc == M.api.MRX_OK and tot == [0, -7] and dt.tolist() == [0, -9, -9, -9, -9]
    assert np.all(v == -9) and np.all(s == 0xEE) and np.all(o == -9)
    values, status = empty.parse("hex")
    assert values.numel() == 0 and status.numel() == 0
    values, status, own = empty.parse_spans(zero, d_spans[:0], 0, "float")
    assert values.numel() == 0 and values.dtype == torch.float64 and own.numel() == 0
    assert lib.mrx_debug_scratch_in_use() == 0


# ---- numbers -----------------------------------------------------------------------------------------------------------

LOG = [b"GET /a 200 1532 0.004", b"", b"POST /b/17 500 12 1.250 x", b"-5 3.25 and -17 0.5 then 8 9.", b"no numbers here",
       b"99999999999999999999 1", b"0x1f 0xzz 0xffffffffffffffffff 0xA", b"x1x xx7", b"12 3.5", b"7 7.0 8 8.00 9 9.125 10 1.5"]


def _findall_want(pat, texts, kind, fill):
    rows = X.findall_rows(pat, texts)
    prefix = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=prefix[1:])
    pieces = [t[s:e] for t, rs in zip(texts, rows) for s, e in rs]
    return prefix, pieces, P.expect_many(pieces, kind, fill)


def _group_want(pat, texts, group, count, kind, fill):
    g = CA.num_groups(pat)
    rows = [CA.expected_rows(pat, t, count, g) for t in texts]
    prefix = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=prefix[1:])
    pieces = [P.clamp_piece(t, *row[X.group_pair(group, g)]) for t, rs in zip(texts, rows) for row in rs]
    return prefix, pieces, P.expect_many(pieces, kind, fill)


def _assert_numbers(got, want, n):
    import torch
    values, status, prefix, owner = got
    w_prefix, pieces, (st, val) = want
    torch.cuda.synchronize()
    assert np.array_equal(_np(prefix), w_prefix)
    assert np.array_equal(_np(status), st), pieces
    assert np.array_equal(_bits(values), val), pieces
    assert np.array_equal(_np(owner), np.repeat(np.arange(n, dtype=np.int64), np.diff(w_prefix)))


def test_numbers_of_findall_matches():
    batch = M.DeviceBatch.from_texts(LOG)
    want = _findall_want(b"\\d+", LOG, "int", -1)
    assert len(want[1]) > 30 and P.RANGE in want[2][0]
    _assert_numbers(M.compile_regex(b"\\d+").numbers(batch, "int", fill=-1), want, len(LOG))
    texts = LOG + [b"0x1f", b"a 0x1f b", b"0x1f 0x2", b"0x7fffffffffffffff 0x8000000000000000", b"0x0 0x", b"0xdeadbeef"]
    want = _findall_want(b"0x[0-9a-f]+", texts, "hex", 0)
    assert set(want[2][0].tolist()) == {P.OK, P.RANGE} and len(want[1]) >= 7
    _assert_numbers(M.compile_regex(b"0x[0-9a-f]+").numbers(M.DeviceBatch.from_texts(texts), "hex"), want, len(texts))
    with pytest.raises(M.MrxError):
        M.compile_regex(b"\\d+").numbers(batch, "int", count=2)
    with pytest.raises(M.MrxError):
        M.compile_regex(b"\\d+").numbers(batch, "decimal")


def test_numbers_of_groups_with_a_count_and_an_unset_group():
    pat = b"(-?\\d+) (\\d+\\.\\d+)"
    rx = M.compile_regex(pat)
    lay = LY.ragged_rows(LOG, False, _poison(5))
    for batch in (M.DeviceBatch.from_texts(LOG), lay.device()):
        _assert_numbers(rx.numbers(batch, "int", group=1, fill=-1), _group_want(pat, LOG, 1, 0, "int", -1), len(LOG))
        _assert_numbers(rx.numbers(batch, "float", group=2, fill=-0.0), _group_want(pat, LOG, 2, 0, "float", -0.0), len(LOG))
        _assert_numbers(rx.numbers(batch, "float", group=0), _group_want(pat, LOG, 0, 0, "float", 0), len(LOG))
        want = _group_want(pat, LOG, 2, 2, "float", 0)
        assert int(np.diff(want[0]).max()) == 2 and len(want[1]) < len(_group_want(pat, LOG, 2, 0, "float", 0)[1])
        _assert_numbers(rx.numbers(batch, "float", group=2, count=2), want, len(LOG))
    with pytest.raises(M.MrxError):
        rx.numbers(M.DeviceBatch.from_texts(LOG), "int", group=3)
    pat = b"x(\\d)?"
    want = _group_want(pat, LOG, 1, 0, "int", -3)
    assert P.EMPTY in want[2][0] and P.OK in want[2][0]
    _assert_numbers(M.compile_regex(pat).numbers(M.DeviceBatch.from_texts(LOG), "int", group=1, fill=-3), want, len(LOG))
    assert M.numbers(pat, [b"x1x xx7", b"", b"x"], "int", group=1) == [[1, None, None, 7], [], [None]]


def test_list_form_of_numbers():
    def lists(want, kind):
        prefix, pieces, _ = want
        flat = [P.python_value(p, kind) for p in pieces]
        return [flat[prefix[i]:prefix[i + 1]] for i in range(len(prefix) - 1)]

    got = M.numbers(b"\\d+", LOG)
    assert got == lists(_findall_want(b"\\d+", LOG, "int", 0), "int") and None in got[5] and got[1] == []
    assert all(type(v) is int for row in got for v in row if v is not None)
    pat = b"(-?\\d+) (\\d+\\.\\d+)"
    got = M.compile_regex(pat).numbers(LOG, kind="float", group=2)
    assert got == lists(_group_want(pat, LOG, 2, 0, "float", 0), "float")
    assert all(type(v) is float for row in got for v in row) and got[3] == [3.25, 0.5]
    assert M.numbers(pat, LOG, "int", 1, 1) == lists(_group_want(pat, LOG, 1, 1, "int", 0), "int")
    assert M.numbers(b"\\d+", []) == []


def test_pipeline_sum_per_text_over_owner():
    import torch
    rng = np.random.default_rng(9)
    texts = [b" ".join(str(int(v)).encode() for v in rng.integers(0, 10 ** 9, size=int(rng.integers(0, 9)))) + b" 1e5 z"
             for _ in range(500)]
    batch = M.DeviceBatch.from_texts(texts)
    values, status, prefix, owner = M.compile_regex(b"\\d+").numbers(batch)
    assert bool((status == 0).all())
    sums = torch.zeros(batch.n, dtype=torch.int64, device="cuda").index_add_(0, owner, values)
    want = [sum(int(t[s:e]) for s, e in rs) for t, rs in zip(texts, X.findall_rows(b"\\d+", texts))]
    assert _np(sums).tolist() == want and max(want) > 10 ** 9
