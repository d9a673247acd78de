"""Quoted fields on the GPU (include/mrx.h, "quoted fields"): rows, nf, prefix and quoted bit for bit against
tests/fields_quoted_expect.py, under every pinned group of lanes and under the rule, with the quote parity crossing a
word's and a round's edge at four alignments, next to texts that never close their quote, in every layout with quote
and delimiter bytes outside the texts, on one long text, on the caller's tensors, in front of parse_spans, expand_spans
and cut, and through csv_columns and csv_of against csv.reader.  Every shape is the smallest at which the kernel can
still go wrong."""
import csv

import numpy as np
import pytest

import mojo_regex_amd as M
import fields_expect as FE
import fields_quoted_cases as QC
import fields_quoted_expect as QE
import layouts as LY

pytestmark = pytest.mark.gpu

Q = QC.Q
PINS = QC.GROUPS + (0,)   # 0: the rule


def _np(t):
    return t.cpu().numpy()


def _scratch_is_untouched():
    assert M.load_library().mrx_debug_scratch_in_use() == 0


def _texts_of(batch):
    raw, off = _np(batch.data).tobytes(), _np(batch.offsets)
    return [raw[off[i]:off[i + 1]] for i in range(batch.n)]


@pytest.fixture
def pin():
    lib = M.load_library()

    def set_group(G):
        assert lib.mrx_debug_fields_group(G) == G

    yield set_group
    assert lib.mrx_debug_fields_group(0) == 0
    lib.mrx_debug_fields_grid(0)


def _quotes_outside(seed):
    """Bytes outside the texts that are mostly quotes and separators: a kernel that read them as text would begin inside,
    or close a quote that the text leaves open."""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(b'",," \t"q', np.uint8)
    return lambda i, t, k: al[rng.integers(0, len(al), size=k)].tobytes() if k > 0 else b""


def _skewed(texts, skew):
    """A CSR batch whose first text begins `skew` bytes behind an aligned address, quote bytes in front of it."""
    if skew == 0:
        return M.DeviceBatch.from_texts(texts)
    return LY.csr_shifted(texts, skew, lambda i, t, k: Q * k).device()


def _assert_quoted(batch, texts, columns, delim, rest, where, counts=True, want=None):
    want = QE.expected(texts, columns, Q, delim, rest) if want is None else want
    prefix, rows, nf, quoted = batch.fields(columns, delim, rest, counts, quote=Q)
    assert M.load_library().mrx_last_kernel_name() == b"k_fields"
    _scratch_is_untouched()
    assert tuple(rows.shape) == (len(texts), len(columns), 2) and tuple(quoted.shape) == (len(texts), len(columns))
    got = _np(rows)
    assert np.array_equal(got, want[0]), (where, [(i, texts[i][:80], got[i].tolist(), want[0][i].tolist())
                                                  for i in np.nonzero((got != want[0]).any(axis=(1, 2)))[0][:3]])
    assert np.array_equal(_np(quoted), want[3]), where
    assert np.array_equal(_np(prefix), want[2]), where
    if counts:
        assert np.array_equal(_np(nf), want[1]), where
    else:
        assert nf is None
    return want


@pytest.mark.parametrize("G", PINS)
def test_the_table_of_the_contract(G, pin):
    pin(G)
    for t, delim, rest, cols, want_row, want_quoted in QC.TABLE:
        prefix, rows, nf, quoted = M.DeviceBatch.from_texts([t]).fields(cols, delim, rest, quote=Q)
        assert [tuple(p) for p in _np(rows)[0].tolist()] == want_row, (t, cols)
        assert _np(quoted)[0].tolist() == want_quoted and _np(prefix).tolist() == [0, 1]
        assert _np(nf).tolist() == [QE.row(t, cols, Q, delim, rest)[1]]


@pytest.mark.parametrize("skew", QC.SKEWS)
@pytest.mark.parametrize("G", PINS)
def test_word_and_round_edges(G, skew, pin):
    pin(G)
    for delim in QC.MODES:
        texts = list(QC.edges(G or 2, delim[0] if delim else 32).values())
        batch = _skewed(texts, skew)
        for k, (cols, rest) in enumerate(QC.REQUESTS + ((QC.WIDE, False),)):   # negative columns, REST, repeats, f = 32
            want = _assert_quoted(batch, texts, cols, delim, rest, (G, skew, delim, cols, rest))
            if not rest and k % 2 == 0:   # counts=False gives the same rows
                _assert_quoted(batch, texts, cols, delim, rest, (G, skew, delim, cols, "no nf"), counts=False, want=want)


@pytest.mark.parametrize("G", PINS)
def test_a_quote_left_open_stays_with_its_text(G, pin):
    pin(G)
    per_round = 64 // (G or 2)
    pair = [b'"a,b', b"a,b", b'x "a b', b"a b"]
    # the parity must not reach the next text of the same wavefront round
    texts = [pair[k % 4] for k in range(per_round + 1)]
    batch = M.DeviceBatch.from_texts(texts)
    for delim in QC.MODES:
        _assert_quoted(batch, texts, [1, 2, -1], delim, False, (G, delim, "one round"))
        _assert_quoted(batch, texts, [2], delim, True, (G, delim, "one round, rest"))
    # one workgroup: every wavefront runs several rounds, and the parity must not survive a round
    M.load_library().mrx_debug_fields_grid(1)
    texts = [pair[(k + k // 7) % 4] for k in range(4 * 3 * per_round + 5)] + QC.generated_texts(200, seed=G)
    batch = M.DeviceBatch.from_texts(texts)
    for delim in QC.MODES:
        _assert_quoted(batch, texts, [1, 2, -1], delim, False, (G, delim, "one workgroup"))
        _assert_quoted(batch, texts, [1, 2], delim, False, (G, delim, "one workgroup, no nf"), counts=False)


def test_every_layout(pin):
    lines, _ = QC.csv_rows(40, seed=3)
    texts = QC.generated_texts(40, seed=3) + QC.combined_log_lines(10, seed=3) + lines
    lays = LY.layouts_for(texts, _quotes_outside(1))
    cols = [1, 3, -1]
    with_outside = changed = 0
    for lay in lays:
        for i, t in enumerate(lay.texts):
            outside, before = lay.outside(i), lay.before(i)
            if outside:
                with_outside += 1
                changed += any(QE.row(t + outside, cols, Q, d) != QE.row(t, cols, Q, d) for d in QC.MODES) or \
                    before.count(Q) % 2 == 1
    assert with_outside >= 300 and 2 * changed >= with_outside, (with_outside, changed)   # the outside would show
    for lay in lays:
        batch = lay.device()
        for delim in QC.MODES:
            want = QE.expected(lay.texts, cols, Q, delim)
            for G in PINS:
                pin(G)
                _assert_quoted(batch, lay.texts, cols, delim, False, (lay.name, delim, G), want=want)
            _assert_quoted(batch, lay.texts, [2, 4], delim, True, (lay.name, delim, "rest"))
            _assert_quoted(batch, lay.texts, [2, 4], delim, False, (lay.name, delim, "early stop"), counts=False)


def test_one_long_text_under_the_rule():
    """384 KiB as a fixed-pitch batch of one row, so that the call knows the length: G = 64 by the rule.  Quoted
    stretches with separators in them every 40 bytes or so."""
    import torch
    rng = np.random.default_rng(5)
    t = np.full(384 << 10, ord("x"), np.uint8)
    at = np.cumsum(rng.integers(30, 50, size=12000))
    at = at[at < len(t) - 20]
    t[at] = ord(",")
    t[at + 1] = ord(" ")
    for p in at[::3]:   # every third field opens with a quoted stretch that holds a separator pair, some a doubled quote
        t[p + 2] = t[p + 12] = Q[0]
        t[p + 6], t[p + 7] = ord(","), ord(" ")
        if p % 5 == 0:
            t[p + 9] = t[p + 10] = Q[0]
    t = t.tobytes() + b',"ta, il" "ta, il"'   # the last field stands in quotes in both modes
    cols = [1, 2, 5000, -1, -2]
    batch = M.DeviceBatch.strided(torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda(), len(t), length=len(t))
    for delim in QC.MODES:
        want = QE.expected([t], cols, Q, delim)
        assert 9000 < want[1][0] < 13000 and want[3][0].tolist() == [0, 0, 0, 1, 0]
        assert want[1][0] < FE.row(t, [1], delim)[1]   # plain fields would count more
        _assert_quoted(batch, [t], cols, delim, False, delim, want=want)
        assert M.load_library().mrx_debug_fields_last_group() == 64


def test_the_asynchronous_form_on_the_callers_tensors():
    import torch
    lines, _ = QC.csv_rows(60, seed=17)
    texts = QC.generated_texts(100, seed=17) + lines
    rows128 = [(t + b'", ' * 43)[:128] for t in texts]
    raw = torch.from_numpy(np.frombuffer(b"".join(rows128), np.uint8).copy()).cuda()
    known = M.DeviceBatch.from_texts(texts)
    batches = [(M.DeviceBatch.strided(raw, 128, length=128), rows128), (known, texts),
               (M.DeviceBatch(known.data, known.offsets), texts)]
    stream = torch.cuda.Stream()
    for batch, its_texts in batches:
        n = batch.n
        for delim, rest, c in ((b",", False, [2, -1, 1]), (None, False, [2, -1, 1]), (b",", True, [1, 2])):
            want = QE.expected(its_texts, c, Q, delim, rest)
            for with_nf, with_prefix, with_quoted in ((True, True, True), (False, False, False), (True, False, True)):
                rows = torch.full((n * len(c) * 2 + 6,), -7, dtype=torch.int32, device="cuda")
                nf = torch.full((n + 3,), -7, dtype=torch.int32, device="cuda")
                prefix = torch.full((n + 1 + 3,), -7, dtype=torch.int64, device="cuda")
                quoted = torch.full((n * len(c) + 5,), 0xEE, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    batch.fields_async((prefix if with_prefix else None, rows, nf if with_nf else None,
                                        quoted if with_quoted else None), c, delim, rest, quote=Q)
                _scratch_is_untouched()
                stream.synchronize()
                rows, nf, prefix, quoted = _np(rows), _np(nf), _np(prefix), _np(quoted)
                assert np.array_equal(rows[:n * len(c) * 2].reshape(n, len(c), 2), want[0]) and np.all(rows[n * len(c) * 2:] == -7)
                assert np.array_equal(nf[:n], want[1]) if with_nf else np.all(nf[:n] == -7)
                assert np.array_equal(prefix[:n + 1], want[2]) if with_prefix else np.all(prefix[:n + 1] == -7)
                assert np.array_equal(quoted[:n * len(c)].reshape(n, len(c)), want[3]) if with_quoted else np.all(quoted == 0xEE)
                assert np.all(nf[n:] == -7) and np.all(prefix[n + 1:] == -7) and np.all(quoted[n * len(c):] == 0xEE)
    with pytest.raises(M.MrxError, match="quoted must be"):
        known.fields_async((None, torch.empty((known.n, 1, 2), dtype=torch.int32, device="cuda"), None,
                            torch.empty(known.n, dtype=torch.int32, device="cuda")), [1], b",", quote=Q)


def test_a_batch_without_texts_and_the_refusals():
    import torch
    empty = M.DeviceBatch(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    prefix, rows, nf, quoted = empty.fields([1, 2], b",", quote=Q)
    assert _np(prefix).tolist() == [0] and tuple(rows.shape) == (0, 2, 2) and nf.numel() == 0 and tuple(quoted.shape) == (0, 2)
    rows = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    prefix = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    quoted = torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    empty.fields_async((prefix, rows, None, quoted), [1, 2], b",", quote=Q)   # n == 0 writes nothing
    torch.cuda.synchronize()
    assert np.all(_np(rows) == -7) and np.all(_np(prefix) == -7) and np.all(_np(quoted) == 0xEE)
    assert M.fields_of([], [1], b",", quote=Q) == [] and M.csv_of([], [1]) == []
    batch = M.DeviceBatch.from_texts([b'a,"b"'])
    with pytest.raises(M.MrxError, match="quote must differ from delim"):
        batch.fields([1], b",", quote=b",")
    with pytest.raises(M.MrxError, match="whitespace byte"):
        batch.fields([1], quote=b" ")
    with pytest.raises(M.MrxError, match="single byte"):
        batch.fields([1], b",", quote=b'""')
    with pytest.raises(M.MrxError):
        batch.fields([1, -1], b",", rest=True, quote=Q)
    # without quote: the three values of before
    assert len(batch.fields([1], b",")) == 3


def test_in_front_of_the_consumers():
    texts = [b'k1,"42",x', b'k2,42,"y z"', b'k3,"4""2",', b'k4,"",w', b"k5", b'"k6","17","a,b"']
    batch = M.DeviceBatch.from_texts(texts)
    # parse_spans: a quoted number is a number once its quotes are off
    prefix, rows, nf = batch.fields([2], b",")
    _, status, _ = batch.parse_spans(prefix, rows, pair=0, kind="int")
    assert _np(status).tolist()[0] == 2
    prefix, rows, nf, quoted = batch.fields([2, 1], b",", quote=Q)
    values, status, owner = batch.parse_spans(prefix, rows, pair=0, kind="int")
    assert _np(status).tolist() == [0, 0, 2, 1, 1, 0]
    assert _np(values).tolist()[:2] == [42, 42] and _np(values).tolist()[5] == 17
    assert _np(quoted).tolist() == [[1, 0], [0, 0], [1, 0], [1, 0], [0, 0], [1, 1]]
    # expand_spans on the contents (one more pair: expand takes a row's last pair for the whole match)
    prefix, rows, _, _ = batch.fields([3, 1, 1], b",", counts=False, quote=Q)
    records, _ = batch.expand_spans(b"\\2=\\1;", prefix, rows)
    assert _texts_of(records) == [b"k1=x;", b"k2=y z;", b"k3=;", b"k4=w;", b"k5=;", b"k6=a,b;"]
    # cut prints contents
    records, owner = batch.cut([3, 2], delim=b",", out_delim=b"|", quote=Q)
    assert _texts_of(records) == [b"x|42\n", b"y z|42\n", b'|4""2\n', b"w|\n", b"|\n", b"a,b|17\n"]
    assert _np(owner).tolist() == list(range(len(texts)))
    assert _texts_of(batch.cut([3], delim=b",")[0])[1] == b'"y z"\n'   # and without quote what it printed before
    # the combined log format in whitespace mode: status and size are $7 and $8, the request is one column
    log = QC.combined_log_lines(50, seed=4)
    lines = M.DeviceBatch.from_texts(log)
    prefix, rows, nf, quoted = lines.fields([6, 7, 8, -1], quote=Q)
    assert set(_np(nf).tolist()) == {10} and _np(quoted).tolist() == [[1, 0, 0, 1]] * len(log)
    status = lines.parse_spans(prefix, rows, pair=1, kind="int")
    assert _np(status[1]).tolist() == [0] * len(log)
    assert _np(status[0]).tolist() == [int(l.split(b'" ')[1].split()[0]) for l in log]
    got = M.fields_of(log, [6, -1], quote=Q)
    assert got == [[l.split(b'"')[1], l.split(b'"')[-2]] for l in log]
    _scratch_is_untouched()


def test_csv_columns_and_csv_of_are_csv_reader():
    lines, cells = QC.csv_rows()
    read = [[c.encode() for c in r] for r in csv.reader([l.decode() for l in lines])]
    assert read == cells
    cols = [1, 2, 3, 4, 5, 6]
    want = [r + [b""] * (6 - len(r)) for r in read]
    batch = M.DeviceBatch.from_texts(lines)
    columns = M.csv_columns(batch, cols)
    assert len(columns) == 6 and all(c.n == len(lines) for c in columns)
    assert [list(r) for r in zip(*[_texts_of(c) for c in columns])] == want
    assert M.csv_of(lines, cols) == want
    contents = [QE.row(l, [2], Q, b",")[0][0] for l in lines]
    assert _texts_of(M.csv_columns(batch, [2], unescape=False)[0]) == [l[s:e] if s >= 0 else b"" for l, (s, e) in zip(lines, contents)]
    assert M.csv_of([b"a;'b;c';'d''e'"], [1, 2, 3, 4], delim=b";", quote=b"'") == [[b"a", b"b;c", b"d'e", b""]]
    assert M.fields_of([b'a,"b,c",d', b'"a,b'], [2, 3], b",", quote=Q) == [[b"b,c", b"d"], [None, None]]


def test_the_c_batch_form():
    lib = M.load_library()
    texts = [t for t, *_ in QC.TABLE] + [b""]
    n = len(texts)
    d, o = M.pack_texts(texts)
    c = np.array([1, 2, -1], np.int32)
    rows, nf, pre = np.zeros((n, 3, 2), np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.int64)
    quoted = np.full((n, 3), 0xEE, np.uint8)
    assert lib.mrx_fields_quoted_batch(0, 44, Q[0], c.ctypes.data, 3, d.ctypes.data, o.ctypes.data, n, rows.ctypes.data,
                                       nf.ctypes.data, quoted.ctypes.data, pre.ctypes.data) == 0
    want = QE.expected(texts, [1, 2, -1], Q, b",")
    assert np.array_equal(rows, want[0]) and np.array_equal(nf, want[1]) and np.array_equal(pre, want[2])
    assert np.array_equal(quoted, want[3])
