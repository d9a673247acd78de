"""Fields on the GPU (include/mrx.h, "fields"): rows, nf and prefix bit for bit against tests/fields_expect.py, under
every pinned group of lanes and under the rule, on the edges of a word and of a round, at the edges of a group and of a
wavefront, in every layout with adversarial bytes outside the texts, on one long text, with the early stop, against the
regex split it replaces for one byte, in front of parse_spans, gather_spans and expand_spans, on the caller's tensors
and on host lists.  Every shape is the smallest at which the kernel can still go wrong."""
import numpy as np
import pytest

import mojo_regex_amd as M
import fields_cases as FC
import fields_expect as FE
import layouts as LY

pytestmark = pytest.mark.gpu

PINS = FC.GROUPS + (0,)   # 0: the rule


def _np(t):
    return t.cpu().numpy()


def _scratch_is_untouched():
    assert M.load_library().mrx_debug_scratch_in_use() == 0


@pytest.fixture
def pin():
    lib = M.load_library()

    def set_group(G):
        assert lib.mrx_debug_fields_group(G) == G

    yield set_group
    assert lib.mrx_debug_fields_group(0) == 0
    lib.mrx_debug_fields_grid(0)


def _assert_fields(batch, texts, columns, delim, rest, where, counts=True, want=None):
    want = FE.expected(texts, columns, delim, rest) if want is None else want
    prefix, rows, nf = batch.fields(columns, delim, rest, counts)
    assert M.load_library().mrx_last_kernel_name() == b"k_fields"
    _scratch_is_untouched()
    assert tuple(rows.shape) == (len(texts), len(columns), 2)
    got = _np(rows)
    assert np.array_equal(got, want[0]), (where, [(i, got[i].tolist(), want[0][i].tolist())
                                                  for i in np.nonzero((got != want[0]).any(axis=(1, 2)))[0][:3]])
    assert np.array_equal(_np(prefix), want[2]), where
    if counts:
        assert np.array_equal(_np(nf), want[1]), where
    else:
        assert nf is None
    return want


@pytest.mark.parametrize("G", PINS)
def test_block_and_round_edges(G, pin):
    pin(G)
    for delim in FC.MODES:
        cases = FC.edges(G or 2, delim[0] if delim else 32)
        texts = list(cases.values())
        batch = M.DeviceBatch.from_texts(texts)
        for cols, rest in FC.REQUESTS + ((FC.WIDE, False),):
            _assert_fields(batch, texts, cols, delim, rest, (G, delim, cols, rest))
        # one text per call: REST with cmax equal to 1, nf and nf + 1
        for name in ("three fields", "a field longer than two rounds", "only separators", "only whitespace", "0 letters"):
            t = cases[name]
            one = M.DeviceBatch.from_texts([t])
            for cols, rest in FC.rest_requests(FE.row(t, [1], delim)[1]):
                _assert_fields(one, [t], cols, delim, rest, (G, delim, name, cols))


@pytest.mark.parametrize("G", PINS)
def test_group_and_wavefront_edges(G, pin):
    pin(G)
    per_round = 64 // (G or 2)
    for n in sorted({1, 63, 64, 65, max(per_round - 1, 1), per_round + 1}):
        texts = FC.short_texts(n, seed=G)
        batch = M.DeviceBatch.from_texts(texts)
        for delim in FC.MODES:
            _assert_fields(batch, texts, [1, 3, -1], delim, False, (G, n, delim))
            _assert_fields(batch, texts, [2], delim, True, (G, n, delim, "rest"))
    # one workgroup: every wavefront takes many rounds of texts
    M.load_library().mrx_debug_fields_grid(1)
    texts = FC.short_texts(3000, seed=G + 1)
    batch = M.DeviceBatch.from_texts(texts)
    _assert_fields(batch, texts, [2, -1, 1], None, False, (G, "one workgroup"))
    _assert_fields(batch, texts, [2, -1, 1], b",", False, (G, "one workgroup"))


def _poison(seed):
    """Bytes outside the texts that are mostly delimiters and whitespace: a kernel that read them as text would find
    other fields."""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(b",, \tq\n", np.uint8)
    return lambda i, t, k: al[rng.integers(0, len(al), size=k)].tobytes() if k > 0 else b""


def test_every_layout(pin):
    texts = FC.short_texts(40, seed=3) + FC.log_lines(20, seed=3)
    lays = LY.layouts_for(texts, _poison(1))
    cols = [1, 3, -1]
    with_outside = changed = 0
    for lay in lays:
        for i, t in enumerate(lay.texts):
            outside = lay.outside(i)
            if outside:
                with_outside += 1
                changed += any(FE.row(t + outside, cols, d) != FE.row(t, cols, d) for d in FC.MODES)
    assert with_outside >= 300 and 2 * changed >= with_outside, (with_outside, changed)   # the outside would show
    for lay in lays:
        batch = lay.device()
        for delim in FC.MODES:
            want = FE.expected(lay.texts, cols, delim)
            for G in PINS:
                pin(G)
                _assert_fields(batch, lay.texts, cols, delim, False, (lay.name, delim, G), want=want)
            _assert_fields(batch, lay.texts, [2, 4], delim, True, (lay.name, delim, "rest"))
            _assert_fields(batch, lay.texts, [2, 4], delim, False, (lay.name, delim, "early stop"), counts=False)


@pytest.fixture(scope="module")
def long_text():
    """1 MiB with about 10^5 fields, for both modes: letters with a ", " every ten bytes or so."""
    rng = np.random.default_rng(5)
    t = np.full(1 << 20, ord("x"), np.uint8)
    at = np.cumsum(rng.integers(6, 15, size=110000))
    at = at[at < len(t) - 2]
    t[at] = ord(",")
    t[at + 1] = ord(" ")
    t = t.tobytes()
    cols = [1, 50000, -1]
    return t, cols, {d: FE.expected([t], cols, d) for d in FC.MODES}


@pytest.mark.parametrize("G", PINS)
def test_one_long_text(G, pin, long_text):
    pin(G)
    t, cols, wants = long_text
    batch = M.DeviceBatch.from_texts([t])
    for delim in FC.MODES:
        assert 90000 < wants[delim][1][0] < 120000
        _assert_fields(batch, [t], cols, delim, False, (G, delim), want=wants[delim])


def test_the_early_stop_gives_the_same_rows(pin):
    texts = FC.short_texts(200, seed=9) + FC.log_lines(100, seed=9) + list(FC.edges(4, 44).values())
    batch = M.DeviceBatch.from_texts(texts)
    for G in PINS:
        pin(G)
        for delim in FC.MODES:
            for cols in ([1], [3, 1], [2, 11]):
                want = _assert_fields(batch, texts, cols, delim, False, (G, delim, cols, "counts"))
                _assert_fields(batch, texts, cols, delim, False, (G, delim, cols, "early stop"), counts=False, want=want)


def test_agrees_with_the_regex_split_it_replaces():
    rng = np.random.default_rng(13)
    al = np.frombuffer(b"ab,,1 ", np.uint8)
    texts = [al[rng.integers(0, len(al), size=int(rng.integers(0, 90)))].tobytes() for _ in range(300)]
    batch = M.DeviceBatch.from_texts(texts)
    cols = [1, 3, 7]
    pprefix, ranges, total = M.compile_regex(b",").split_dev(batch)
    pprefix, ranges = _np(pprefix), _np(ranges)
    prefix, rows, nf = batch.fields(cols, b",")
    rows, nf = _np(rows), _np(nf)
    assert np.array_equal(nf, np.diff(pprefix))
    for i in range(len(texts)):
        for j, c in enumerate(cols):
            k = pprefix[i] + c - 1
            want = tuple(ranges[k].tolist()) if k < pprefix[i + 1] else (-1, -1)
            assert tuple(rows[i, j].tolist()) == want, (i, j)


def test_in_front_of_the_consumers():
    import torch
    log = FC.log_lines(400, seed=21)
    log[7] = b""                  # no field at all
    log[8] = b"host1 too short"   # no column 10
    data = torch.from_numpy(np.frombuffer(b"\n".join(log) + b"\n", np.uint8).copy()).cuda()
    lines = M.DeviceBatch.from_lines(data)
    assert lines.n == len(log)
    cols = [1, 10]
    prefix, rows, nf = lines.fields(cols)
    # awk '{s[$1] += $10}': the sums per key, with no pattern and no host in between
    values, status, owner = lines.parse_spans(prefix, rows, pair=1, kind="int")
    keys, _ = lines.gather_spans(prefix, rows, pair=0)
    uniq, counts, group_of, first = keys.distinct()
    ok = status == 0
    sums = torch.zeros(uniq.n, dtype=torch.int64, device="cuda").index_add_(0, group_of[owner[ok]], values[ok])
    want = {}
    for l in log:
        p = l.split()
        if len(p) >= 10 and p[9].isdigit():
            want[p[0]] = want.get(p[0], 0) + int(p[9])
    raw, off = _np(uniq.data).tobytes(), _np(uniq.offsets)
    got = {raw[off[g]:off[g + 1]]: int(s) for g, s in enumerate(_np(sums).tolist())}
    assert {k: v for k, v in got.items() if k in want or v} == want
    assert _np(status).tolist() == [0 if len(l.split()) >= 10 and l.split()[9].isdigit() else (1 if len(l.split()) < 10 else 2) for l in log]
    # gather_spans(pair=j) against fields_of
    host = M.fields_of(log, cols)
    assert host == [[(l.split()[c - 1] if len(l.split()) >= c else None) for c in cols] for l in log]
    for j in range(len(cols)):
        pieces, _ = lines.gather_spans(prefix, rows, pair=j)
        raw, off = _np(pieces.data).tobytes(), _np(pieces.offsets)
        assert [raw[off[i]:off[i + 1]] for i in range(pieces.n)] == [h[j] or b"" for h in host]
    # cut against join
    records, rowner = lines.cut([1, 3, 2])
    raw, off = _np(records.data).tobytes(), _np(records.offsets)
    want_records = [b" ".join((l.split() + [b"", b"", b""])[k] for k in (0, 2, 1)) + b"\n" for l in log]
    assert [raw[off[i]:off[i + 1]] for i in range(records.n)] == want_records
    assert _np(rowner).tolist() == list(range(len(log)))
    csv = [l.replace(b" ", b";") for l in log]
    records, _ = M.DeviceBatch.from_texts(csv).cut([2, 1], delim=b";", out_delim=b"\t", end=b"|")
    raw, off = _np(records.data).tobytes(), _np(records.offsets)
    assert [raw[off[i]:off[i + 1]] for i in range(records.n)] == [
        b"\t".join((l.split(b";") + [b""])[k] for k in (1, 0)) + b"|" for l in csv]
    with pytest.raises(M.MrxError, match="at most 9 columns"):
        lines.cut(list(range(1, 11)))
    _scratch_is_untouched()


def test_the_asynchronous_form_on_the_callers_tensors():
    import torch
    texts = FC.short_texts(130, seed=17) + FC.log_lines(30, seed=17)
    rows128 = [(t + b", " * 64)[:128] for t in texts]
    raw = torch.from_numpy(np.frombuffer(b"".join(rows128), np.uint8).copy()).cuda()
    known = M.DeviceBatch.from_texts(texts)
    batches = [(M.DeviceBatch.strided(raw, 128, length=128), rows128), (known, texts),
               (M.DeviceBatch(known.data, known.offsets), texts)]
    cols = [2, -1, 1]
    stream = torch.cuda.Stream()
    for batch, its_texts in batches:
        n = batch.n
        for delim, rest, c in ((b",", False, cols), (None, False, cols), (None, True, [1, 2])):
            want = FE.expected(its_texts, c, delim, rest)
            for with_nf, with_prefix in ((True, True), (False, False)):
                rows = torch.full((n * len(c) * 2 + 6,), -7, dtype=torch.int32, device="cuda")
                nf = torch.full((n + 3,), -7, dtype=torch.int32, device="cuda")
                prefix = torch.full((n + 1 + 3,), -7, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    batch.fields_async((prefix if with_prefix else None, rows, nf if with_nf else None), c, delim, rest)
                _scratch_is_untouched()
                stream.synchronize()
                rows, nf, prefix = _np(rows), _np(nf), _np(prefix)
                assert np.array_equal(rows[:n * len(c) * 2].reshape(n, len(c), 2), want[0]) and np.all(rows[n * len(c) * 2:] == -7)
                assert np.array_equal(nf[:n], want[1]) if with_nf else np.all(nf[:n] == -7)
                assert np.array_equal(prefix[:n + 1], want[2]) if with_prefix else np.all(prefix[:n + 1] == -7)
                assert np.all(nf[n:] == -7) and np.all(prefix[n + 1:] == -7)


def test_host_lists_and_a_batch_without_texts():
    import torch
    assert M.fields_of([], [1, -1]) == []
    texts = [b"", b"a b", b"", b"", b" x ", b""]
    assert M.fields_of(texts, [1, -1, 2]) == [[None] * 3, [b"a", b"b", b"b"], [None] * 3, [None] * 3, [b"x", b"x", None], [None] * 3]
    assert M.fields_of(texts, [1, -1], delim=b" ") == [[b"", b""], [b"a", b"b"], [b"", b""], [b"", b""], [b"", b""], [b"", b""]]
    assert M.fields_of([b"k=v=w"], [2], delim=b"=", rest=True) == [[b"v=w"]]
    empty = M.DeviceBatch(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    prefix, rows, nf = empty.fields([1, 2], b",")
    assert _np(prefix).tolist() == [0] and tuple(rows.shape) == (0, 2, 2) and nf.numel() == 0
    # mrx_fields_batch, the C wrapper on host buffers
    lib = M.load_library()
    d, o = M.pack_texts(texts)
    c = np.array([1, -1], np.int32)
    rows, nf, pre = np.zeros((6, 2, 2), np.int32), np.zeros(6, np.int32), np.zeros(7, np.int64)
    assert lib.mrx_fields_batch(M.api.MRX_FIELDS_WHITESPACE, 0, c.ctypes.data, 2, d.ctypes.data, o.ctypes.data, 6,
                                rows.ctypes.data, nf.ctypes.data, pre.ctypes.data) == 0
    want = FE.expected(texts, [1, -1])
    assert np.array_equal(rows, want[0]) and np.array_equal(nf, want[1]) and np.array_equal(pre, want[2])
    for bad in ([0], [], list(range(1, 34))):
        with pytest.raises(M.MrxError):
            M.fields_of(texts, bad)
    with pytest.raises(M.MrxError):
        M.fields_of(texts, [1, -1], rest=True)
