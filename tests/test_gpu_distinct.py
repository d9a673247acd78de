"""distinct on the GPU against a Python dict in insertion order (tests/distinct_expect.py): the group of every text, the
first index and count of every group, the values' CSR and bytes and the totals, bit for bit, on every layout of
tests/layouts.py; forced hash collisions; the edges of the contract in include/mrx.h (capacity, canaries, asynchronous
form, sizes, scratch); and value_counts behind a pattern against collections.Counter over the oracle's pieces."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import mojo_regex_amd as M
import distinct_expect as D
import extract_expect as X
import layouts as LY

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _poison(seed=0):
    """Bytes around the texts that would change an answer if they were read as text: zero bytes (a masked window reads
    as zeros: "a" against "a\\0"), the texts' own alphabet, and the text itself once more."""
    rng = np.random.default_rng(1000 + seed)

    def pz(i, t, k):
        if k <= 0:
            return b""
        kind = int(rng.integers(0, 3))
        fill = b"\0" * k if kind == 0 else bytes(rng.integers(97, 101, size=k).tolist()) if kind == 1 else (t + b"\0a") * k
        return fill[:k]
    return pz


def _edge_texts():
    """About 120 texts: duplicates at distance, empty texts, a text and its proper prefix, pairs that differ in the last
    byte or by a trailing \\0 only, lengths 0..49, and three 70 KB texts, two equal and one with another last byte."""
    rng = np.random.default_rng(42)
    by_len = [bytes(rng.integers(97, 101, size=k).tolist()) for k in range(50)]          # lengths 0..49
    texts = list(by_len)
    texts += [b"", b"a", b"a\0", b"a\0\0", b"\0", b"\0\0", b"ab", b"abc", b"abd", b""]   # prefixes, NULs, last bytes
    texts += [t[:-1] + bytes([t[-1] ^ 1]) for t in by_len[15:19] + by_len[31:34] + by_len[47:50]]   # last byte differs
    texts += [t + b"\0" for t in (by_len[15], by_len[16], by_len[32], by_len[48])]        # a trailing NUL more
    texts += [by_len[k] for k in (0, 1, 7, 16, 17, 32, 33, 48, 49)]                       # duplicates at distance
    big = bytes(rng.integers(97, 123, size=70000).tolist())
    texts += [big, b"a", big[:-1] + b"!", b"", by_len[16]]
    texts += [bytes(rng.integers(97, 99, size=int(rng.integers(0, 4))).tolist()) for _ in range(20)]   # many repeats
    texts += [big, by_len[49], b"a\0"]
    assert 100 <= len(texts) <= 140
    return texts


def _assert_result(res, want, where):
    values, counts, group_of, first = res
    wg, wf, wc, woff, wdata = want
    assert values.offsets is not None and values.n == len(wf), where
    assert np.array_equal(_np(group_of), wg), where
    assert np.array_equal(_np(first), wf), where
    assert np.array_equal(_np(counts), wc), where
    assert np.array_equal(_np(values.offsets), woff), where
    assert np.array_equal(_np(values.data), wdata), where


def _raw_call(batch, out_data, cap, totals=True, pad=0):
    """The C call on the caller's own buffers, each n-sized array with `pad` canary elements behind it: (rc, group_of,
    first, counts, out_offsets, d_totals, host totals), the arrays with their canaries."""
    import torch
    dev, n = batch.data.device, batch.n
    g, f, c = (torch.full((n + pad,), -9, dtype=torch.int64, device=dev) for _ in range(3))
    off = torch.full((n + 1 + pad,), -9, dtype=torch.int64, device=dev)
    dt = torch.full((2,), -9, dtype=torch.int64, device=dev)
    ht = (C.c_int64 * 2)(-7, -7)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = batch.call(M.load_library(), "mrx_distinct", (),
                    (g.data_ptr(), f.data_ptr(), c.data_ptr(), off.data_ptr(), out_data.data_ptr(), cap, dt.data_ptr(),
                     C.cast(ht, C.c_void_p) if totals else None, stream))
    torch.cuda.synchronize()
    return rc, _np(g), _np(f), _np(c), _np(off), _np(dt).tolist(), list(ht)


def _assert_raw(got, want, n, pad):
    _, g, f, c, off, dt, _ = got
    wg, wf, wc, woff, wdata = want
    u = len(wf)
    assert dt == [u, len(wdata)]
    assert np.array_equal(g[:n], wg) and np.array_equal(f[:u], wf) and np.array_equal(c[:u], wc)
    assert np.array_equal(off[:u + 1], woff)
    for a, size in ((g, n), (f, n), (c, n), (off, n + 1)):   # the canaries behind the n-sized arrays
        assert len(a) == size + pad and np.all(a[size:] == -9)


@pytest.fixture(scope="module")
def edge_layouts():
    texts = _edge_texts()
    lays = LY.layouts_for(texts, _poison())
    lays.append(LY.fixed_length(texts, 32, 1, _poison(1)))   # rows of one byte: few values, every text a duplicate
    lays.append(LY.fixed_length(texts, 80, 49, _poison(2)))
    for lay in lays[-2:]:
        lay.check()
    return [(lay, D.expected(lay.texts)) for lay in lays]


def test_every_layout(edge_layouts):
    import torch
    lib = M.load_library()
    names = set()
    for lay, want in edge_layouts:
        names.add(lay.name)
        batch = lay.device()
        res = batch.distinct()
        torch.cuda.synchronize()
        _assert_result(res, want, lay.name)
        assert 1 <= len(want[1]) and want[2].sum() == batch.n
        if lay.csr or lay.lens is not None:
            assert len(want[1]) < batch.n and 70000 in np.diff(want[3])   # duplicates, and the long value
        if not lay.csr and lay.lens is None:
            assert res[0]._max_len == lay.length
        elif not lay.csr:
            assert res[0]._max_len == lay.stride
        elif lay.known:
            assert res[0]._max_len == max(len(t) for t in lay.texts)
        else:
            assert res[0]._max_len is None and res[0]._end_offset is None
        if not lay.csr or lay.known:
            assert res[0]._end_offset == len(want[4])
        assert lib.mrx_debug_scratch_in_use() == 0
    assert {"csr_packed", "csr_shift1", "csr_shift7", "csr_shift15", "fixed32_len1", "fixed80_len49"} <= names


def _collision_batches():
    rng = np.random.default_rng(8)
    vals = [bytes(rng.integers(97, 100, size=int(rng.integers(0, 20))).tolist()) for _ in range(60)]
    many = [vals[int(k)] for k in rng.integers(0, 60, size=200)]
    assert len(set(many)) > 40
    return many


@pytest.mark.parametrize("mask", [0, 3])
def test_forced_collisions_change_nothing(edge_layouts, mask):
    import torch
    lib = M.load_library()
    many = _collision_batches()
    cases = [(lay.device(), want, lay.name) for lay, want in edge_layouts if lay.name in ("csr_packed", "csr_shift7") or lay.name.startswith("lens")]
    assert len(cases) == 4
    cases.append((M.DeviceBatch.from_texts(many), D.expected(many), "200 texts"))
    plain = [b.distinct() for b, _, _ in cases]
    torch.cuda.synchronize()
    try:
        lib.mrx_debug_distinct_hash_mask(mask)
        for (batch, want, name), base in zip(cases, plain):
            assert batch.n <= 400
            res = batch.distinct()
            torch.cuda.synchronize()
            _assert_result(res, want, (name, mask))
            for a, b in zip((res[0].data, res[0].offsets) + res[1:], (base[0].data, base[0].offsets) + base[1:]):
                assert torch.equal(a, b), (name, mask)
    finally:
        lib.mrx_debug_distinct_hash_mask(0xFFFFFFFFFFFFFFFF)


def _repeats(n, u, seed, lo=0, hi=24):
    rng = np.random.default_rng(seed)
    vals = list(dict.fromkeys(bytes(rng.integers(97, 123, size=int(rng.integers(lo, hi))).tolist()) for _ in range(4 * u)))[:u]
    assert len(vals) == u
    skew = np.minimum((rng.pareto(1.1, size=n) * 3).astype(np.int64), u - 1)   # a few values take most of the texts
    return [vals[int(k)] for k in skew[:n - u]] + vals   # (every value occurs)


def test_several_rounds_per_wavefront():
    import torch
    lib = M.load_library()
    texts = _repeats(5000, 1500, 3)
    want = D.expected(texts)
    assert len(want[1]) == 1500
    batches = (M.DeviceBatch.from_texts(texts), LY.csr_shifted(texts, 7, _poison(3)).device())
    try:
        lib.mrx_debug_distinct_grid(1)
        for batch in batches:   # known bounds: a lane per text hashes; unknown: 16 lanes per text
            res = batch.distinct()
            torch.cuda.synchronize()
            _assert_result(res, want, "grid 1")
    finally:
        lib.mrx_debug_distinct_grid(0)
    _assert_result(batches[0].distinct(), want, "no cap")


def test_hot_slot_and_no_duplicates():
    import torch
    same = [b"the same text"] * 4096
    values, counts, group_of, first = M.DeviceBatch.from_texts(same).distinct()
    assert values.n == 1 and _np(counts).tolist() == [4096] and _np(first).tolist() == [0]
    assert not _np(group_of).any() and _np(values.data).tobytes() == b"the same text"
    assert _np(values.offsets).tolist() == [0, 13]
    n = 5000
    texts = [b"%09d" % (k * 7919) for k in range(n)]
    batch = M.DeviceBatch.from_texts(texts)
    values, counts, group_of, first = batch.distinct()
    assert values.n == n and np.array_equal(_np(first), np.arange(n)) and np.array_equal(_np(group_of), np.arange(n))
    assert np.all(_np(counts) == 1)
    assert torch.equal(values.data, batch.data) and torch.equal(values.offsets, batch.offsets)


def test_no_text_and_one_text():
    import torch
    values, counts, group_of, first = M.DeviceBatch.from_texts([]).distinct()
    assert values.n == 0 and _np(values.offsets).tolist() == [0] and values.data.numel() == 0
    assert counts.numel() == 0 and group_of.numel() == 0 and first.numel() == 0
    d = torch.zeros(0, dtype=torch.uint8, device="cuda")
    got = _raw_call(M.DeviceBatch(d, torch.zeros(1, dtype=torch.int64, device="cuda")), d, 0)
    assert got[0] == M.api.MRX_OK and got[4].tolist() == [0] and got[5] == [0, 0] and got[6] == [0, 0]
    assert M.distinct([])[0] == []
    for t in (b"one text", b""):
        _assert_result(M.DeviceBatch.from_texts([t]).distinct(), D.expected([t]), t)
        v, c, g, f = M.distinct([t])
        assert v == [t] and c.tolist() == [1] and g.tolist() == [0] and f.tolist() == [0]


def test_reproducible():
    import torch
    batch = M.DeviceBatch.from_texts(_repeats(5000, 700, 9))
    a, b = batch.distinct(), batch.distinct()
    torch.cuda.synchronize()
    for x, y in zip((a[0].data, a[0].offsets) + a[1:], (b[0].data, b[0].offsets) + b[1:]):
        assert torch.equal(x, y)


def test_capacity_and_canaries():
    import torch
    texts = _repeats(900, 200, 11, lo=1, hi=40) + [b"", b"x" * 300, b""]
    batch = M.DeviceBatch.from_texts(texts)
    want = D.expected(texts)
    nbytes, n, pad = len(want[4]), len(texts), 8
    assert 0 < nbytes < batch.data.numel()
    buf = torch.full((nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    got = _raw_call(batch, buf, nbytes - 1, pad=pad)
    assert got[0] == M.api.MRX_E_CAPACITY and got[6] == [len(want[1]), nbytes]
    assert ("need %d" % nbytes).encode() in M.load_library().mrx_last_error()
    _assert_raw(got, want, n, pad)
    assert np.all(_np(buf) == 0xA5)
    got = _raw_call(batch, buf, nbytes, pad=pad)
    assert got[0] == M.api.MRX_OK and got[6] == [len(want[1]), nbytes]
    _assert_raw(got, want, n, pad)
    out = _np(buf)
    assert np.array_equal(out[:nbytes], want[4]) and np.all(out[nbytes:] == 0xA5)
    with pytest.raises(M.MrxError):
        batch.distinct(out_cap=nbytes - 1)
    _assert_result(batch.distinct(out_cap=nbytes), want, "exact capacity")


def test_asynchronous_form():
    import torch
    texts = _repeats(2000, 300, 13)
    want = D.expected(texts)
    nbytes, n = len(want[4]), len(texts)
    for batch in (M.DeviceBatch.from_texts(texts), LY.ragged_rows(texts, False, _poison(4)).device()):
        buf = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        got = _raw_call(batch, buf, nbytes, totals=False, pad=4)
        assert got[0] == M.api.MRX_OK and got[6] == [-7, -7]   # nothing on the host changed
        _assert_raw(got, want, n, 4)
        out = _np(buf)
        assert np.array_equal(out[:nbytes], want[4]) and np.all(out[nbytes:] == 0xA5)
        # too small: the device decides, no byte is written, the rest is complete
        buf.fill_(0xA5)
        got = _raw_call(batch, buf, nbytes - 1, totals=False, pad=4)
        assert got[0] == M.api.MRX_OK and got[6] == [-7, -7] and np.all(_np(buf) == 0xA5)
        _assert_raw(got, want, n, 4)
        outs = (torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda"),
                torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                torch.empty(int(batch.data.numel()), dtype=torch.uint8, device="cuda"),
                torch.empty(2, dtype=torch.int64, device="cuda"))
        batch.distinct_async(outs)
        torch.cuda.synchronize()
        u = len(want[1])
        assert _np(outs[5]).tolist() == [u, nbytes] and np.array_equal(_np(outs[0]), want[0])
        assert np.array_equal(_np(outs[1])[:u], want[1]) and np.array_equal(_np(outs[2])[:u], want[2])
        assert np.array_equal(_np(outs[3])[:u + 1], want[3]) and np.array_equal(_np(outs[4])[:nbytes], want[4])
    assert M.load_library().mrx_debug_scratch_in_use() == 0


def test_host_list_form():
    texts = _edge_texts()
    want = D.expected(texts)
    v, c, g, f = M.distinct(texts)
    assert v == D.values(want) == list(dict.fromkeys(texts))
    for got, w in zip((g, f, c), want[:3]):
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, w)


@pytest.mark.parametrize("pat,group", [(b"[a-z]+\\d+", None), (b"(\\w+) (\\w+)", 1)], ids=["findall", "group1"])
def test_value_counts_chains_extract_and_distinct(pat, group):
    texts = LY.make_texts(pat, 150, n_long=2) + [b"ab1 ab1 zz9 ab1", b"foo bar foo bar", b"", b"ab1"]
    rx, rx2 = M.compile_regex(pat), M.compile_regex(b"a")
    packed = X.expected_findall(pat, texts) if group is None else X.expected_group(pat, texts, group)
    pieces = [p for per_text in X.lists(packed) for p in per_text]
    want = list(Counter(pieces).items())
    assert want == D.value_counts(pieces) and len(want) < len(pieces)
    for batch in (M.DeviceBatch.from_texts(texts), LY.ragged_rows(texts, False, LY.pattern_poison(pat)).device()):
        values, counts = rx.value_counts(batch, group=group)
        raw, off = _np(values.data).tobytes(), _np(values.offsets)
        assert [(raw[off[g]:off[g + 1]], int(c)) for g, c in enumerate(_np(counts))] == want
        assert values._end_offset == len(raw) and values._max_len is not None
        kept, idx = rx2.filter(values)   # the values are a batch like any other
        assert [raw[off[int(g)]:off[int(g) + 1]] for g in _np(idx)] == [v for v, _ in want if b"a" in v]
    assert rx.value_counts(texts, group=group) == want
    assert M.value_counts(pat, texts, group=group) == want
