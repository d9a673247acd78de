"""sort and take on the GPU against Python's own sorted(), set and Counter (tests/sort_expect.py): the order, the dense
ranks and the number of different texts, bit for bit, on every layout of tests/layouts.py; groups around the limit of
the comparison kernel and both routes past it; several tiles per wavefront; take in every order through both byte
movers; the edges of the contract in include/mrx.h (capacity, canaries, asynchronous form, invalid indices, sizes,
scratch); and sort= / top= of value_counts and distinct against collections.Counter over the oracle's pieces."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import mojo_regex_amd as M
import extract_expect as X
import layouts as LY
import sort_expect as S

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _poison(seed=0):
    """Bytes around the texts that would change an answer if they were read as text: zero bytes (a masked window reads
    as zeros: "a" against "a\\0"), 0xFF and the texts' own alphabet, and the text itself once more."""
    rng = np.random.default_rng(2000 + seed)

    def pz(i, t, k):
        if k <= 0:
            return b""
        kind = int(rng.integers(0, 4))
        fill = (b"\0" * k if kind == 0 else b"\xff" * k if kind == 1 else
                bytes(rng.integers(97, 101, size=k).tolist()) if kind == 2 else (t + b"\0a") * k)
        return fill[:k]
    return pz


def _edge_texts(big=True):
    """About 150 texts: lengths 0..49, empty texts, a text and its proper prefixes, trailing NULs, the bytes 0x7f, 0x80
    and 0xff, pairs that first differ at byte 7, 8, 9, 15, 16 and 17 (the edges of a round and of a 16-byte window),
    duplicates at distance and, with `big`, three 70 KB texts, two equal and one with another last byte."""
    rng = np.random.default_rng(43)
    by_len = [bytes(rng.integers(97, 101, size=k).tolist()) for k in range(50)]          # lengths 0..49
    texts = list(by_len)
    texts += [b"", b"a", b"a\0", b"a\0\0", b"\0", b"\0\0", b"aa", b"\x7f", b"\x80", b"\xff", b"\x7f\xff", b"\x80\0", b""]
    base = bytes(rng.integers(97, 123, size=24).tolist())
    for k in (7, 8, 9, 15, 16, 17):
        texts += [base[:k] + b"\x80" + base[k + 1:], base[:k] + b"\x7f" + base[k + 1:]]   # unsigned: 0x80 is the larger
        texts += [base[:k] + b"q", base[:k], base[:k] + b"\0"]                            # ... and the prefix rule there
    texts += [t + b"\0" for t in (by_len[7], by_len[8], by_len[16], by_len[32], by_len[48])]   # a trailing NUL more
    texts += [t[:-1] + bytes([t[-1] ^ 1]) for t in by_len[15:19] + by_len[31:34] + by_len[47:50]]   # last byte differs
    texts += [by_len[k] for k in (0, 1, 7, 8, 16, 17, 32, 33, 48, 49)]                    # duplicates at distance
    if big:
        huge = bytes(rng.integers(97, 123, size=70000).tolist())
        texts += [huge, b"a", huge[:-1] + b"!", b"", by_len[16], huge]
    texts += [bytes(rng.integers(97, 99, size=int(rng.integers(0, 4))).tolist()) for _ in range(20)]   # many repeats
    texts += [by_len[49], b"a\0", b"\xff"]
    assert 130 <= len(texts) <= 170
    return texts


def _raw_sort(batch, pad=4, rank=True, totals=True):
    """The C call on the caller's own buffers, each with `pad` canary elements behind it: (rc, order, rank, d_totals)."""
    import torch
    dev, n = batch.data.device, batch.n
    order = torch.full((n + pad,), -9, dtype=torch.int64, device=dev)
    ranks = torch.full((n + pad,), -9, dtype=torch.int64, device=dev)
    dt = torch.full((1 + pad,), -9, dtype=torch.int64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = batch.call(M.load_library(), "mrx_sort", (),
                    (order.data_ptr(), ranks.data_ptr() if rank else None, dt.data_ptr() if totals else None, stream))
    torch.cuda.synchronize()
    return rc, _np(order), _np(ranks), _np(dt)


def _assert_raw_sort(got, want, n, pad=4, rank=True, totals=True):
    rc, order, ranks, dt = got
    assert rc == M.api.MRX_OK
    assert np.array_equal(order[:n], want[0]) and np.all(order[n:] == -9) and len(order) == n + pad
    assert np.array_equal(ranks[:n], want[1]) if rank else np.all(ranks == -9)
    assert np.all(ranks[n:] == -9)
    assert dt[0] == (want[2] if totals else -9) and np.all(dt[1:] == -9)


def _assert_sorted(batch, texts, where):
    import torch
    want = S.expected(texts)
    order, rank, u = batch.argsort(rank=True)
    torch.cuda.synchronize()
    assert order.dtype == torch.int64 and rank.dtype == torch.int64, where
    assert np.array_equal(_np(order), want[0]), where
    assert np.array_equal(_np(rank), want[1]), where
    assert u == want[2], where
    assert M.load_library().mrx_debug_scratch_in_use() == 0
    return want


@pytest.fixture(scope="module")
def edge_layouts():
    texts = _edge_texts()
    lays = LY.layouts_for(texts, _poison())
    lays.append(LY.fixed_length(texts, 32, 1, _poison(1)))   # rows of one byte: few values, every text a duplicate
    lays.append(LY.fixed_length(texts, 80, 49, _poison(2)))
    for lay in lays[-2:]:
        lay.check()
    return [(lay, S.expected(lay.texts)) for lay in lays]


def test_every_layout(edge_layouts):
    import torch
    lib = M.load_library()
    names = set()
    for lay, want in edge_layouts:
        names.add(lay.name)
        batch = lay.device()
        order, rank, u = batch.argsort(rank=True)
        torch.cuda.synchronize()
        assert np.array_equal(_np(order), want[0]), lay.name
        assert np.array_equal(_np(rank), want[1]), lay.name
        assert u == want[2] and 1 <= u, lay.name
        if lay.csr or lay.lens is not None:
            assert u < batch.n and max(len(t) for t in lay.texts) == 70000   # duplicates, and the long texts
        assert lib.mrx_last_kernel_name() == b"k_sort_small"
        assert lib.mrx_debug_scratch_in_use() == 0
        assert torch.equal(batch.argsort(), order)
        _assert_raw_sort(_raw_sort(batch), want, batch.n)
    assert {"csr_packed", "csr_shift1", "csr_shift7", "csr_shift15", "fixed32_len1", "fixed80_len49"} <= names


def _limit_cases():
    rng = np.random.default_rng(17)

    def tails(k, alphabet=(0, 1, 97, 0x7f, 0x80, 0xff), longest=12):
        return [bytes(rng.choice(alphabet, size=int(rng.integers(0, longest))).tolist()) for _ in range(k)]

    cases = {}
    for size in (63, 64, 65):   # exactly `size` texts in one group of round 0, at the limit of the comparison kernel
        cases["share8_%d" % size] = ([b"samehead" + t for t in tails(size - 1)] + [b"samehea", b"samehead", b"samehebd", b"other"])
    cases["equal65"] = [b"one and the same text"] * 65 + [b"one and the same tex", b"one and the same text\0"]
    prefix = bytes(rng.integers(0, 256, size=100).tolist())
    cases["prefix100_80"] = [prefix + t for t in tails(80)] + [prefix[:99], prefix]   # 13 rounds and more
    cases["two_letters_200"] = [bytes(rng.integers(97, 99, size=int(rng.integers(0, 13))).tolist()) for _ in range(200)]
    return cases


@pytest.mark.parametrize("name", ["share8_63", "share8_64", "share8_65", "equal65", "prefix100_80", "two_letters_200"])
def test_group_sizes_around_the_limit_on_both_routes(name):
    lib = M.load_library()
    texts = _limit_cases()[name]
    batches = (M.DeviceBatch.from_texts(texts), LY.csr_shifted(texts, 7, _poison(3)).device())
    try:
        for small in (64, 0, 3):   # the default; every group through radix rounds; a limit in between
            lib.mrx_debug_sort_small(small)
            for batch in batches:   # known bounds: passes are skipped; unknown: every pass runs
                _assert_sorted(batch, texts, (name, small))
                rounds = lib.mrx_debug_sort_rounds()   # which route the groups took
                if name in ("share8_63", "share8_64"):
                    assert rounds == 1 if small == 64 else rounds >= 2, (name, small, rounds)
                elif name == "share8_65":
                    assert rounds >= 2, (name, small, rounds)
                elif name == "equal65":
                    assert rounds == 3, (name, small, rounds)    # 21 bytes: the texts end in the third word
                elif name == "prefix100_80":
                    assert 13 <= rounds <= 15, (name, small, rounds)
    finally:
        lib.mrx_debug_sort_small(-1)


def test_equal_texts_of_the_longest_known_length_end_with_their_last_word():
    lib = M.load_library()
    texts = [b"error503"] * 100 + [b"error504"] * 70 + [b"error50"]
    _assert_sorted(M.DeviceBatch.from_texts(texts), texts, "known bounds")
    assert lib.mrx_debug_sort_rounds() == 1       # no text is longer than 8 bytes: a full word is a whole text
    _assert_sorted(LY.csr_shifted(texts, 7, _poison(10)).device(), texts, "unknown bounds")
    assert lib.mrx_debug_sort_rounds() == 2       # ... which a batch of unknown shape learns one round later
    rows = LY.whole_rows(texts, 8, _poison(11))
    _assert_sorted(rows.device(), rows.texts, "fixed pitch")
    assert lib.mrx_debug_sort_rounds() == 1


def test_both_routes_agree_on_the_edge_texts():
    lib = M.load_library()
    texts = _edge_texts(big=False)   # (without the 70 KB twins: radix rounds alone would take 8750 of them)
    lays = [lay for lay in LY.layouts_for(texts, _poison(4)) if lay.name in ("csr_packed", "csr_shift15", "rows50") or lay.name.startswith("lens")]
    assert len(lays) == 5
    try:
        for small in (64, 0):
            lib.mrx_debug_sort_small(small)
            for lay in lays:
                _assert_sorted(lay.device(), lay.texts, (lay.name, small))
    finally:
        lib.mrx_debug_sort_small(-1)


def test_several_tiles_per_wavefront():
    lib = M.load_library()
    rng = np.random.default_rng(5)
    ties = [bytes(rng.integers(97, 99, size=int(rng.integers(0, 7))).tolist()) for _ in range(20000)]   # stability
    wide = [bytes(rng.integers(0, 256, size=int(rng.integers(0, 41))).tolist()) for _ in range(5000)]
    for texts in (ties, wide):
        want = S.expected(texts)
        batches = (M.DeviceBatch.from_texts(texts), LY.csr_shifted(texts, 1, _poison(5)).device())
        try:
            lib.mrx_debug_sort_grid(1)
            for batch in batches:
                assert _assert_sorted(batch, texts, "grid 1")[2] == want[2]
        finally:
            lib.mrx_debug_sort_grid(0)
        _assert_sorted(batches[0], texts, "no cap")
    assert len(set(ties)) < 300   # groups of hundreds of equal texts


def test_no_text_and_one_text_and_canaries():
    import torch
    empty = M.DeviceBatch.from_texts([])
    assert empty.argsort().numel() == 0
    order, rank, u = empty.argsort(rank=True)
    assert order.numel() == 0 and rank.numel() == 0 and u == 0
    d = torch.zeros(0, dtype=torch.uint8, device="cuda")
    raw = M.DeviceBatch(d, torch.zeros(1, dtype=torch.int64, device="cuda"))
    _assert_raw_sort(_raw_sort(raw), S.expected([]), 0)
    for texts in ([b"one text"], [b""], [b"b", b"a"], [b"", b""], _edge_texts(big=False)):
        batch = M.DeviceBatch.from_texts(texts)
        want = S.expected(texts)
        _assert_raw_sort(_raw_sort(batch), want, len(texts))
        _assert_raw_sort(_raw_sort(batch, rank=False), want, len(texts), rank=False)
        _assert_raw_sort(_raw_sort(batch, rank=False, totals=False), want, len(texts), rank=False, totals=False)
        _assert_raw_sort(_raw_sort(batch, totals=False), want, len(texts), totals=False)
    assert M.load_library().mrx_debug_scratch_in_use() == 0


def test_reproducible_and_host_forms():
    import torch
    texts = _edge_texts()
    batch = M.DeviceBatch.from_texts(texts)
    a, b = batch.argsort(rank=True), batch.argsort(rank=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    got, order = M.sort_texts(texts)
    assert got == sorted(texts) and isinstance(order, np.ndarray) and order.dtype == np.int64
    assert np.array_equal(order, S.order(texts))
    assert M.sort_texts([])[0] == [] and M.sort_texts([b"x"])[1].tolist() == [0]
    sorted_batch, order = batch.sort()
    off, data = S.packed(sorted(texts))
    assert np.array_equal(_np(order), S.order(texts))
    assert np.array_equal(_np(sorted_batch.offsets), off) and np.array_equal(_np(sorted_batch.data), data)
    assert sorted_batch._end_offset == len(data) and sorted_batch._max_len == 70000
    # the host form of rank and totals
    lib = M.load_library()
    pdata, poff = M.pack_texts(texts)
    o, r = np.zeros(len(texts), np.int64), np.zeros(len(texts), np.int64)
    tot = (C.c_int64 * 1)(-7)
    assert lib.mrx_sort_batch(pdata.ctypes.data, poff.ctypes.data, len(texts), o.ctypes.data, r.ctypes.data,
                              C.cast(tot, C.c_void_p)) == M.api.MRX_OK
    want = S.expected(texts)
    assert np.array_equal(o, want[0]) and np.array_equal(r, want[1]) and tot[0] == want[2]


# ---- take --------------------------------------------------------------------------------------------------------------

def _raw_take(batch, index, out_data, cap, totals=True, pad=4):
    """The C call on the caller's own buffers: (rc, out_offsets with `pad` canaries, d_totals, host totals)."""
    import torch
    k = int(index.numel())
    off = torch.full((k + 1 + pad,), -9, dtype=torch.int64, device="cuda")
    dt = torch.full((2,), -9, dtype=torch.int64, device="cuda")
    ht = (C.c_int64 * 2)(-7, -7)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = batch.call(M.load_library(), "mrx_take", (),
                    (index.data_ptr() if k else None, k, off.data_ptr(), out_data.data_ptr(), cap, dt.data_ptr(),
                     C.cast(ht, C.c_void_p) if totals else None, stream))
    torch.cuda.synchronize()
    return rc, _np(off), _np(dt).tolist(), list(ht)


def _index(values):
    import torch
    return torch.tensor(list(values), dtype=torch.int64, device="cuda")


def _assert_taken(taken, want_texts, where):
    off, data = S.packed(want_texts)
    assert taken.offsets is not None and taken.n == len(want_texts), where
    assert np.array_equal(_np(taken.offsets), off), where
    assert np.array_equal(_np(taken.data), data), where


def test_take_in_every_order(edge_layouts):
    import torch
    lib = M.load_library()
    rng = np.random.default_rng(23)
    for lay, want in edge_layouts:
        batch, texts, n = lay.device(), lay.texts, len(lay.texts)
        picks = {
            "permutation": rng.permutation(n),
            "reversed": np.arange(n)[::-1].copy(),
            "repeats": rng.integers(0, n, size=n // 2),
            "more than n": np.concatenate([rng.integers(0, n, size=n), np.arange(n), [0, 0, n - 1]]),
            "sorted": want[0],
            "none": np.zeros(0, np.int64),
            "one": np.array([n - 1]),
        }
        for name, idx in picks.items():
            taken = batch.take(_index(idx))
            torch.cuda.synchronize()
            _assert_taken(taken, S.take(texts, idx), (lay.name, name))
            longest = batch.longest()
            assert taken._max_len == longest and taken._end_offset == (None if longest is None else int(taken.data.numel()))
            assert lib.mrx_debug_scratch_in_use() == 0
        assert S.take(texts, want[0]) == sorted(texts)
        name = lib.mrx_last_kernel_name()
        longest = batch.longest()
        assert name == (b"k_filter_gather_text" if longest is not None and longest <= 4096 else b"k_filter_gather"), lay.name


def test_take_through_both_byte_movers():
    import torch
    lib = M.load_library()
    rng = np.random.default_rng(29)
    texts = _edge_texts(big=False) + [b"x" * 5000, b"", b"y" * 4097]
    idx = np.concatenate([rng.permutation(len(texts)), rng.integers(0, len(texts), size=40)])
    want = S.take(texts, idx)
    batches = (M.DeviceBatch.from_texts(texts), LY.csr_shifted(texts, 7, _poison(6)).device(),
               LY.ragged_rows(texts, False, _poison(7)).device())
    try:
        for form, kernel in ((1, b"k_filter_gather"), (16, b"k_filter_gather_text")):
            lib.mrx_debug_filter_form(form)
            for batch in batches:
                taken = batch.take(_index(idx))
                torch.cuda.synchronize()
                assert lib.mrx_last_kernel_name() == kernel
                _assert_taken(taken, want, (form, batch.longest()))
    finally:
        lib.mrx_debug_filter_form(0)


def test_take_of_empty_texts_and_of_nothing():
    import torch
    batch = M.DeviceBatch.from_texts([b"", b"", b"abc", b""])
    taken = batch.take(_index([0, 3, 1, 1]))
    assert taken.n == 4 and _np(taken.offsets).tolist() == [0, 0, 0, 0, 0] and taken.data.numel() == 0
    none = batch.take(_index([]))
    assert none.n == 0 and _np(none.offsets).tolist() == [0] and none.data.numel() == 0
    buf = torch.full((8,), 0xA5, dtype=torch.uint8, device="cuda")
    got = _raw_take(batch, _index([]), buf, 8)
    assert got[0] == M.api.MRX_OK and got[1][0] == 0 and np.all(got[1][1:] == -9) and got[2] == [0, 0] and got[3] == [0, 0]
    got = _raw_take(batch, _index([1, 0]), buf, 0)   # an empty selection needs no capacity
    assert got[0] == M.api.MRX_OK and got[1][:3].tolist() == [0, 0, 0] and got[2] == [2, 0] and got[3] == [2, 0]
    assert np.all(_np(buf) == 0xA5)
    empty = M.DeviceBatch.from_texts([])
    assert empty.take(_index([])).n == 0
    with pytest.raises(M.MrxError):
        empty.take(_index([0]))
    assert M.load_library().mrx_debug_scratch_in_use() == 0


def test_take_capacity_totals_and_canaries():
    import torch
    lib = M.load_library()
    rng = np.random.default_rng(31)
    texts = [bytes(rng.integers(97, 123, size=int(rng.integers(1, 40))).tolist()) for _ in range(300)] + [b"", b"x" * 300, b""]
    idx = np.concatenate([rng.integers(0, len(texts), size=500), [len(texts) - 2, len(texts) - 1]])
    off, data = S.packed(S.take(texts, idx))
    nbytes, k = len(data), len(idx)
    assert nbytes > sum(len(t) for t in texts)   # repeats: the input's byte count is no bound
    for batch in (M.DeviceBatch.from_texts(texts), LY.csr_shifted(texts, 15, _poison(8)).device()):
        index = _index(idx)
        buf = torch.full((nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        got = _raw_take(batch, index, buf, nbytes - 1)   # one byte short: everything but the bytes
        assert got[0] == M.api.MRX_E_CAPACITY and got[3] == [k, nbytes] and got[2] == [k, nbytes]
        assert ("need %d" % nbytes).encode() in lib.mrx_last_error()
        assert np.array_equal(got[1][:k + 1], off) and np.all(got[1][k + 1:] == -9)
        assert np.all(_np(buf) == 0xA5)
        got = _raw_take(batch, index, buf, nbytes)
        assert got[0] == M.api.MRX_OK and got[3] == [k, nbytes] and got[2] == [k, nbytes]
        assert np.array_equal(got[1][:k + 1], off) and np.all(got[1][k + 1:] == -9)
        out = _np(buf)
        assert np.array_equal(out[:nbytes], data) and np.all(out[nbytes:] == 0xA5)
        # totals == NULL: nothing is read back, the device decides
        buf.fill_(0xA5)
        got = _raw_take(batch, index, buf, nbytes, totals=False)
        assert got[0] == M.api.MRX_OK and got[3] == [-7, -7] and got[2] == [k, nbytes]
        out = _np(buf)
        assert np.array_equal(out[:nbytes], data) and np.all(out[nbytes:] == 0xA5)
        buf.fill_(0xA5)
        got = _raw_take(batch, index, buf, nbytes - 1, totals=False)
        assert got[0] == M.api.MRX_OK and got[3] == [-7, -7] and got[2] == [k, nbytes] and np.all(_np(buf) == 0xA5)
        assert np.array_equal(got[1][:k + 1], off)
        with pytest.raises(M.MrxError):
            batch.take(index, out_cap=nbytes - 1)
        _assert_taken(batch.take(index, out_cap=nbytes), S.take(texts, idx), "exact capacity")
        _assert_taken(batch.take(index), S.take(texts, idx), "grown")   # starts at the input's bytes and grows
        outs = (torch.empty(k + 1, dtype=torch.int64, device="cuda"), torch.full((nbytes + 8,), 0xA5, dtype=torch.uint8, device="cuda"),
                torch.empty(2, dtype=torch.int64, device="cuda"))
        batch.take_async(index, outs)
        torch.cuda.synchronize()
        assert _np(outs[2]).tolist() == [k, nbytes] and np.array_equal(_np(outs[0]), off)
        assert np.array_equal(_np(outs[1])[:nbytes], data) and np.all(_np(outs[1])[nbytes:] == 0xA5)
    assert lib.mrx_debug_scratch_in_use() == 0


@pytest.mark.parametrize("bad", [-1, "n"])
def test_take_refuses_an_index_outside_the_batch(bad):
    import torch
    lib = M.load_library()
    texts = [b"abc", b"", b"defgh", b"ij"]
    bad = len(texts) if bad == "n" else bad
    for batch in (M.DeviceBatch.from_texts(texts), LY.ragged_rows(texts, True, _poison(9)).device()):
        index = _index([2, 0, bad, 1])
        buf = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
        got = _raw_take(batch, index, buf, 64)
        assert got[0] == M.api.MRX_E_ARGUMENT and got[2] == [-1, -1] and got[3] == [-1, -1]
        assert b"outside" in lib.mrx_last_error()
        assert np.all(_np(buf) == 0xA5) and np.all(got[1][5:] == -9)
        got = _raw_take(batch, index, buf, 64, totals=False)
        assert got[0] == M.api.MRX_OK and got[2] == [-1, -1] and got[3] == [-7, -7] and np.all(_np(buf) == 0xA5)
        with pytest.raises(M.MrxError):
            batch.take(index)
        assert lib.mrx_debug_scratch_in_use() == 0
        _assert_taken(batch.take(_index([2, 0, 1])), [b"defgh", b"abc", b""], "the next call")


def test_taken_batch_feeds_distinct_and_a_dictionary():
    rng = np.random.default_rng(37)
    texts = _edge_texts(big=False)
    batch = M.DeviceBatch.from_texts(texts)
    idx = rng.integers(0, len(texts), size=400)
    want = S.take(texts, idx)
    taken = batch.take(_index(idx))
    values, counts, _, _ = taken.distinct()
    raw, off = _np(values.data).tobytes(), _np(values.offsets)
    assert [(raw[off[g]:off[g + 1]], int(c)) for g, c in enumerate(_np(counts))] == list(Counter(want).items())
    entries = [b"a", b"", b"a\0", b"nothing like it", b"\xff", b"a"]
    where = {}
    for j, e in enumerate(entries):
        where.setdefault(e, j)
    got = M.Dictionary(entries).lookup(taken)
    assert _np(got).tolist() == [where.get(t, -1) for t in want]
    again, order = taken.sort()   # and sort takes a taken batch
    _assert_taken(again, sorted(want), "sorted twice")


@pytest.mark.parametrize("sort", [None, "value", "count"])
def test_value_counts_and_distinct_in_order(sort):
    pat = b"[a-z]+\\d+"
    texts = LY.make_texts(pat, 150, n_long=2) + [b"ab1 ab1 zz9 ab1", b"zz9 foo7 foo7 ab1 q0", b"", b"ab1"]
    rx = M.compile_regex(pat)
    pieces = [p for per_text in X.lists(X.expected_findall(pat, texts)) for p in per_text]
    plain = list(Counter(pieces).items())
    assert len(plain) < len(pieces) and len(plain) > 10
    batch = M.DeviceBatch.from_texts(texts)
    today = rx.value_counts(batch)
    for top in (None, 0, 3, 10 ** 9):
        want = S.value_counts(pieces, sort, top)
        if sort == "count":
            assert want == (Counter(pieces).most_common() if top is None else Counter(pieces).most_common(top))
        for b in (batch, LY.ragged_rows(texts, False, LY.pattern_poison(pat)).device()):
            values, counts = rx.value_counts(b, sort=sort, top=top)
            raw, off = _np(values.data).tobytes(), _np(values.offsets)
            assert [(raw[off[g]:off[g + 1]], int(c)) for g, c in enumerate(_np(counts))] == want, (sort, top)
            assert values.n == len(want) and counts.numel() == len(want)
        assert rx.value_counts(texts, sort=sort, top=top) == want
        assert M.value_counts(pat, texts, sort=sort, top=top) == want
        v, c, g, f = M.distinct(pieces, sort=sort, top=top)
        assert list(zip(v, c.tolist())) == want
        assert [pieces[i] for i in f] == v
        row = {value: r for r, value in enumerate(v)}
        assert g.tolist() == [row.get(p, -1) for p in pieces]
    import torch
    same = rx.value_counts(batch, sort=None)   # sort=None is today's result, tensor for tensor
    assert torch.equal(same[0].data, today[0].data) and torch.equal(same[0].offsets, today[0].offsets)
    assert torch.equal(same[1], today[1])
    assert rx.value_counts(texts) == plain
    with pytest.raises(M.MrxError):
        rx.value_counts(batch, sort="length")
