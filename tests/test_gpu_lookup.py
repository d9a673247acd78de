"""Dictionaries on the GPU against a Python dict (tests/lookup_expect.py): the lookup result, element for element, with
the entries and the probed batch each in every layout of tests/layouts.py; forced hash collisions and the mask a handle
keeps; agreement with distinct on the device; the filter's contract (include/mrx.h: capacity, canaries, asynchronous
form, sizes, scratch); and the merge of two chunks' value_counts, which is what dictionaries are for."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import mojo_regex_amd as M
import extract_expect as X
import layouts as LY
import lookup_expect as LE

pytestmark = pytest.mark.gpu

ALL_ONES = 0xFFFFFFFFFFFFFFFF


def _np(t):
    return t.cpu().numpy()


def _poison(seed=0):
    """distinct's poison (tests/test_gpu_distinct.py): bytes around the texts that would change an answer if they were read
    as text: zero bytes (a masked window reads as zeros: "a" against "a\\0"), the texts' own alphabet, and the text itself
    once more."""
    rng = np.random.default_rng(1000 + seed)

    def pz(i, t, k):
        if k <= 0:
            return b""
        kind = int(rng.integers(0, 3))
        fill = b"\0" * k if kind == 0 else bytes(rng.integers(97, 101, size=k).tolist()) if kind == 1 else (t + b"\0a") * k
        return fill[:k]
    return pz


def _edge_texts():
    """About 120 texts: lengths 0..49, a text and its proper prefix, pairs that differ in the last byte or by a trailing
    \\0 only, duplicates, and three 70 KB texts, two equal and one with another last byte.  Returns (texts, the 70 KB
    text, its near miss)."""
    rng = np.random.default_rng(4242)
    by_len = [bytes(rng.integers(97, 101, size=k).tolist()) for k in range(50)]          # lengths 0..49
    texts = list(by_len)
    texts += [b"", b"a", b"a\0", b"a\0\0", b"\0", b"\0\0", b"ab", b"abc", b"abd", b""]   # prefixes, NULs, last bytes
    texts += [t[:-1] + bytes([t[-1] ^ 1]) for t in by_len[15:19] + by_len[31:34] + by_len[47:50]]   # last byte differs
    texts += [t + b"\0" for t in (by_len[15], by_len[16], by_len[32], by_len[48])]        # a trailing NUL more
    texts += [by_len[k] for k in (0, 1, 7, 16, 17, 32, 33, 48, 49)]                       # duplicates at distance
    big = bytes(rng.integers(97, 123, size=70000).tolist())
    near = big[:-1] + b"!"
    texts += [big, b"a", near, b"", by_len[16]]
    texts += [bytes(rng.integers(97, 99, size=int(rng.integers(0, 4))).tolist()) for _ in range(20)]   # many repeats
    texts += [big, by_len[49], b"a\0"]
    assert 100 <= len(texts) <= 140
    return texts, big, near


def _entries_of(texts, big, near):
    """About half of the texts, every other one, so that of a pair that differs in its last byte or by a trailing NUL
    often only one is an entry; duplicates, the empty text and ONE of the 70 KB texts (not its near miss)."""
    entries = [t for k, t in enumerate(texts) if k % 2 == 0 and t not in (big, near)]
    entries += [big, b"", entries[3], entries[20], entries[3]]
    assert b"" in entries and near not in entries and len(set(entries)) < len(entries)
    assert 50 <= len(entries) <= 80
    return entries


@pytest.fixture(scope="module")
def edge():
    texts, big, near = _edge_texts()
    entries = _entries_of(texts, big, near)
    return {"texts": texts, "big": big, "near": near, "entries": entries,
            "probe_layouts": LY.layouts_for(texts, _poison()), "entry_layouts": LY.layouts_for(entries, _poison(1))}


def test_every_layout_on_both_sides(edge):
    import torch
    lib = M.load_library()
    probes = [(lay, lay.device()) for lay in edge["probe_layouts"]]
    names = {lay.name for lay, _ in probes}
    assert {"csr_packed", "csr_shift1", "csr_shift7", "csr_shift15", "rows48", "rows1001", "fixed64_len45"} <= names
    assert sum(n.startswith("lens") for n in names) == 2
    whole = 0
    for elay in edge["entry_layouts"]:
        d = M.Dictionary(elay.device())
        assert len(d) == len(elay.texts) and d.distinct_count == len(set(elay.texts)), elay.name
        for play, batch in probes:
            want = LE.expected(elay.texts, play.texts)
            got = d.lookup(batch)
            assert got.dtype == torch.int64 and got.is_cuda
            assert np.array_equal(_np(got), want), (elay.name, play.name)
            if (elay.csr or elay.lens is not None) and (play.csr or play.lens is not None):   # the texts themselves
                whole += 1
                at = {t: int(w) for t, w in zip(play.texts, want)}
                assert (want >= 0).sum() > 40 and (want < 0).sum() > 20
                assert at[edge["big"]] == elay.texts.index(edge["big"]) and at[edge["near"]] == -1
                assert at[b""] == elay.texts.index(b"")
        assert lib.mrx_debug_scratch_in_use() == 0
        del d
    assert whole == 36


def _small_case():
    rng = np.random.default_rng(8)
    vals = [bytes(rng.integers(97, 100, size=int(rng.integers(0, 20))).tolist()) for _ in range(150)]
    entries = [vals[int(k)] for k in rng.integers(0, 100, size=190)] + [b"", b"a", b"a\0", b"q" * 100, b"q" * 99 + b"r"]
    texts = [vals[int(k)] for k in rng.integers(0, 150, size=390)] + [b"", b"a\0\0", b"\0", b"q" * 100, b"q" * 99 + b"s"]
    assert len(entries) <= 200 and len(texts) <= 400 and len(set(entries)) > 60
    want = LE.expected(entries, texts)
    assert (want >= 0).sum() > 100 and (want < 0).sum() > 50
    return entries, texts, want


@pytest.mark.parametrize("mask", [0, 3])
def test_forced_collisions_change_nothing(mask):
    import torch
    lib = M.load_library()
    entries, texts, want = _small_case()
    ebatches = (M.DeviceBatch.from_texts(entries), LY.csr_shifted(entries, 7, _poison(2)).device())
    batches = (M.DeviceBatch.from_texts(texts), LY.ragged_rows(texts, False, _poison(3)).device())
    plain = [M.Dictionary(eb).lookup(b) for eb in ebatches for b in batches]
    try:
        lib.mrx_debug_distinct_hash_mask(mask)
        dicts = [M.Dictionary(eb) for eb in ebatches]
        masked = [d.lookup(b) for d in dicts for b in batches]
        kept = [d.filter(batches[0])[1] for d in dicts]
    finally:
        lib.mrx_debug_distinct_hash_mask(ALL_ONES)
    # the hook is back at its default: a handle built under the mask still answers, because it kept its mask
    later = [d.lookup(b) for d in dicts for b in batches]
    torch.cuda.synchronize()
    for a, b, c in zip(plain, masked, later):
        assert np.array_equal(_np(a), want) and torch.equal(a, b) and torch.equal(a, c), mask
    for k in kept:
        assert np.array_equal(_np(k), np.flatnonzero(want >= 0))
    assert all(d.distinct_count == len(set(entries)) for d in dicts)


def test_duplicates_and_determinism():
    import torch
    x, y = b"the one text", b"another"
    d = M.Dictionary([x, y, x, x])
    assert len(d) == 4 and d.distinct_count == 2
    assert d.lookup([x, y, x, b"", x + b"\0", x]).tolist() == [0, 1, 0, -1, -1, 0]
    entries, texts, want = _small_case()
    entries = entries * 5   # every entry five times: the lowest index stands for them
    batch = M.DeviceBatch.from_texts(texts)
    a, b = M.Dictionary(entries), M.Dictionary(entries)
    ra, rb, ra2 = a.lookup(batch), b.lookup(batch), a.lookup(batch)
    torch.cuda.synchronize()
    assert torch.equal(ra, rb) and torch.equal(ra, ra2) and np.array_equal(_np(ra), want)
    assert a.distinct_count == b.distinct_count == len(set(entries))


def _repeats(n, u, seed, lo=0, hi=24):
    rng = np.random.default_rng(seed)
    vals = list(dict.fromkeys(bytes(rng.integers(97, 123, size=int(rng.integers(lo, hi))).tolist()) for _ in range(4 * u)))[:u]
    assert len(vals) == u
    skew = np.minimum((rng.pareto(1.1, size=n) * 3).astype(np.int64), u - 1)   # a few values take most of the texts
    return [vals[int(k)] for k in skew[:n - u]] + vals   # (every value occurs)


@pytest.fixture(scope="module")
def skewed():
    texts = _repeats(5000, 1500, 3)
    values = list(dict.fromkeys(texts))
    assert len(values) == 1500
    return texts, values, LE.expected(values, texts)


def test_agrees_with_distinct_on_the_device(skewed):
    import torch
    texts, values, want = skewed
    batch = M.DeviceBatch.from_texts(texts)
    dvalues, _, group_of, _ = batch.distinct()
    got = M.Dictionary(dvalues).lookup(batch)
    assert torch.equal(got, group_of) and np.array_equal(_np(got), want)
    # the route the API offered before: the entries in front of the batch, distinct over the whole, and
    # first[group_of[m + i]] < m reads as "text i is an entry".  Here the dictionary holds only part of the values.
    part = values[1::3] + values[5:40]   # (with duplicates)
    m = len(part)
    _, _, g, first = M.DeviceBatch.from_texts(part + texts).distinct()
    f = first[g[m:]]
    route = torch.where(f < m, f, torch.full_like(f, -1))
    got = M.Dictionary(part).lookup(batch)
    assert torch.equal(got, route) and np.array_equal(_np(got), LE.expected(part, texts))
    assert 0 < int((got >= 0).sum()) < len(texts)


def test_several_rounds_per_wavefront(skewed):
    import torch
    lib = M.load_library()
    texts, values, want = skewed
    batches = (M.DeviceBatch.from_texts(texts), LY.csr_shifted(texts, 7, _poison(4)).device())
    assert batches[0]._max_len is not None and batches[1]._max_len is None
    try:
        lib.mrx_debug_distinct_grid(1)
        d = M.Dictionary(LY.csr_shifted(values, 15, _poison(5)).device())   # the build under the cap too
        for batch in batches:
            got = d.lookup(batch)
            assert lib.mrx_last_kernel_name() == b"k_dict_lookup"
            kept, idx = d.filter(batch)
            torch.cuda.synchronize()
            assert np.array_equal(_np(got), want)
            assert np.array_equal(_np(idx), np.arange(len(texts))) and kept.n == len(texts)
    finally:
        lib.mrx_debug_distinct_grid(0)
    assert np.array_equal(_np(d.lookup(batches[0])), want)


def test_hot_entry_and_all_misses():
    d = M.Dictionary([b"cold", b"the same text", b"colder"])
    got = _np(d.lookup(M.DeviceBatch.from_texts([b"the same text"] * 4096)))
    assert got.shape == (4096,) and np.all(got == 1)
    entries = [b"%09d" % (k * 7919) for k in range(3000)]
    texts = [b"%09d" % (k * 7919 + 1) for k in range(5000)]
    assert not set(entries) & set(texts)
    d = M.Dictionary(entries)
    assert np.all(_np(d.lookup(M.DeviceBatch.from_texts(texts))) == -1)
    assert np.array_equal(_np(d.lookup(M.DeviceBatch.from_texts(entries))), np.arange(3000))


def test_sizes():
    import torch
    none = M.Dictionary([])
    assert len(none) == 0 and none.distinct_count == 0
    batch = M.DeviceBatch.from_texts([b"a", b"", b"bc"])
    assert _np(none.lookup(batch)).tolist() == [-1, -1, -1]
    kept, idx = none.filter(batch)
    assert kept.n == 0 and idx.numel() == 0
    kept, idx = none.filter(batch, invert=True)
    assert _np(idx).tolist() == [0, 1, 2] and _np(kept.data).tobytes() == b"abc" and _np(kept.offsets).tolist() == [0, 1, 1, 3]
    d = M.Dictionary([b"a", b"bc"])
    empty = M.DeviceBatch.from_texts([])
    got = d.lookup(empty)
    assert got.numel() == 0 and got.dtype == torch.int64
    kept, idx = d.filter(empty)
    assert kept.n == 0 and _np(kept.offsets).tolist() == [0] and idx.numel() == 0
    assert none.lookup(empty).numel() == 0
    only_empty = M.Dictionary([b""])
    assert len(only_empty) == 1 and only_empty.distinct_count == 1
    assert _np(only_empty.lookup(M.DeviceBatch.from_texts([b"", b"a", b"\0", b""]))).tolist() == [0, -1, -1, 0]
    one = M.Dictionary([b"one entry"])
    assert _np(one.lookup(M.DeviceBatch.from_texts([b"one entry"]))).tolist() == [0]
    assert _np(one.lookup(M.DeviceBatch.from_texts([b"one entrz"]))).tolist() == [-1]
    assert M.lookup([], [b"a"]).tolist() == [-1] and M.lookup([b"a"], []).shape == (0,)
    assert M.load_library().mrx_debug_scratch_in_use() == 0


def _raw_filter(d, batch, out_data, cap, invert=False, totals=True, with_index=True, pad=8):
    """The C call on the caller's own buffers, each n-sized array with `pad` canary elements behind it: (rc, index or
    None, kept_idx, out_offsets, d_totals, host totals), the arrays with their canaries."""
    import torch
    dev, n = batch.data.device, batch.n
    index = torch.full((n + pad,), -9, dtype=torch.int64, device=dev) if with_index else None
    kept = torch.full((n + pad,), -9, dtype=torch.int64, device=dev)
    off = torch.full((n + 1 + pad,), -9, dtype=torch.int64, device=dev)
    dt = torch.full((2,), -9, dtype=torch.int64, device=dev)
    ht = (C.c_int64 * 2)(-7, -7)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = batch.call(M.load_library(), "mrx_dict_filter", (d._h, 1 if invert else 0),
                    (None if index is None else index.data_ptr(), kept.data_ptr(), off.data_ptr(), out_data.data_ptr(), cap,
                     dt.data_ptr(), C.cast(ht, C.c_void_p) if totals else None, stream))
    torch.cuda.synchronize()
    return rc, None if index is None else _np(index), _np(kept), _np(off), _np(dt).tolist(), list(ht)


def _assert_raw(got, want, want_index, n, pad):
    _, index, kept, off, dt, _ = got
    widx, woff, wdata = want
    k = len(widx)
    assert dt == [k, len(wdata)]
    assert np.array_equal(kept[:k], widx) and np.array_equal(off[:k + 1], woff)
    if index is not None:
        assert np.array_equal(index[:n], want_index)
    for a, size in ((index, n), (kept, n), (off, n + 1)):   # the canaries behind the n-sized arrays
        assert a is None or (len(a) == size + pad and np.all(a[size:] == -9))


def test_canaries_behind_the_index(edge):
    """d_index with 8 elements behind it stays untouched past n on every entry point."""
    import torch
    lib = M.load_library()
    texts, entries = edge["texts"], edge["entries"]
    d = M.Dictionary(entries)
    lays = {lay.name: lay for lay in edge["probe_layouts"]}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    seen = set()
    for name in ("csr_packed", "csr_shift7", "rows50", "fixed50_len37") + tuple(n for n in lays if n.startswith("lens")):
        lay = lays[name]
        batch, want = lay.device(), LE.expected(entries, lay.texts)
        n = batch.n
        index = torch.full((n + 8,), -9, dtype=torch.int64, device="cuda")
        assert batch.call(lib, (lib.mrx_dict_lookup_dev, lib.mrx_dict_lookup_strided_dev), (d._h,),
                          (index.data_ptr(), stream)) == M.api.MRX_OK
        torch.cuda.synchronize()
        got = _np(index)
        assert np.array_equal(got[:n], want) and np.all(got[n:] == -9), name
        seen.add("lookup_dev" if lay.csr else "lookup_strided_dev")
        buf = torch.empty(int(batch.data.numel()), dtype=torch.uint8, device="cuda")
        for invert in (False, True):
            res = _raw_filter(d, batch, buf, int(buf.numel()), invert=invert)
            assert res[0] == M.api.MRX_OK
            _assert_raw(res, LE.filtered(entries, lay.texts, invert), want, n, 8)
        seen.add("filter_strided_dev" if not lay.csr else "filter_known_dev" if lay.known else "filter_dev")
    assert seen == {"lookup_dev", "lookup_strided_dev", "filter_dev", "filter_known_dev", "filter_strided_dev"}


def test_filter_every_layout(edge):
    import torch
    lib = M.load_library()
    dicts = [(lay.texts, M.Dictionary(lay.device())) for lay in edge["entry_layouts"] if lay.name in ("csr_shift1", "rows48")]
    assert len(dicts) == 2
    for lay in edge["probe_layouts"]:
        batch = lay.device()
        n = batch.n
        for entries, d in dicts:
            sets = []
            for invert in (False, True):
                widx, woff, wdata = LE.filtered(entries, lay.texts, invert)
                kept, idx = d.filter(batch, invert=invert)
                torch.cuda.synchronize()
                where = (lay.name, invert)
                assert kept.offsets is not None and kept.n == len(widx), where
                assert np.array_equal(_np(idx), widx) and np.array_equal(_np(kept.offsets), woff), where
                assert np.array_equal(_np(kept.data), wdata), where
                # known bounds as CompiledRegex.filter sets them
                if not lay.csr and lay.lens is None:
                    assert kept._max_len == lay.length
                elif not lay.csr:
                    assert kept._max_len == lay.stride
                elif lay.known:
                    assert kept._max_len == max(len(t) for t in lay.texts)
                else:
                    assert kept._max_len is None and kept._end_offset is None
                if not lay.csr or lay.known:
                    assert kept._end_offset == len(wdata)
                sets.append(set(_np(idx).tolist()))
                # d_index given and NULL give the same output
                cap = int(batch.data.numel())
                bufs = [torch.full((cap + 16,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
                with_index = _raw_filter(d, batch, bufs[0], cap, invert=invert, with_index=True)
                without = _raw_filter(d, batch, bufs[1], cap, invert=invert, with_index=False)
                assert with_index[0] == without[0] == M.api.MRX_OK
                _assert_raw(with_index, (widx, woff, wdata), LE.expected(entries, lay.texts), n, 8)
                _assert_raw(without, (widx, woff, wdata), None, n, 8)
                assert torch.equal(bufs[0], bufs[1]) and np.all(_np(bufs[0])[len(wdata):] == 0xA5)
            assert sets[0] | sets[1] == set(range(n)) and not sets[0] & sets[1], lay.name
        assert lib.mrx_debug_scratch_in_use() == 0


def test_filter_capacity_and_asynchronous_form():
    import torch
    lib = M.load_library()
    texts = _repeats(900, 200, 11, lo=1, hi=40) + [b"", b"x" * 300, b""]
    entries = list(dict.fromkeys(texts))[::2] + [b"not there"]
    d = M.Dictionary(entries)
    want_index = LE.expected(entries, texts)
    want = LE.filtered(entries, texts)
    nbytes, n, pad = len(want[2]), len(texts), 8
    for batch in (M.DeviceBatch.from_texts(texts), LY.ragged_rows(texts, False, _poison(6)).device()):
        assert 0 < nbytes < batch.data.numel()
        # one byte short: MRX_E_CAPACITY, totals filled, indices and offsets complete, no byte written
        buf = torch.full((nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        got = _raw_filter(d, batch, buf, nbytes - 1, pad=pad)
        assert got[0] == M.api.MRX_E_CAPACITY and got[5] == [len(want[0]), nbytes]
        assert ("need %d" % nbytes).encode() in lib.mrx_last_error()
        _assert_raw(got, want, want_index, n, pad)
        assert np.all(_np(buf) == 0xA5)
        # exact capacity
        got = _raw_filter(d, batch, buf, nbytes, pad=pad)
        assert got[0] == M.api.MRX_OK and got[5] == [len(want[0]), nbytes]
        _assert_raw(got, want, want_index, n, pad)
        out = _np(buf)
        assert np.array_equal(out[:nbytes], want[2]) and np.all(out[nbytes:] == 0xA5)
        # totals == NULL: nothing on the host changes; fitting, and one byte short (the device decides)
        buf.fill_(0xA5)
        got = _raw_filter(d, batch, buf, nbytes, totals=False, pad=pad)
        assert got[0] == M.api.MRX_OK and got[5] == [-7, -7]
        _assert_raw(got, want, want_index, n, pad)
        out = _np(buf)
        assert np.array_equal(out[:nbytes], want[2]) and np.all(out[nbytes:] == 0xA5)
        buf.fill_(0xA5)
        got = _raw_filter(d, batch, buf, nbytes - 1, totals=False, pad=pad)
        assert got[0] == M.api.MRX_OK and got[5] == [-7, -7] and np.all(_np(buf) == 0xA5)
        _assert_raw(got, want, want_index, n, pad)
        # the Python form of the asynchronous call, with and without the index
        for index in (None, torch.full((n,), -9, dtype=torch.int64, device="cuda")):
            outs = (torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                    torch.empty(int(batch.data.numel()), dtype=torch.uint8, device="cuda"),
                    torch.empty(2, dtype=torch.int64, device="cuda"))
            d.filter_async(batch, outs, index=index)
            torch.cuda.synchronize()
            k = len(want[0])
            assert _np(outs[3]).tolist() == [k, nbytes] and np.array_equal(_np(outs[0])[:k], want[0])
            assert np.array_equal(_np(outs[1])[:k + 1], want[1]) and np.array_equal(_np(outs[2])[:nbytes], want[2])
            assert index is None or np.array_equal(_np(index), want_index)
        out = torch.full((n,), -9, dtype=torch.int64, device="cuda")
        d.lookup_async(batch, out)
        assert np.array_equal(_np(out), want_index)
    assert lib.mrx_debug_scratch_in_use() == 0


def test_filter_result_is_a_batch_like_any_other():
    texts = [b"ab1", b"zz", b"", b"ab1", b"q9 ab7", b"zz", b"x" * 70]
    d = M.Dictionary([b"zz", b"q9 ab7", b"ab1", b""])
    for batch in (M.DeviceBatch.from_texts(texts), LY.ragged_rows(texts, True, _poison(7)).device()):
        kept, idx = d.filter(batch)
        assert _np(idx).tolist() == [0, 1, 2, 3, 4, 5] and kept._max_len is not None
        again, idx2 = M.compile_regex(b"[a-z]+\\d").filter(kept)   # into a pattern's filter as it stands
        assert _np(idx2).tolist() == [0, 3, 4] and _np(again.data).tobytes() == b"ab1ab1q9 ab7"
        assert _np(M.Dictionary([b"ab1", b"nope"]).lookup(kept)).tolist() == [0, -1, -1, 0, -1, -1]   # and into a lookup
        assert _np(d.lookup(again)).tolist() == [2, 2, 1]


def test_merge_of_chunked_counts():
    """value_counts of a text list that arrives in two chunks, merged on the device: the first chunk's values become a
    dictionary, the second chunk's values are looked up in it, hits add their counts, misses are appended."""
    import torch
    pat = b"[a-z]+\\d+"
    texts = LY.make_texts(pat, 160, n_long=2) + [b"ab1 ab1 zz9 ab1", b"zz9 new5", b"", b"ab1"]
    half = len(texts) // 2
    rx = M.compile_regex(pat)
    v1, c1 = rx.value_counts(M.DeviceBatch.from_texts(texts[:half]))
    v2, c2 = rx.value_counts(M.DeviceBatch.from_texts(texts[half:]))
    d = M.Dictionary(v1)
    at = d.lookup(v2)
    hit = at >= 0
    counts = c1.clone()
    counts.index_add_(0, at[hit], c2[hit])
    missed, missed_at = d.filter(v2, invert=True)
    counts = torch.cat([counts, c2[missed_at]])
    data = torch.cat([v1.data, missed.data])
    offsets = torch.cat([v1.offsets, missed.offsets[1:] + v1.offsets[-1]])
    assert 0 < int(hit.sum()) < v2.n and missed.n == v2.n - int(hit.sum())
    raw, off = _np(data).tobytes(), _np(offsets)
    merged = [(raw[off[g]:off[g + 1]], int(c)) for g, c in enumerate(_np(counts))]
    pieces = [p for per_text in X.lists(X.expected_findall(pat, texts)) for p in per_text]
    want = Counter(pieces)
    assert dict(merged) == dict(want) and len(merged) == len(want)
    assert [v for v, _ in merged] == list(want)   # first-occurrence order of the whole list
    # and the merged values are a dictionary's entries in turn: all different
    assert M.Dictionary(M.DeviceBatch(data, offsets)).distinct_count == len(want)


def test_host_list_forms(edge):
    texts, entries = edge["texts"], edge["entries"]
    want = LE.expected(entries, texts)
    d = M.build_dictionary(entries)
    assert isinstance(d, M.Dictionary) and len(d) == len(entries) and d.distinct_count == len(set(entries))
    got = d.lookup(texts)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
    isin = d.isin(texts)
    assert isinstance(isin, np.ndarray) and isin.dtype == np.bool_ and np.array_equal(isin, want >= 0)
    dev = d.isin(M.DeviceBatch.from_texts(texts))
    assert dev.is_cuda and np.array_equal(_np(dev), want >= 0)
    for invert in (False, True):
        kept, idx = d.filter(texts, invert=invert)
        widx = LE.filtered(entries, texts, invert)[0]
        assert isinstance(idx, np.ndarray) and np.array_equal(idx, widx) and kept == [texts[int(i)] for i in widx]
    got = M.lookup(entries, texts)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
    assert M.lookup([s.decode() for s in (b"a", b"b")], ["b", "c"]).tolist() == [1, -1]
