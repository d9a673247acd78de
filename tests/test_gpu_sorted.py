"""The sorted index on the GPU against sorted(), bisect and startswith (tests/sorted_expect.py): all three modes, element for
element, with the entries and the probed batch each in every layout of tests/layouts.py; the index sizes at which a search
aid changes shape, with every combination of the aids; probe counts around a wavefront with the grid held to one
workgroup; canaries and NULL outputs; agreement with Dictionary, sort and argsort on the device; the asynchronous form and
two threads on one handle."""
import ctypes as C
import threading

import numpy as np
import pytest

import mojo_regex_amd as M
import layouts as LY
import sorted_expect as SX
from test_gpu_sort import _edge_texts, _poison

pytestmark = pytest.mark.gpu

MODES = (SX.EQUAL, SX.PREFIX, SX.LONGEST)
AIDS = (0, 1, 3)   # the plain search, the key array, the fence posts above it


def _np(t):
    return t.cpu().numpy()


def _near_misses(entries, rng):
    """Texts that are not entries (most of them): each entry with its last byte changed, one byte dropped, \\0 appended."""
    out = []
    for e in entries:
        kind = int(rng.integers(0, 3))
        if kind == 0 and e:
            out.append(e[:-1] + bytes([e[-1] ^ (1 << int(rng.integers(0, 8)))]))
        elif kind == 1 and e:
            k = int(rng.integers(0, len(e)))
            out.append(e[:k] + e[k + 1:])
        else:
            out.append(e + b"\0")
    return out


def _raw_search(ix, batch, mode, lo=True, hi=True, pad=4):
    """The C call on the caller's own buffers, each with `pad` canary elements behind it: (rc, lo, hi)."""
    import torch
    n = batch.n
    d_lo = torch.full((n + pad,), -9, dtype=torch.int64, device="cuda")
    d_hi = torch.full((n + pad,), -9, dtype=torch.int64, device="cuda")
    lib = M.load_library()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = batch.call(lib, (lib.mrx_sorted_search_dev, lib.mrx_sorted_search_strided_dev), (ix._h, mode),
                    (d_lo.data_ptr() if lo else None, d_hi.data_ptr() if hi else None, stream))
    torch.cuda.synchronize()
    return rc, _np(d_lo), _np(d_hi)


def _assert_modes(ix, batch, want, where):
    """Every mode of `batch` against want[mode] = (lo, hi), through the class."""
    for mode in MODES:
        lo, hi = ix._search(batch, mode)
        assert np.array_equal(_np(lo), want[mode][0]), (where, mode, "lo")
        assert np.array_equal(_np(hi), want[mode][1]), (where, mode, "hi")


def _expect(entries, texts):
    return {mode: SX.search(entries, texts, mode) for mode in MODES}


@pytest.fixture(scope="module")
def edge():
    texts = _edge_texts()
    rng = np.random.default_rng(61)
    entries = texts[::2]
    big = max(texts, key=len)
    if big not in entries:
        entries.append(big)
    probes = texts + _near_misses(entries, rng) + _near_misses(texts[1::2], rng)
    assert 70 <= len(entries) <= 90 and 280 <= len(probes) <= 340
    assert len(big) == 70000 and big[:-1] + b"!" in probes and probes.count(big) >= 2
    return entries, probes


def test_edge_texts_with_the_entries_in_every_layout(edge):
    lib = M.load_library()
    entries, probes = edge
    batch = M.DeviceBatch.from_texts(probes)
    names = set()
    for lay in LY.layouts_for(entries, _poison(20)):
        names.add(lay.name)
        ix = M.SortedIndex(lay.device())
        want = _expect(lay.texts, probes)
        _assert_modes(ix, batch, want, lay.name)
        assert len(ix) == len(lay.texts) and ix.distinct_count == len(set(lay.texts)), lay.name
        assert np.array_equal(_np(ix.order), SX.order(lay.texts)), lay.name
        assert lib.mrx_last_kernel_name() == b"k_sorted_search"
        assert lib.mrx_debug_scratch_in_use() == 0
        if lay.csr or lay.lens is not None:   # the texts themselves: hits, misses and the long twins
            lo, hi = want[SX.EQUAL]
            assert (hi > lo).sum() > 70 and (hi == lo).sum() > 100 and (hi - lo).max() >= 2
            assert (want[SX.LONGEST][1] == 70000).sum() >= 2 and (want[SX.LONGEST][0] < 0).sum() == 0   # b"" is an entry
    assert {"csr_packed", "csr_shift1", "csr_shift7", "csr_shift15", "rows48", "fixed64_len45"} <= names and len(names) == 12


def test_edge_texts_with_the_probes_in_every_layout(edge):
    lib = M.load_library()
    entries, probes = edge
    ix = M.SortedIndex(entries)
    try:
        for lay in LY.layouts_for(probes, _poison(21)):
            want = _expect(entries, lay.texts)
            batch = lay.device()
            for aids in AIDS:
                assert lib.mrx_debug_sorted_aids(aids) == aids
                _assert_modes(ix, batch, want, (lay.name, aids))
    finally:
        lib.mrx_debug_sorted_aids(-1)
    assert lib.mrx_debug_scratch_in_use() == 0


def _three_letters(m, rng):
    return [bytes(rng.integers(97, 100, size=int(rng.integers(0, 13))).tolist()) for _ in range(m)]


def _aid_cases():
    rng = np.random.default_rng(67)
    cases = {"m%d" % m: _three_letters(m, rng) for m in (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4097)}
    cases["equal200"] = [b"one and the same text"] * 200
    prefix = bytes(rng.integers(0, 256, size=100).tolist())
    cases["prefix100_300"] = [prefix + bytes(rng.choice((0, 1, 97, 0x7f, 0x80, 0xff), size=int(rng.integers(0, 12))).tolist())
                              for _ in range(300)]
    return cases, rng


@pytest.mark.parametrize("name", ["m0", "m1", "m2", "m63", "m64", "m65", "m1023", "m1024", "m1025", "m4097", "equal200",
                                  "prefix100_300"])
def test_index_sizes_at_which_a_search_aid_changes_shape(name):
    lib = M.load_library()
    cases, rng = _aid_cases()
    entries = cases[name]
    pool = entries[:150] + _near_misses(entries[:120], rng) + _three_letters(60, rng)
    pool += [b"", b"a", b"abcabcab", b"abcabcabc", b"cccccccccccc", b"d", b"one and the same text", b"one and the same tex",
             b"one and the same text\0"]
    if name == "prefix100_300":
        pool += [entries[0][:100], entries[0][:99], entries[0][:96], entries[0][:100] + b"\xff\xff"]
    want = _expect(entries, pool)
    if name in ("m1024", "m4097"):   # duplicates, prefixes and long runs of equal first words all occur
        assert len(set(entries)) < len(entries) and (want[SX.PREFIX][1] - want[SX.PREFIX][0]).max() > 64
    batch = M.DeviceBatch.from_texts(pool)
    ix = M.SortedIndex(entries)
    assert len(ix) == len(entries) and ix.distinct_count == len(set(entries))
    assert np.array_equal(_np(ix.order), SX.order(entries))
    got = {}
    try:
        for aids in AIDS:
            assert lib.mrx_debug_sorted_aids(aids) == aids
            _assert_modes(ix, batch, want, (name, aids))
            got[aids] = [_raw_search(ix, batch, mode) for mode in MODES]
    finally:
        lib.mrx_debug_sorted_aids(-1)
    for aids in AIDS[1:]:   # both aid switches on and off: identical arrays, canaries included
        for a, b in zip(got[0], got[aids]):
            assert a[0] == b[0] == M.api.MRX_OK and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    if not entries:
        assert np.all(want[SX.EQUAL][0] == 0) and np.all(want[SX.PREFIX][1] == 0) and np.all(want[SX.LONGEST][0] == -1)
    assert lib.mrx_debug_scratch_in_use() == 0


@pytest.fixture(scope="module")
def counted():
    rng = np.random.default_rng(71)
    entries = _three_letters(300, rng)
    probes = (_three_letters(3000, rng) + entries + _near_misses(entries, rng) * 2 + [b""] * 197)[:4097]
    assert len(probes) == 4097
    return entries, probes, _expect(entries, probes)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_probe_counts_with_one_workgroup_and_canaries(counted, n):
    import torch
    lib = M.load_library()
    entries, probes, want = counted
    ix = M.SortedIndex(entries)
    batch = M.DeviceBatch.from_texts(probes[:n])
    try:
        lib.mrx_debug_sorted_grid(1)   # 256 lanes: 4097 probes are 17 rounds of the stride loop
        for aids in AIDS:
            lib.mrx_debug_sorted_aids(aids)
            for mode in MODES:
                for lo, hi in ((True, True), (True, False), (False, True)):   # each output as NULL in turn
                    rc, got_lo, got_hi = _raw_search(ix, batch, mode, lo, hi)
                    assert rc == M.api.MRX_OK
                    assert np.array_equal(got_lo[:n], want[mode][0][:n]) if lo else np.all(got_lo[:n] == -9), (n, aids, mode)
                    assert np.array_equal(got_hi[:n], want[mode][1][:n]) if hi else np.all(got_hi[:n] == -9), (n, aids, mode)
                    assert np.all(got_lo[n:] == -9) and np.all(got_hi[n:] == -9) and len(got_lo) == n + 4
        rc, _, _ = _raw_search(ix, batch, SX.EQUAL, False, False)
        assert rc == (M.api.MRX_E_ARGUMENT if n else M.api.MRX_OK)   # not both, unless there is nothing to write
    finally:
        lib.mrx_debug_sorted_grid(0)
        lib.mrx_debug_sorted_aids(-1)
    if n:
        left = ix.searchsorted(batch)
        right = ix.searchsorted(batch, side="right")
        assert torch.equal(left, ix.equal_range(batch)[0]) and torch.equal(right, ix.equal_range(batch)[1])
        assert np.array_equal(_np(left), want[SX.EQUAL][0][:n]) and np.array_equal(_np(right), want[SX.EQUAL][1][:n])
    assert lib.mrx_debug_scratch_in_use() == 0


def test_index_agrees_with_dictionary_sort_and_argsort(edge):
    import torch
    entries, probes = edge
    ebatch = M.DeviceBatch.from_texts(entries)
    pbatch = M.DeviceBatch.from_texts(probes)
    ix = M.SortedIndex(ebatch)
    # the lowest original index of an equal entry: a dictionary's answer, element for element
    got = ix.index(pbatch)
    assert torch.equal(got, M.Dictionary(ebatch).lookup(pbatch))
    assert _np(got).tolist() == SX.index(entries, probes) and (got >= 0).sum() > 70
    assert ix.index(probes[:50]).tolist() == SX.index(entries, probes[:50])
    # the sorted entries: sort's batch, byte for byte
    srt, order = ebatch.sort()
    assert torch.equal(ix.order, order)
    assert torch.equal(ix.values.data, srt.data) and torch.equal(ix.values.offsets, srt.offsets) and ix.values is ix.values
    # the entries among themselves: the dense ranks' group bounds
    order, rank, u = ebatch.argsort(rank=True)
    counts = torch.bincount(rank, minlength=u)
    starts = torch.cumsum(counts, 0) - counts
    lo, hi = ix.equal_range(ebatch)
    assert torch.equal(lo, starts[rank]) and torch.equal(hi, starts[rank] + counts[rank]) and u == ix.distinct_count
    assert torch.equal(ix.searchsorted(ebatch), lo) and torch.equal(ix.searchsorted(ebatch, side="right"), hi)


def test_route_table_and_host_forms():
    routes = [b"/", b"/api/", b"/api/v2/", b"/static/", b"/static/img/", b"/api/v2/users", b"/api/"]
    paths = [b"/api/v2/users/17", b"/api/v2/user", b"/api/v1/x", b"/static/img/a.png", b"/static", b"/", b"", b"api/",
             b"/api/v2/users", b"/api/v2/", b"/zzz", b"/static/\xff"]
    ix = M.build_sorted_index(routes)
    srt = sorted(routes)
    pos, length = ix.longest_prefix(paths, lengths=True)
    assert isinstance(pos, np.ndarray) and pos.dtype == np.int64 and length.dtype == np.int64
    for p, n, path in zip(pos.tolist(), length.tolist(), paths):
        cands = [r for r in routes if path.startswith(r)]
        if not cands:
            assert (p, n) == (-1, -1), path
        else:
            best = max(cands, key=len)
            assert srt[p] == best and n == len(best) and p == srt.index(best), path
    assert np.array_equal(ix.longest_prefix(paths), pos)
    assert ix.longest_prefix(paths).tolist() == SX.search(routes, paths, SX.LONGEST)[0].tolist()
    lo, hi = ix.prefix_range([b"/api/", b"/static", b"/q", b""])
    assert lo.tolist() == [1, 5, 5, 0] and hi.tolist() == [5, 7, 5, 7]
    assert [srt[p] for p in range(1, 5)] == [b"/api/", b"/api/", b"/api/v2/", b"/api/v2/users"]
    # a time window of a sorted log: two searchsorted calls and a slice
    log = [b"2026-10-21T06:%02d:00 event %d" % (k, k) for k in range(0, 60, 7)]
    stamps = M.SortedIndex([line[:19] for line in log])
    a, b = stamps.searchsorted([b"2026-10-21T06:10", b"2026-10-21T06:30"]).tolist()
    assert log[a:b] == [line for line in log if b"2026-10-21T06:10" <= line[:19] < b"2026-10-21T06:30"] and b - a == 3
    # module level, through mrx_sorted_search_batch
    entries = [b"b", b"", b"a\0", b"a", b"\x80", b"a", b"\x7f"]
    texts = [b"a", b"", b"a\0\0", b"\x7f\x01", b"\xff", b"b"]
    want = SX.search(entries, texts, SX.EQUAL)
    assert np.array_equal(M.searchsorted(entries, texts), want[0])
    assert np.array_equal(M.searchsorted(entries, texts, side="right"), want[1])
    assert M.searchsorted([], texts).tolist() == [0] * 6 and M.searchsorted(entries, []).shape == (0,)
    with pytest.raises(M.MrxError):
        ix.searchsorted(paths, side="middle")
    # no entry: a valid handle
    none = M.SortedIndex([])
    assert len(none) == 0 and none.distinct_count == 0 and none.order.numel() == 0 and none.values.n == 0
    assert [a.tolist() for a in none.equal_range(texts)] == [[0] * 6, [0] * 6]
    assert [a.tolist() for a in none.prefix_range(texts)] == [[0] * 6, [0] * 6]
    assert [a.tolist() for a in none.longest_prefix(texts, lengths=True)] == [[-1] * 6, [-1] * 6]
    assert none.index(texts).tolist() == [-1] * 6
    assert M.load_library().mrx_debug_scratch_in_use() == 0


def test_search_async_takes_no_scratch_and_reads_nothing_back(counted):
    import torch
    lib = M.load_library()
    entries, probes, want = counted
    ix = M.SortedIndex(entries)
    batch = M.DeviceBatch.from_texts(probes)
    lo = torch.full((len(probes) + 4,), -9, dtype=torch.int64, device="cuda")
    hi = torch.full((len(probes) + 4,), -9, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    size0 = lib.mrx_debug_scratch_bytes()
    for mode, name in zip(MODES, ("equal", "prefix", "longest")):
        ix.search_async(batch, name, lo, hi)
        assert lib.mrx_debug_scratch_in_use() == 0 and lib.mrx_debug_scratch_bytes() == size0
        torch.cuda.synchronize()
        assert np.array_equal(_np(lo)[:-4], want[mode][0]) and np.array_equal(_np(hi)[:-4], want[mode][1])
        assert np.all(_np(lo)[-4:] == -9) and np.all(_np(hi)[-4:] == -9)
    ix.search_async(batch, M.api.MRX_SORTED_PREFIX, None, hi)
    torch.cuda.synchronize()
    assert np.array_equal(_np(hi)[:-4], want[SX.PREFIX][1]) and np.array_equal(_np(lo)[:-4], want[SX.LONGEST][0])
    with pytest.raises(M.MrxError):
        ix.search_async(batch, "equal", None, None)
    with pytest.raises(M.MrxError):
        ix.search_async(batch, "equal", lo[:10], hi)


def test_two_threads_on_two_streams_search_one_handle(counted):
    import torch
    entries, probes, want = counted
    ix = M.SortedIndex(entries)
    batch = M.DeviceBatch.from_texts(probes)
    torch.cuda.synchronize()
    results, errors = {}, []

    def work(k):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                got = []
                for _ in range(5):
                    got = [ix._search(batch, mode) for mode in MODES]
                stream.synchronize()
                results[k] = [(_np(lo), _np(hi)) for lo, hi in got]
        except Exception as e:   # a thread's assertion must reach the test
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and sorted(results) == [0, 1]
    for k in range(2):
        for mode, (lo, hi) in zip(MODES, results[k]):
            assert np.array_equal(lo, want[mode][0]) and np.array_equal(hi, want[mode][1]), (k, mode)


def test_order_needs_its_array_unless_there_is_no_entry():
    import torch
    lib = M.load_library()
    ix = M.SortedIndex([b"b", b"a", b"b"])
    assert lib.mrx_sorted_order_dev(ix._h, None, None) == M.api.MRX_E_ARGUMENT
    order = torch.full((3 + 4,), -9, dtype=torch.int64, device="cuda")
    assert lib.mrx_sorted_order_dev(ix._h, order.data_ptr(), None) == M.api.MRX_OK
    torch.cuda.synchronize()
    assert _np(order).tolist() == [1, 0, 2, -9, -9, -9, -9]
    none = M.SortedIndex([])
    assert lib.mrx_sorted_order_dev(none._h, None, None) == M.api.MRX_OK
