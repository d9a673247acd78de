"""extract on the GPU against the oracle (tests/extract_expect.py): the piece CSR over the texts, the owners, the output
CSR and the output bytes, bit for bit -- findall's matches for every pattern of tests/layouts.py on every layout, the
primitive on hand-made spans (alignment sweep, empty pieces, several rounds per wavefront, the clamp), split_batch,
PatternSet.extract, and the edges of the contract in include/mrx.h (capacities, canaries, asynchronous form, scratch,
chaining).

Every parity batch is asserted to hold a non-empty piece and a text without a piece, but for the cases the filter test
names too: `x*`, `.*` and `a+b*` (the reference answers all three with a match in every text, the empty one included,
so no text is without a piece), and `^abc$` on the layouts whose texts share one length other than 3 (no piece at
all; it gets a fixed-length layout of length 3 of its own)."""
import ctypes as C

import numpy as np
import pytest

import mojo_regex_amd as M
import captures_all_expect as CA
import extract_expect as X
import layouts as LY
import test_gpu_filter as TF
import test_gpu_pattern_set as PS

pytestmark = pytest.mark.gpu

OK, CAPACITY = M.api.MRX_OK, M.api.MRX_E_CAPACITY


def _np(t):
    return t.cpu().numpy()


def _assert_result(res, want, where):
    pieces, prefix, owner = res
    wprefix, wowner, woff, wdata = want
    assert pieces.offsets is not None and pieces.n == len(wowner), where
    assert np.array_equal(_np(prefix), wprefix), where
    assert np.array_equal(_np(owner), wowner), where
    assert np.array_equal(_np(pieces.offsets), woff), where
    assert np.array_equal(_np(pieces.data), wdata), where
    assert pieces._end_offset in (None, len(wdata)), where


def _scratch_is_returned():
    assert M.load_library().mrx_debug_scratch_in_use() == 0


@pytest.mark.parametrize("pat", LY.PATTERNS, ids=[p.decode() for p in LY.PATTERNS])
def test_one_pattern_on_every_layout(pat):
    import torch
    rx = M.compile_regex(pat)
    texts = LY.make_texts(pat, 90, n_long=3) + TF.CANNOT + TF.SURE + [b""]
    row_texts = texts + TF.LONG_ROWS
    cache = {}
    lays = LY.layouts_for(texts, LY.pattern_poison(pat), row_texts)
    if pat == b"^abc$":
        lays.append(LY.fixed_length(row_texts, 16, 3, LY.pattern_poison(pat, 1)))
        lays[-1].check()
    for lay in lays:
        batch = lay.device()
        try:
            rx.match_all(batch)
        except M.UnsupportedPattern as e:
            with pytest.raises(M.UnsupportedPattern) as ei:
                rx.extract(batch)
            assert str(ei.value) == str(e)
            continue
        want = X.expected_findall(pat, lay.texts, cache)
        rows = np.diff(want[0])
        if pat in TF.MATCH_EVERY_TEXT:
            assert rows.min() > 0 and len(want[3]) > 0
        elif pat == b"^abc$" and not lay.csr and lay.lens is None and lay.length != 3:
            assert rows.max() == 0
        else:
            assert len(want[3]) > 0 and rows.min() == 0, (pat, lay.name)
        res = rx.extract(batch)
        torch.cuda.synchronize()
        _assert_result(res, want, (pat, lay.name))
        _scratch_is_returned()
        if not lay.csr and lay.lens is None:
            assert res[0]._max_len == lay.length
        elif lay.known:
            assert res[0]._max_len == max(len(t) for t in lay.texts)
        if not lay.csr or lay.known:
            assert res[0]._end_offset == len(want[3])


def _raw_gather(batch, prefix, spans, pair, piece_cap, out, out_cap, totals=True, canary=0):
    """mrx_gather_spans_* on the caller's buffers: (rc, owner, out_offsets, d_totals, host totals).  owner and
    out_offsets have `canary` more elements than the capacity says."""
    import torch
    lib = M.load_library()
    owner = torch.full((max(piece_cap, 1) + canary,), -9, dtype=torch.int64, device="cuda")
    off = torch.full((piece_cap + 1 + canary,), -9, dtype=torch.int64, device="cuda")
    dt = torch.full((2,), -9, dtype=torch.int64, device="cuda")
    ht = (C.c_int64 * 2)(-7, -7)
    row_pairs = int(spans.shape[1]) if spans.dim() == 3 else 1
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = batch.call(lib, "mrx_gather_spans", (),
                    (prefix.data_ptr(), spans.data_ptr(), row_pairs, pair, piece_cap, owner.data_ptr(), off.data_ptr(),
                     out.data_ptr(), out_cap, dt.data_ptr(), C.cast(ht, C.c_void_p) if totals else None, stream))
    torch.cuda.synchronize()
    return rc, _np(owner), _np(off), _np(dt).tolist(), list(ht)


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


SWEEP_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 47)


def test_alignment_sweep_on_the_primitive():
    import torch
    text = bytes((37 * k + 11) % 251 for k in range(200))
    rows = [(s, s + k) for s in range(16) for k in SWEEP_LENGTHS]
    want = X.pack([rows], [text])
    nbytes = len(want[3])
    batch = M.DeviceBatch.from_texts([text])
    prefix, spans = _dev(want[0], np.int64), _dev(rows, np.int32)
    for skew in range(16):
        buf = torch.full((16 + skew + nbytes + 48,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        rc, owner, off, dt, ht = _raw_gather(batch, prefix, spans, 0, len(rows), buf[16 + skew:], nbytes)
        assert rc == OK and dt == [len(rows), nbytes] and ht == dt, skew
        got = _np(buf)
        assert np.all(got[:16 + skew] == 0xA5) and np.all(got[16 + skew + nbytes:] == 0xA5), skew
        assert np.array_equal(got[16 + skew:16 + skew + nbytes], want[3]), skew
        assert np.array_equal(owner[:len(rows)], want[1]) and np.array_equal(off, want[2]), skew
    _scratch_is_returned()


def test_empty_pieces_and_texts_without_rows():
    import torch
    rng = np.random.default_rng(5)
    texts = [bytes(rng.integers(1, 255, size=int(k)).tolist()) for k in rng.integers(20, 60, size=80)]
    rows = [[] for _ in texts]
    # no rows at the start (texts 0, 1), in the middle (a run of 70) and at the end (the last two)
    rows[2] = [(0, 7)] + [(3, 3)] * 200 + [(5, 19)]          # 200 empty pieces between two non-empty ones
    rows[3] = [(1, 2), (0, 0), (-1, -1), (9, 4), (2, 20)]
    rows[74] = [(0, len(texts[74]))]
    rows[77] = [(4, 4), (0, 1)]
    want = X.pack(rows, texts)
    for lay in (LY.csr_packed(texts), LY.csr_shifted(texts, 7, lambda i, t, k: b"\xEE" * k),
                LY.ragged_rows(texts, False, lambda i, t, k: b"\xEE" * k)):
        batch = lay.device()
        spans = _dev([p for r in rows for p in r], np.int32)
        pieces, owner = batch.gather_spans(_dev(want[0], np.int64), spans)
        _assert_result((pieces, _dev(want[0], np.int64), owner), want, lay.name)
    # n = 1, n = 0, pieces = 0
    one = M.DeviceBatch.from_texts([b"hello world"])
    pieces, owner = one.gather_spans(_dev([0, 2], np.int64), _dev([(6, 11), (0, 5)], np.int32))
    assert _np(pieces.data).tobytes() == b"worldhello" and _np(pieces.offsets).tolist() == [0, 5, 10]
    assert _np(owner).tolist() == [0, 0]
    none = torch.zeros((0, 2), dtype=torch.int32, device="cuda")
    pieces, owner = one.gather_spans(_dev([0, 0], np.int64), none)
    assert pieces.n == 0 and _np(pieces.offsets).tolist() == [0] and pieces.data.numel() == 0 and owner.numel() == 0
    pieces, owner = M.DeviceBatch.from_texts([]).gather_spans(_dev([0], np.int64), none)
    assert pieces.n == 0 and _np(pieces.offsets).tolist() == [0] and owner.numel() == 0
    d = torch.zeros(16, dtype=torch.uint8, device="cuda")
    rc, _, off, dt, ht = _raw_gather(M.DeviceBatch.from_texts([]), _dev([0], np.int64), none, 0, 0, d, 0)
    assert rc == OK and off.tolist() == [0] and dt == [0, 0] and ht == [0, 0]
    rx = M.compile_regex(b"\\d+")
    pieces, prefix, owner = rx.extract(M.DeviceBatch.from_texts([]))
    assert pieces.n == 0 and _np(prefix).tolist() == [0] and _np(pieces.offsets).tolist() == [0]
    assert rx.extract([]) == [] and rx.extract([b"", b"ab"]) == [[], []]
    _scratch_is_returned()


def test_several_rounds_per_wavefront():
    lib = M.load_library()
    rng = np.random.default_rng(9)
    big = bytes(rng.integers(0, 256, size=100 << 10, dtype=np.uint8).tolist())
    small = [bytes(rng.integers(97, 123, size=40).tolist()) for _ in range(300)]
    texts = small[:150] + [big] + small[150:]
    rows = [[(3, 9), (9, 9), (20, 26)] for _ in small[:150]] + [[(0, len(big))]] + [[(1, 7)] for _ in small[150:]]
    want = X.pack(rows, texts)
    batch = M.DeviceBatch.from_texts(texts)
    prefix, spans = _dev(want[0], np.int64), _dev([p for r in rows for p in r], np.int32)
    lib.mrx_debug_extract_grid(1)   # 4 wavefronts: about 26 rounds of 64 blocks each
    try:
        pieces, owner = batch.gather_spans(prefix, spans)
        assert lib.mrx_last_kernel_name() == b"k_extract_gather"
        _assert_result((pieces, prefix, owner), want, "one workgroup")
    finally:
        lib.mrx_debug_extract_grid(0)
    pieces, owner = batch.gather_spans(prefix, spans)
    _assert_result((pieces, prefix, owner), want, "full grid")
    _scratch_is_returned()


@pytest.mark.parametrize("pat", [b"x(\\d)?", b"(\\d+)|([a-z]+)|(-)"])
def test_clamp_on_captures_all_rows(pat):
    rx = M.compile_regex(pat)
    g = rx.num_groups
    assert g == CA.num_groups(pat)
    texts = [b"x", b"x5x", b"", b"ab12-x", b"xx7x", b"--", b"9x"] * 5 + [b"x1" * 40 + b"x"]
    for lay in (LY.csr_packed(texts), LY.ragged_rows(texts, False, lambda i, t, k: b"7" * k)):
        batch = lay.device()
        mprefix, groups = rx.captures_all(batch)
        assert groups.shape[1] == g + 1
        for group in range(g + 1):
            want = X.expected_group(pat, lay.texts, group)
            pieces, owner = batch.gather_spans(mprefix, groups, pair=X.group_pair(group, g))
            _assert_result((pieces, mprefix, owner), want, (pat, lay.name, group))
            _assert_result(rx.extract(batch, group=group), want, (pat, lay.name, group, "extract"))
        assert rx.extract(lay.texts, group=1, count=1) == X.lists(X.expected_group(pat, lay.texts, 1, 1))
    unset = X.expected_group(pat, texts, g)
    assert np.any(np.diff(unset[2]) == 0) and len(unset[3]) > 0   # some empty pieces, some bytes
    with pytest.raises(M.MrxError):
        rx.extract(texts, group=g + 1)
    with pytest.raises(M.MrxError):
        rx.extract(texts, count=1)
    _scratch_is_returned()


def test_split_batch_and_pattern_set_extract():
    pat = b"[ ,]+"
    rx = M.compile_regex(pat)
    texts = LY.make_texts(pat, 120, n_long=2) + [b"", b",", b"a,b , c", b",,a"]
    batch = M.DeviceBatch.from_texts(texts)
    cache = {}
    for maxsplit in (0, 2, -1):
        res = rx.split_batch(batch, maxsplit)
        _assert_result(res, X.expected_split(pat, texts, maxsplit, cache), maxsplit)
        raw, off, pre = _np(res[0].data).tobytes(), _np(res[0].offsets), _np(res[1])
        got = [[raw[off[r]:off[r + 1]] for r in range(pre[i], pre[i + 1])] for i in range(len(texts))]
        assert got == rx.split(texts, maxsplit), maxsplit
    _scratch_is_returned()
    small = PS._texts(17, 300)
    sbatch = M.DeviceBatch.from_texts(small)
    for name in ("mixed7", "gen64"):
        s = M.compile_set(PS.SETS[name])
        hits = s.findall_lists(small)
        want = [[(m, t[a:b]) for m, a, b in row] for row, t in zip(hits, small)]
        assert s.extract(small) == want, name
        pieces, tprefix, members, owner = s.extract(sbatch)
        flat = [p for row in want for p in row]
        assert pieces.n == len(flat) and _np(members).tolist() == [m for m, _ in flat]
        assert _np(pieces.data).tobytes() == b"".join(p for _, p in flat)
        assert np.array_equal(_np(owner), np.repeat(np.arange(len(small)), np.diff(_np(tprefix))))
    _scratch_is_returned()


def _raw_extract(rx, batch, piece_cap, out, out_cap, totals=True, canary=0):
    import torch
    prefix = torch.full((batch.n + 1,), -9, dtype=torch.int64, device="cuda")
    owner = torch.full((max(piece_cap, 1) + canary,), -9, dtype=torch.int64, device="cuda")
    off = torch.full((piece_cap + 1 + canary,), -9, dtype=torch.int64, device="cuda")
    dt = torch.full((2,), -9, dtype=torch.int64, device="cuda")
    ht = (C.c_int64 * 2)(-7, -7)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = batch.call(rx._lib, "mrx_extract", (rx._h,),
                    (prefix.data_ptr(), owner.data_ptr(), off.data_ptr(), piece_cap, out.data_ptr(), out_cap, dt.data_ptr(),
                     C.cast(ht, C.c_void_p) if totals else None, stream))
    torch.cuda.synchronize()
    return rc, _np(prefix), _np(owner), _np(off), _np(dt).tolist(), list(ht)


def test_capacities():
    import torch
    pat = b"[a-z]+\\d+"
    rx = M.compile_regex(pat)
    texts = TF._short_texts(5)
    want = X.expected_findall(pat, texts)
    pieces, nbytes = len(want[1]), len(want[3])
    assert pieces > 8 and nbytes > 64
    for batch in (M.DeviceBatch.from_texts(texts), LY.ragged_rows(texts, True, lambda i, t, k: (b"a1" * k)[:k]).device()):
        buf = torch.full((nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        # one piece short: no data byte, nothing past the capacity, the need in totals[0]
        for totals in (True, False):
            rc, prefix, owner, off, dt, ht = _raw_extract(rx, batch, pieces - 1, buf, nbytes, totals, canary=8)
            assert rc == (CAPACITY if totals else OK) and dt[0] == pieces and 0 <= dt[1] <= nbytes
            assert ht == (dt if totals else [-7, -7])
            assert prefix[-1] == pieces
            assert np.all(_np(buf) == 0xA5) and np.all(owner[pieces - 1:] == -9) and np.all(off[pieces:] == -9)
        # one byte short: owner, offsets and totals complete, no data byte
        for totals in (True, False):
            rc, prefix, owner, off, dt, ht = _raw_extract(rx, batch, pieces, buf, nbytes - 1, totals, canary=8)
            assert rc == (CAPACITY if totals else OK) and dt == [pieces, nbytes]
            assert np.array_equal(owner[:pieces], want[1]) and np.array_equal(off[:pieces + 1], want[2])
            assert np.all(_np(buf) == 0xA5) and np.all(owner[pieces:] == -9) and np.all(off[pieces + 1:] == -9)
        rc, prefix, owner, off, dt, ht = _raw_extract(rx, batch, pieces, buf, nbytes, canary=8)
        assert rc == OK and dt == [pieces, nbytes] and ht == dt
        got = _np(buf)
        assert np.array_equal(got[:nbytes], want[3]) and np.all(got[nbytes:] == 0xA5)
        # the primitive, on findall's own spans
        fprefix, spans, total = rx._dev_findall(batch)
        assert total == pieces
        buf.fill_(0xA5)
        rc, owner, off, dt, ht = _raw_gather(batch, fprefix, spans, 0, pieces - 1, buf, nbytes, canary=8)
        assert rc == CAPACITY and dt[0] == pieces and ht == dt and np.all(_np(buf) == 0xA5)
        assert np.all(owner[pieces - 1:] == -9) and np.all(off[pieces:] == -9)
        rc, owner, off, dt, ht = _raw_gather(batch, fprefix, spans, 0, pieces, buf, nbytes - 1, canary=8)
        assert rc == CAPACITY and dt == [pieces, nbytes] and np.all(_np(buf) == 0xA5)
        assert np.array_equal(owner[:pieces], want[1]) and np.array_equal(off[:pieces + 1], want[2])
        # the wrappers grow: the pieces first, then the bytes
        res = batch.gather_spans(fprefix, spans[:total], piece_cap=None, out_cap=None)
        _assert_result((res[0], fprefix, res[1]), want, "gather_spans")
        _scratch_is_returned()
    # more bytes out than in (overlapping occurrences) and more pieces than the default capacity (empty matches)
    over = [b"a" * 60, b"b", b"a" * 22]
    _assert_result(M.compile_regex(b"a" * 21).extract(M.DeviceBatch.from_texts(over)),
                   X.expected_findall(b"a" * 21, over), "outgrown bytes")
    many = [b"ab" * 300, b""]
    _assert_result(M.compile_regex(b"z*").extract(M.DeviceBatch.from_texts(many)), X.expected_findall(b"z*", many),
                   "outgrown pieces")
    assert M.findall_texts(b"a" * 21, over) == X.lists(X.expected_findall(b"a" * 21, over))
    _scratch_is_returned()


def test_host_buffer_entry_points():
    lib = M.load_library()
    pat = b"[a-z]+\\d+"
    rx = M.compile_regex(pat)
    texts = TF._short_texts(8, 200)
    want = X.expected_findall(pat, texts)
    pieces, nbytes = len(want[1]), len(want[3])
    data, off = M.pack_texts(texts)
    n = len(texts)

    def bufs():
        return (np.full(n + 1, -5, np.int64), np.full(pieces, -5, np.int64), np.full(pieces + 1, -5, np.int64),
                np.full(nbytes, 0xEE, np.uint8), (C.c_int64 * 2)(-7, -7))

    prefix, owner, out_off, out, tot = bufs()
    rc = lib.mrx_extract_batch(rx._h, data.ctypes.data, off.ctypes.data, n, prefix.ctypes.data, owner.ctypes.data,
                               out_off.ctypes.data, pieces, out.ctypes.data, nbytes, C.cast(tot, C.c_void_p))
    assert rc == OK and list(tot) == [pieces, nbytes]
    for got, w in zip((prefix, owner, out_off, out), want):
        assert np.array_equal(got, w)
    spans = np.ascontiguousarray(rx.match_all(texts)[1])
    for pcap, ocap, code in ((pieces, nbytes, OK), (pieces - 1, nbytes, CAPACITY), (pieces, nbytes - 1, CAPACITY)):
        _, owner, out_off, out, tot = bufs()
        rc = lib.mrx_gather_spans_batch(data.ctypes.data, off.ctypes.data, n, want[0].ctypes.data, spans.ctypes.data, 1, 0,
                                        pcap, owner.ctypes.data, out_off.ctypes.data, out.ctypes.data, ocap,
                                        C.cast(tot, C.c_void_p))
        assert rc == code and tot[0] == pieces
        if pcap == pieces:
            assert tot[1] == nbytes and np.array_equal(owner, want[1]) and np.array_equal(out_off, want[2])
        assert np.array_equal(out, want[3]) if code == OK else np.all(out == 0xEE)
    _scratch_is_returned()


def test_async_on_two_streams():
    import torch
    pats = (b"[a-z]+\\d+", b"\\d+")
    texts = [TF._short_texts(21, 1500), TF._short_texts(22, 1100)]
    rows40 = [(t + b" " * 40)[:40] for t in texts[1]]
    batches = [M.DeviceBatch.from_texts(texts[0]),
               M.DeviceBatch.strided(torch.from_numpy(np.frombuffer(b"".join(rows40), np.uint8).copy()).cuda(), 40, length=40)]
    texts[1] = rows40
    assert batches[0]._end_offset is not None
    outs = []
    for b in batches:
        cap = b.data.numel() // 2 + b.n
        outs.append((torch.empty(b.n + 1, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda"),
                     torch.empty(cap + 1, dtype=torch.int64, device="cuda"),
                     torch.full((b.data.numel(),), 0xA5, dtype=torch.uint8, device="cuda"),
                     torch.empty(2, dtype=torch.int64, device="cuda")))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for rep in range(3):
        for q in range(2):
            with torch.cuda.stream(streams[q]):
                M.compile_regex(pats[q]).extract_async(batches[q], outs[q])
    torch.cuda.synchronize()
    for q in range(2):
        wprefix, wowner, woff, wdata = X.expected_findall(pats[q], texts[q])
        prefix, owner, off, data, tot = (_np(t) for t in outs[q])
        assert tot.tolist() == [len(wowner), len(wdata)]
        assert np.array_equal(prefix, wprefix) and np.array_equal(owner[:len(wowner)], wowner)
        assert np.array_equal(off[:len(wowner) + 1], woff)
        assert np.array_equal(data[:len(wdata)], wdata) and np.all(data[len(wdata):] == 0xA5)
    _scratch_is_returned()


def test_pieces_feed_a_second_pattern():
    from mrx_ref import hybrid as O
    texts = LY.make_texts(b"[a-z]+\\d+", 300, n_long=4) + TF._short_texts(4, 200)
    rx, rx2 = M.compile_regex(b"[a-z]+\\d+"), M.compile_regex(b"\\d+")
    for batch in (M.DeviceBatch.from_texts(texts), LY.ragged_rows(texts, False, lambda i, t, k: (b"a1" * k)[:k]).device()):
        pieces, prefix, owner = rx.extract(batch)
        first = [p for row in X.lists(X.expected_findall(b"[a-z]+\\d+", texts)) for p in row]
        assert pieces.n == len(first) and pieces._end_offset == sum(len(p) for p in first) and pieces._max_len is not None
        fprefix, spans, total = rx2._dev_findall(pieces)
        fprefix, spans = _np(fprefix), _np(spans)
        for r, p in enumerate(first):
            assert [tuple(int(x) for x in sp) for sp in spans[fprefix[r]:fprefix[r + 1]]] == O.findall(b"\\d+", p), r
        second, prefix2, owner2 = rx2.extract(pieces)
        _assert_result((second, prefix2, owner2), X.expected_findall(b"\\d+", first), "second extract")
    _scratch_is_returned()
