"""Lines on the GPU (include/mrx.h, "lines"): prefix, owner, offsets, data and all four totals bit for bit against
tests/lines_expect.py, on every batch of tests/lines_cases.py (built from the piece length of the testing hook) in every
layout, under short capacities, in the asynchronous and the zero-copy form, in chunks, past 2^31 bytes, against the
regex split it replaces for one byte, and in front of filter, extract and distinct."""
import ctypes as C

import numpy as np
import pytest

import mojo_regex_amd as M
import layouts as LY
import lines_cases as LC
import lines_expect as LE

pytestmark = pytest.mark.gpu

OK, CAPACITY = M.api.MRX_OK, M.api.MRX_E_CAPACITY


def _np(t):
    return t.cpu().numpy()


def _scratch_is_returned():
    assert M.load_library().mrx_debug_scratch_in_use() == 0


def _assert_lines(batch, texts, where, **opts):
    res, prefix, owner = batch.lines(**opts)
    wprefix, wowner, woff, wdata, wtot = LE.expected(texts, **{k: v for k, v in opts.items() if not k.endswith("_cap")})
    assert [res.n, res._end_offset, res._max_len, res.tail] == wtot, (where, wtot)
    assert res.offsets is not None
    assert np.array_equal(_np(prefix), wprefix), where
    assert np.array_equal(_np(owner), wowner), where
    assert np.array_equal(_np(res.offsets), woff), where
    assert np.array_equal(_np(res.data)[:wtot[1]], wdata), where
    _scratch_is_returned()
    return res


def _sep_poison(seed):
    """Bytes outside the texts that are mostly line ends: a kernel that read them as text would make lines of them."""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(b"\n\r\n\n\rq", np.uint8)
    return lambda i, t, k: al[rng.integers(0, len(al), size=k)].tobytes() if k > 0 else b""


def test_every_layout_with_every_option_set():
    P = LC.piece_length()
    texts = LC.log_texts(60, 11, n_long=2, P=P)
    lays = LY.layouts_for(texts, _sep_poison(1))
    with_outside = changed = 0
    for lay in lays:
        for i, t in enumerate(lay.texts):
            outside = lay.outside(i)
            if outside:
                with_outside += 1
                changed += LE.lines(t + outside) != LE.lines(t)
    assert with_outside > 300 and 2 * changed >= with_outside, (with_outside, changed)   # the outside would show
    for lay in lays:
        batch = lay.device()
        for opts in LE.OPTION_SETS:
            _assert_lines(batch, lay.texts, (lay.name, opts), **opts)


def _cases(group):
    return sorted(group(LC.piece_length()).items())


@pytest.mark.parametrize("name", [k for k, _ in _cases(LC.piece_edges)])
def test_piece_edges(name):
    texts = dict(_cases(LC.piece_edges))[name]
    batch = M.DeviceBatch.from_texts(texts)
    for opts in LE.OPTION_SETS:
        _assert_lines(batch, texts, (name, opts), **opts)
    import torch
    if len(texts) == 1:   # the same text as one raw buffer: the strided form of one text
        data = torch.from_numpy(np.frombuffer(texts[0], np.uint8).copy()).cuda()
        for opts in LE.OPTION_SETS:
            res = M.DeviceBatch.from_lines(data, **opts)
            want = LE.expected(texts, **opts)
            assert [res.n, res._end_offset, res._max_len, res.tail] == want[4], (name, opts)
            assert np.array_equal(_np(res.offsets), want[2]) and np.array_equal(_np(res.data)[:want[4][1]], want[3])


def test_output_alignment_with_shifted_inputs():
    for name, texts in _cases(LC.output_alignment):
        pz = _sep_poison(len(name))
        for lay in [LY.csr_packed(texts)] + [LY.csr_shifted(texts, s, pz) for s in LY.CSR_SHIFTS]:
            batch = lay.device()
            for opts in LE.OPTION_SETS:
                _assert_lines(batch, texts, (name, lay.name, opts), **opts)


def test_empty_texts_and_many_short_ones():
    for group in (LC.empty_texts, LC.many_short_texts):
        for name, texts in _cases(group):
            batch = M.DeviceBatch.from_texts(texts)
            for opts in LE.OPTION_SETS:
                _assert_lines(batch, texts, (name, opts), **opts)


def test_another_separator_and_host_lists():
    texts = [b"a;b;;c", b";", b"", b"x\ny;", b"no separator"]
    batch = M.DeviceBatch.from_texts(texts)
    for opts in (dict(sep=b";"), dict(sep=b";", keepends=True), dict(sep=b";", partial=False)):
        _assert_lines(batch, texts, opts, **opts)
    assert M.lines_of(texts, sep=b";") == [LE.lines(t, sep=b";")[0] for t in texts]
    assert M.lines_of(b"a\r\nb\n\nc", crlf=True) == [b"a", b"b", b"", b"c"]
    assert M.lines_of([]) == [] and M.lines_of(b"") == []
    with pytest.raises(M.MrxError):
        batch.lines(sep=b";", crlf=True)
    with pytest.raises(M.MrxError):
        batch.lines(keepends=True, crlf=True)
    _scratch_is_returned()


def _raw(batch, pcap, ocap, flags=0, host_totals=True):
    """One C call on buffers with canaries behind every output: (rc, prefix, owner, offsets, data, device totals, host
    totals)."""
    import torch
    dev, n = batch.data.device, batch.n
    prefix = torch.full((n + 1 + 8,), -7, dtype=torch.int64, device=dev)
    owner = torch.full((pcap + 8,), -7, dtype=torch.int64, device=dev)
    off = torch.full((pcap + 1 + 8,), -7, dtype=torch.int64, device=dev)
    out = torch.full((ocap + 32,), 0xEE, dtype=torch.uint8, device=dev)
    d_tot = torch.full((4 + 4,), -7, dtype=torch.int64, device=dev)
    tot = (C.c_int64 * 4)(-1, -1, -1, -1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = batch.call(M.load_library(), "mrx_lines", (flags, 10),
                    (prefix.data_ptr(), owner.data_ptr(), off.data_ptr(), pcap, out.data_ptr(), ocap, d_tot.data_ptr(),
                     C.cast(tot, C.c_void_p) if host_totals else None, stream))
    torch.cuda.synchronize()
    prefix, owner, off, out, d_tot = (_np(t) for t in (prefix, owner, off, out, d_tot))
    assert np.all(prefix[n + 1:] == -7) and np.all(owner[pcap:] == -7) and np.all(off[pcap + 1:] == -7)
    assert np.all(out[ocap:] == 0xEE) and np.all(d_tot[4:] == -7)   # the canaries
    return rc, prefix[:n + 1], owner[:pcap], off[:pcap + 1], out[:ocap], d_tot[:4].tolist(), list(tot)


def test_capacity():
    texts = LC.log_texts(50, 13, n_long=2, P=LC.piece_length())
    wprefix, wowner, woff, wdata, wtot = LE.expected(texts)
    lines, nbytes = wtot[0], wtot[1]
    for batch in (LY.csr_packed(texts).device(), LY.ragged_rows(texts, False, _sep_poison(2)).device()):
        rc, prefix, owner, off, out, d_tot, tot = _raw(batch, lines - 1, nbytes)
        assert rc == CAPACITY and tot == d_tot and tot[0] == lines and tot[1] == nbytes and tot[3] == wtot[3]
        assert np.array_equal(prefix, wprefix) and np.all(out == 0xEE)
        rc, prefix, owner, off, out, d_tot, tot = _raw(batch, lines, nbytes - 1)
        assert rc == CAPACITY and tot == d_tot == wtot
        assert np.array_equal(prefix, wprefix) and np.array_equal(owner, wowner) and np.array_equal(off, woff)
        assert np.all(out == 0xEE)   # no output byte at all
        rc, prefix, owner, off, out, d_tot, tot = _raw(batch, lines, nbytes)   # the retry
        assert rc == OK and tot == d_tot == wtot
        assert np.array_equal(prefix, wprefix) and np.array_equal(owner, wowner) and np.array_equal(off, woff)
        assert np.array_equal(out, wdata)
        rc, prefix, owner, off, out, d_tot, tot = _raw(batch, 0, 0)   # no capacity at all
        assert rc == CAPACITY and tot[0] == lines and np.array_equal(prefix, wprefix)
        with pytest.raises(M.MrxError):
            batch.lines(piece_cap=lines - 1)
        with pytest.raises(M.MrxError):
            batch.lines(out_cap=nbytes - 1)
        _assert_lines(batch, texts, "own capacities that fit", piece_cap=lines, out_cap=nbytes)
    # the default capacity holds a line per 32 bytes: a text of separators alone makes the call grow it
    many = [b"\n" * 5000, b"a"]
    _assert_lines(M.DeviceBatch.from_texts(many), many, "grown")
    _scratch_is_returned()


def test_async_equals_sync_and_reads_nothing_back():
    import torch
    lib = M.load_library()
    texts = LC.log_texts(64, 17, longest=120)
    rows = [(t + b"\n" * 128)[:128] for t in texts]
    raw = torch.from_numpy(np.frombuffer(b"".join(rows), np.uint8).copy()).cuda()
    known = M.DeviceBatch.from_texts(texts)
    assert known._end_offset is not None
    # a fixed pitch and a CSR batch with known bounds never look at the device; a CSR batch without them reads its first
    # and last offset, once
    batches = [(M.DeviceBatch.strided(raw, 128, length=128), rows, 0), (known, texts, 0),
               (M.DeviceBatch(known.data, known.offsets), texts, 1)]
    for batch, its_texts, reads in batches:
        for opts in LE.OPTION_SETS:
            wprefix, wowner, woff, wdata, wtot = LE.expected(its_texts, **opts)
            out = (torch.empty(batch.n + 1, dtype=torch.int64, device="cuda"), torch.empty(wtot[0] + 3, dtype=torch.int64, device="cuda"),
                   torch.empty(wtot[0] + 4, dtype=torch.int64, device="cuda"),
                   torch.full((wtot[1] + 5,), 0xA5, dtype=torch.uint8, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda"))
            before = lib.mrx_debug_lines_syncs()
            batch.lines_async(out, **opts)
            assert lib.mrx_debug_lines_syncs() - before == reads
            _scratch_is_returned()
            torch.cuda.synchronize()
            prefix, owner, off, data, tot = (_np(t) for t in out)
            assert tot.tolist() == wtot, opts
            assert np.array_equal(prefix, wprefix) and np.array_equal(owner[:wtot[0]], wowner)
            assert np.array_equal(off[:wtot[0] + 1], woff)
            assert np.array_equal(data[:wtot[1]], wdata) and np.all(data[wtot[1]:] == 0xA5)
            sync = batch.lines(**opts)
            assert np.array_equal(_np(sync[0].offsets), off[:wtot[0] + 1]) and np.array_equal(_np(sync[0].data)[:wtot[1]], data[:wtot[1]])


def test_keepends_of_a_buffer_moves_no_byte():
    import torch
    text = b"".join(LC.log_texts(30, 19)) + b"\ntail"
    data = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    for partial in (True, False):
        res = M.DeviceBatch.from_lines(data, keepends=True, partial=partial)
        want = LE.expected([text], keepends=True, partial=partial)
        assert res.data.data_ptr() == data.data_ptr() and res.data.numel() == data.numel()   # the caller's tensor
        assert [res.n, res._end_offset, res._max_len, res.tail] == want[4] and res.tail == 4
        assert np.array_equal(_np(res.offsets), want[2])
        raw = _np(res.data).tobytes()
        off = _np(res.offsets)
        assert [raw[off[j]:off[j + 1]] for j in range(res.n)] == LE.lines(text, keepends=True, partial=partial)[0]
    _scratch_is_returned()


def _lists(batch):
    raw, off = _np(batch.data).tobytes(), _np(batch.offsets)
    return [raw[off[j]:off[j + 1]] for j in range(batch.n)]


def test_reading_in_chunks_carries_the_tail():
    import torch
    rng = np.random.default_rng(23)
    al = np.frombuffer(b"abcdefgh 0123456789\n\r\n", np.uint8)
    whole = al[rng.integers(0, len(al), size=10000)].tobytes()[:-1] + b"x"   # an unterminated last line
    cuts = [0, 1234, 5003, 7777, len(whole)]
    got, carry = [], b""
    for a, b in zip(cuts, cuts[1:]):
        buf = carry + whole[a:b]
        res = M.DeviceBatch.from_lines(torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda(), crlf=True, partial=False)
        got += _lists(res)
        carry = buf[len(buf) - res.tail:]
    got.append(carry)   # the end of the file: what is left is its last line
    one = M.DeviceBatch.from_lines(torch.from_numpy(np.frombuffer(whole, np.uint8).copy()).cuda(), crlf=True)
    assert got == _lists(one) == LE.lines(whole, crlf=True)[0]
    _scratch_is_returned()


def test_a_text_of_more_than_2_to_the_31_bytes():
    import torch
    size = (1 << 31) + 4096 + 5
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory: a 2 GiB text and its 2 GiB of lines")
    data = torch.zeros(size, dtype=torch.uint8, device="cuda")
    seps = [5, (1 << 31) - 4097, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 31) + 4096]
    idx = torch.tensor(seps, dtype=torch.int64, device="cuda")
    data[idx + 1] = 7   # the first byte of every line behind a separator, unless it is a separator too
    data[idx] = 10
    marked = [s + 1 for s in seps if s + 1 not in seps]
    batch = M.DeviceBatch(data, torch.tensor([0, size], dtype=torch.int64, device="cuda"))
    res, prefix, owner = batch.lines(piece_cap=16)
    ends, woff = [0] + [s + 1 for s in seps] + [size], [0]
    for a, b in zip(ends, ends[1:]):
        if b - 1 in seps:
            woff.append(woff[-1] + (b - a - 1))
        elif b > a:
            woff.append(woff[-1] + (b - a))
    lines, nbytes = len(woff) - 1, size - len(seps)
    assert lines == 7 and woff[-1] == nbytes
    assert [res.n, res._end_offset, res._max_len, res.tail] == [lines, nbytes, max(np.diff(woff)), size - seps[-1] - 1]
    assert _np(res.offsets).tolist() == woff and _np(prefix).tolist() == [0, lines] and _np(owner).tolist() == [0] * lines
    out = res.data[:nbytes]
    assert int(torch.count_nonzero(out)) == len(marked) == 4              # the separators are gone, the marks are not
    starts = [woff[j] for j in range(lines) if ends[j] in marked]         # ... and each begins its line
    assert len(starts) == 4 and _np(out[torch.tensor(starts, device="cuda")]).tolist() == [7] * 4
    del res, out, data, batch
    _scratch_is_returned()


def test_agrees_with_the_regex_split_it_replaces():
    texts = LC.log_texts(80, 29, n_long=2, P=LC.piece_length())
    batch = M.DeviceBatch.from_texts(texts)
    # (the pattern is the newline byte itself: this dialect has no \n escape)
    pieces, pprefix, _ = M.compile_regex(b"\n").split_batch(batch)
    old = M.api._piece_lists(pieces, pprefix)
    old = [p[:-1] if p and p[-1] == b"" else p for p in old]
    res, prefix, _ = batch.lines()
    assert M.api._piece_lists(res, prefix) == old == [LE.lines(t)[0] for t in texts]


def test_lines_feed_filter_extract_and_distinct(monkeypatch):
    import torch
    rng = np.random.default_rng(31)
    log = [b"%s /item%d/%s %d" % (rng.choice([b"GET", b"POST", b"HEAD"]), rng.integers(0, 9), rng.choice([b"a", b"bb", b"ccc"]),
                                  rng.integers(200, 504)) for _ in range(200)]
    data = torch.from_numpy(np.frombuffer(b"\n".join(log) + b"\n", np.uint8).copy()).cuda()
    keep, path = M.compile_regex(b"GET|HEAD"), M.compile_regex(b"/item\\d")
    lib = M.load_library()
    path.extract(M.DeviceBatch.from_texts([b"/item1"]))   # (resolves the entry points of the stems below)
    keep.filter(M.DeviceBatch.from_texts([b"GET"]))
    known_calls = []
    for stem in ("mrx_filter", "mrx_extract"):
        fn_csr, fn_known, fn_strided = M.DeviceBatch._entry_points[stem]

        def spy(*args, _fn=fn_known, _stem=stem):
            known_calls.append(_stem)
            return _fn(*args)

        def never(*args, _stem=stem):
            raise AssertionError("%s took the entry point that reads the bounds back" % _stem)

        monkeypatch.setitem(M.DeviceBatch._entry_points, stem, (never, spy, fn_strided))

    def chain(batch):
        kept, idx = keep.filter(batch)
        pieces, _, _ = path.extract(kept)
        values, counts, _, _ = pieces.distinct()
        return _lists(values), _np(counts).tolist(), _np(idx).tolist()

    lines = M.DeviceBatch.from_lines(data)
    assert lines.n == 200 and lines._end_offset == sum(len(l) for l in log) and lines._max_len == max(len(l) for l in log)
    got = chain(lines)
    assert known_calls == ["mrx_filter", "mrx_extract"]   # findall on the lines: the entry with known bounds
    assert got == chain(M.DeviceBatch.from_texts(log))
    assert sum(got[1]) == len(got[2]) == sum(l.startswith((b"GET", b"HEAD")) for l in log)
    assert lib.mrx_last_error() is not None
    _scratch_is_returned()
