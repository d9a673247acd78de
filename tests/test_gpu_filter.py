"""filter on the GPU against the oracle (tests/filter_expect.py: `compile_regex(p).test(text)` per text): the kept
indices, the output CSR and the output bytes, bit for bit, for every pattern of tests/layouts.py on every layout, plain
and inverted; pattern sets under any / all / inverted; the edges of the contract in include/mrx.h (canary, capacity,
sizes, asynchronous form, scratch, kernel name, host lists).

Every parity batch is asserted to hold a text that the oracle keeps and one that it drops, but for two cases where none
can exist: `x*`, `.*` and `a+b*` (the reference answers all three with a match at position 0 of every text, the empty
one included, so their plain predicate drops nothing and their inverted call is the none-kept case), and `^abc$` on the
layouts whose texts share one length other than 3 (it matches the text "abc" alone; it gets a fixed-length layout of
length 3 of its own, which does keep and drop)."""
import ctypes as C

import numpy as np
import pytest

import mojo_regex_amd as M
import filter_expect as E
import layouts as LY
import test_gpu_pattern_set as PS

pytestmark = pytest.mark.gpu

MATCH_EVERY_TEXT = (b"x*", b".*", b"a+b*")   # the oracle: a match at 0 whatever the text holds
CANNOT = [b"\x01\x02\x03", b"7", b"123456789012", b"\x7f" * 33, b"\n\n", b"\x01"]
SURE = [b"@.com a@b.com", b"ab" * 10, b"abc", b"foo 12", b"xyz123"]   # (the prefilter route finds no other address)
ROW = max(LY.WHOLE_ROW_STRIDES)     # rows at least this long are cut, never continued with poison
LONG_ROWS = [bytes([c]) * ROW for c in (1, 0x37, 0x7F, 0x0A)] + [b" " * (ROW - 3) + b"foo", b" " * (ROW - 1) + b"7"]


def _np(t):
    return t.cpu().numpy()


def _assert_result(res, want, where):
    kb, idx = res
    widx, woff, wdata = want
    assert kb.offsets is not None and kb.n == len(widx), where
    assert np.array_equal(_np(idx), widx), (where, _np(idx)[:8], widx[:8])
    assert np.array_equal(_np(kb.offsets), woff), where
    assert np.array_equal(_np(kb.data), wdata), where
    assert kb._end_offset in (None, len(wdata)), where   # (None: the input did not know its longest text)


@pytest.mark.parametrize("pat", LY.PATTERNS, ids=[p.decode() for p in LY.PATTERNS])
def test_one_pattern_on_every_layout(pat):
    import torch
    rx = M.compile_regex(pat)
    texts = LY.make_texts(pat, 90, n_long=3) + CANNOT + SURE + [b""]
    row_texts = texts + LONG_ROWS
    cache = {}
    lays = LY.layouts_for(texts, LY.pattern_poison(pat), row_texts)
    if pat == b"^abc$":   # rows of its one matching length too, so that a fixed-length batch keeps and drops texts
        lays.append(LY.fixed_length(row_texts, 16, 3, LY.pattern_poison(pat, 1)))
        lays[-1].check()
    for lay in lays:
        batch = lay.device()
        try:
            rx.match_next(batch)
        except M.UnsupportedPattern as e:
            with pytest.raises(M.UnsupportedPattern) as ei:
                rx.filter(batch)
            assert str(ei.value) == str(e)
            continue
        flags = E.keep_flags([pat], lay.texts, cache=cache)
        if pat in MATCH_EVERY_TEXT:
            assert all(flags)
        elif pat == b"^abc$" and not lay.csr and lay.lens is None and lay.length != 3:
            assert not any(flags)
        else:
            assert any(flags) and not all(flags), (pat, lay.name)
        for inv in (False, True):
            want = E.expected([pat], lay.texts, invert=inv, cache=cache)
            res = rx.filter(batch, invert=inv)
            torch.cuda.synchronize()
            _assert_result(res, want, (pat, lay.name, inv))
            if not lay.csr and lay.lens is None:
                assert res[0]._max_len == lay.length
            elif lay.known:
                assert res[0]._max_len == max(len(t) for t in lay.texts)
            if not lay.csr or lay.known:
                assert res[0]._end_offset == len(want[2])


def test_all_kept_and_none_kept():
    texts = [b"ab1", b"", b"z9" * 40, b"q7"]
    all_in = [t for t in texts if t]
    for lay in LY.layouts_for(all_in, LY.pattern_poison(b"\\d")):
        batch = lay.device()
        rx = M.compile_regex(b"[a-z7]")
        want = E.expected([b"[a-z7]"], lay.texts)
        assert len(want[0]) == batch.n
        _assert_result(rx.filter(batch), want, lay.name)
        kb, idx = rx.filter(batch, invert=True)
        assert kb.n == 0 and idx.numel() == 0 and _np(kb.offsets).tolist() == [0] and kb.data.numel() == 0
    kb, idx = M.compile_regex(b"x*").filter(M.DeviceBatch.from_texts(texts))
    assert _np(idx).tolist() == [0, 1, 2, 3] and _np(kb.offsets).tolist() == [0, 3, 3, 83, 85]


@pytest.fixture(scope="module")
def set_batches():
    import torch
    texts = PS._texts(11, 200)
    b = PS._batches(texts)
    out = {"csr": b["csr"], "known": (M.DeviceBatch.from_texts(texts), texts), "pitch_lens": b["pitch_lens"],
           "pitch_aligned": b["pitch_aligned"]}
    assert out["known"][0]._end_offset is not None
    return out


@pytest.mark.parametrize("setname", list(PS.SETS))
def test_sets_any_all_inverted(set_batches, setname):
    import torch
    pats = PS.SETS[setname]
    s = M.compile_set(pats)
    cache = {}
    for form, (batch, texts) in set_batches.items():
        hits = _np(s.matches(batch))
        for mode in ("any", "all"):
            row = hits.any(axis=1) if mode == "any" else hits.all(axis=1)
            for inv in (False, True):
                want = E.expected(pats, texts, mode, inv, cache)
                res = s.filter(batch, mode=mode, invert=inv)
                torch.cuda.synchronize()
                _assert_result(res, want, (setname, form, mode, inv))
                assert np.array_equal(_np(res[1]), np.nonzero(row != inv)[0]), (setname, form, mode, inv)


def _raw_call(rx, batch, out_data, cap, flags=0, totals=True):
    """The C call on the caller's own buffers: (rc, kept_idx, out_offsets, d_totals, host totals)."""
    import torch
    dev = batch.data.device
    idx = torch.full((batch.n,), -9, dtype=torch.int64, device=dev)
    off = torch.full((batch.n + 1,), -9, dtype=torch.int64, device=dev)
    dt = torch.full((2,), -9, dtype=torch.int64, device=dev)
    ht = (C.c_int64 * 2)(-7, -7)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = batch.call(rx._lib, "mrx_filter", (rx._h, flags), (idx.data_ptr(), off.data_ptr(), out_data.data_ptr(), cap,
                                                            dt.data_ptr(), C.cast(ht, C.c_void_p) if totals else None,
                                                            stream))
    torch.cuda.synchronize()
    return rc, _np(idx), _np(off), _np(dt).tolist(), list(ht)


def _short_texts(seed=3, n=700):
    rng = np.random.default_rng(seed)
    al = np.frombuffer(b"ab01 -", dtype=np.uint8)
    return [al[rng.integers(0, len(al), size=int(rng.integers(1, 41)))].tobytes() for _ in range(n)] + [b"", b"a1", b""]


@pytest.fixture(params=[1, 16], ids=["block_form", "text_form"])
def each_form(request):
    lib = M.load_library()
    lib.mrx_debug_filter_form(request.param)
    yield b"k_filter_gather" if request.param == 1 else b"k_filter_gather_text"
    lib.mrx_debug_filter_form(0)


@pytest.mark.parametrize("skew", [0, 1, 7, 15])
def test_canary_nothing_at_or_past_bytes_is_written(skew, each_form):
    import torch
    pat = b"[a-z]+\\d+"
    rx = M.compile_regex(pat)
    texts = _short_texts()
    batch = M.DeviceBatch.from_texts(texts)
    widx, woff, wdata = E.expected([pat], texts)
    nbytes = len(wdata)
    assert 0 < nbytes < batch.data.numel()
    buf = torch.full((skew + batch.data.numel() + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[skew:]
    rc, idx, off, dt, ht = _raw_call(rx, batch, out, int(batch.data.numel()))
    assert rc == M.api.MRX_OK and dt == [len(widx), nbytes] and ht == dt
    assert rx._lib.mrx_last_kernel_name() == each_form
    got = _np(buf)
    assert np.all(got[:skew] == 0xA5) and np.all(got[skew + nbytes:] == 0xA5)
    assert np.array_equal(got[skew:skew + nbytes], wdata)
    assert np.array_equal(idx[:len(widx)], widx) and np.array_equal(off[:len(widx) + 1], woff)


def test_capacity(each_form):
    import torch
    pat = b"[a-z]+\\d+"
    rx = M.compile_regex(pat)
    texts = _short_texts(5)
    batch = M.DeviceBatch.from_texts(texts)
    widx, woff, wdata = E.expected([pat], texts)
    nbytes = len(wdata)
    buf = torch.full((nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, idx, off, dt, ht = _raw_call(rx, batch, buf, nbytes - 1)
    assert rc == M.api.MRX_E_CAPACITY
    assert dt == [len(widx), nbytes] and ht == dt
    assert np.array_equal(idx[:len(widx)], widx) and np.array_equal(off[:len(widx) + 1], woff)
    assert np.all(_np(buf) == 0xA5)
    # the asynchronous form: the gather decides on the device
    rc, idx, off, dt, ht = _raw_call(rx, batch, buf, nbytes - 1, totals=False)
    assert rc == M.api.MRX_OK and dt == [len(widx), nbytes] and ht == [-7, -7] and np.all(_np(buf) == 0xA5)
    rc, idx, off, dt, ht = _raw_call(rx, batch, buf, nbytes)
    assert rc == M.api.MRX_OK and dt == [len(widx), nbytes]
    got = _np(buf)
    assert np.array_equal(got[:nbytes], wdata) and np.all(got[nbytes:] == 0xA5)


def test_sizes_empty_short_and_long_texts():
    import torch
    rx = M.compile_regex(b"\\d+")
    kb, idx = rx.filter(M.DeviceBatch.from_texts([]))
    assert kb.n == 0 and idx.numel() == 0 and _np(kb.offsets).tolist() == [0]
    assert rx.filter([])[0] == []
    d = torch.zeros(0, dtype=torch.uint8, device="cuda")
    rc, _, off, dt, ht = _raw_call(rx, M.DeviceBatch(d, torch.zeros(1, dtype=torch.int64, device="cuda")), d, 0)
    assert rc == M.api.MRX_OK and off.tolist() == [0] and dt == [0, 0] and ht == [0, 0]
    # texts of 1 to 40 bytes, several to one 16-byte block, and kept empty texts (inverted: empty texts have no digit)
    texts = _short_texts(9, 2000)
    for inv in (False, True):
        _assert_result(rx.filter(M.DeviceBatch.from_texts(texts), invert=inv), E.expected([b"\\d+"], texts, invert=inv),
                       ("short", inv))
    # a few texts beyond 1 MiB among short ones
    rng = np.random.default_rng(77)
    al = np.frombuffer(b"abc -", dtype=np.uint8)
    big = [al[rng.integers(0, len(al), size=(1 << 20) + k)].tobytes() for k in (5, 333, 70001)]
    big[1] = big[1][:500000] + b"42" + big[1][500002:]
    texts = _short_texts(10, 300) + [big[0]] + _short_texts(12, 50) + [big[1], big[2], b"9"]
    cache = {}
    want_plain = E.expected([b"\\d+"], texts, cache=cache)
    assert len(texts) - 2 not in want_plain[0] and len(texts) - 3 in want_plain[0]
    for lay in (LY.csr_packed(texts), LY.csr_shifted(texts, 7, lambda i, t, k: b"5" * k)):
        batch = lay.device()
        for inv in (False, True):
            _assert_result(rx.filter(batch, invert=inv), E.expected([b"\\d+"], texts, invert=inv, cache=cache),
                           (lay.name, inv))


def test_async_on_two_streams():
    import torch
    pats = (b"[a-z]+\\d+", b"\\d+")
    texts = [_short_texts(21, 1500), _short_texts(22, 1100)]
    batches = [M.DeviceBatch.from_texts(t) for t in texts]
    outs = []
    for b in batches:
        outs.append((torch.empty(b.n, dtype=torch.int64, device="cuda"), torch.empty(b.n + 1, dtype=torch.int64, device="cuda"),
                     torch.full((b.data.numel(),), 0xA5, dtype=torch.uint8, device="cuda"),
                     torch.empty(2, dtype=torch.int64, device="cuda")))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for rep in range(3):
        for q in range(2):
            with torch.cuda.stream(streams[q]):
                M.compile_regex(pats[q]).filter_async(batches[q], outs[q], invert=bool(q))
    torch.cuda.synchronize()
    for q in range(2):
        widx, woff, wdata = E.expected([pats[q]], texts[q], invert=bool(q))
        idx, off, data, tot = (_np(t) for t in outs[q])
        assert tot.tolist() == [len(widx), len(wdata)]
        assert np.array_equal(idx[:len(widx)], widx) and np.array_equal(off[:len(widx) + 1], woff)
        assert np.array_equal(data[:len(wdata)], wdata) and np.all(data[len(wdata):] == 0xA5)


def test_result_feeds_findall_and_a_second_filter():
    from mrx_ref import hybrid as O
    texts = LY.make_texts(b"[a-z]+\\d+", 300, n_long=4) + _short_texts(4, 200)
    rx, rx2 = M.compile_regex(b"[a-z]+\\d+"), M.compile_regex(b"hello|ab")
    for batch in (M.DeviceBatch.from_texts(texts), LY.ragged_rows(texts, False, lambda i, t, k: (b"a1" * k)[:k]).device()):
        kb, idx = rx.filter(batch)
        kept = [texts[int(i)] for i in _np(idx)]
        assert kept == E.expected_lists([b"[a-z]+\\d+"], texts)[0]
        assert kb._end_offset == sum(len(t) for t in kept) and kb._max_len is not None
        prefix, spans, total = rx._dev_findall(kb)
        prefix, spans = _np(prefix), _np(spans)
        for r, t in enumerate(kept):
            assert [tuple(int(x) for x in sp) for sp in spans[prefix[r]:prefix[r + 1]]] == O.findall(b"[a-z]+\\d+", t), r
        kb2, idx2 = rx2.filter(kb, invert=True)
        _assert_result((kb2, idx2), E.expected([b"hello|ab"], kept, invert=True), "second filter")


def test_scratch_does_not_grow_and_the_gather_is_named():
    lib = M.load_library()
    rx = M.compile_regex(b"[a-z]+\\d+")
    s = M.compile_set(PS.MIXED)
    batch = M.DeviceBatch.from_texts(_short_texts(31, 5000))
    sizes = []
    unknown = M.DeviceBatch(batch.data, batch.offsets)   # a CSR batch whose longest text the host does not know
    for call in range(10):
        rx.filter(batch)
        assert lib.mrx_last_kernel_name() == b"k_filter_gather_text"
        s.filter(batch, mode="all", invert=True)
        assert lib.mrx_last_kernel_name() == b"k_filter_gather_text"
        rx.filter(unknown)
        assert lib.mrx_last_kernel_name() == b"k_filter_gather"
        sizes.append(lib.mrx_debug_scratch_bytes())
    assert sizes[1] == sizes[9], sizes


def test_both_forms_give_the_same_bytes_on_short_and_long_texts(each_form):
    lib = M.load_library()
    rx = M.compile_regex(b"\\d+")
    texts = _short_texts(41, 900) + [b"ab7" * 3000, b"x" * 5000, b"1" * 4097]
    want = E.expected([b"\\d+"], texts)
    for lay in (LY.csr_packed(texts), LY.csr_shifted(texts, 1, lambda i, t, k: b"5" * k)):
        _assert_result(rx.filter(lay.device()), want, (each_form, lay.name))
        assert lib.mrx_last_kernel_name() == each_form


def test_block_form_carries_its_texts_over_three_rounds_of_a_wavefront():
    """At its full grid (2048 workgroups of 4 wavefronts) k_filter_gather gives a wavefront one round of 64 blocks up to
    2048 x 4 x 64 x 16 B = 8 MiB of kept bytes.  Between 16 and 24 MiB make it three, so that the texts a round ended
    with (cur, hi) are where the next one begins.  The predicate is one literal byte that the generator plants, inverted
    so that empty texts are kept too: the expected output is a numpy selection, no oracle call per text."""
    import torch
    lib = M.load_library()
    rng = np.random.default_rng(20261020)
    n = 170_000
    lens = rng.integers(0, 301, size=n)
    lens[rng.random(n) < 0.05] = 0
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    al = np.frombuffer(b"abcxyz0189 -", dtype=np.uint8)
    data = al[rng.integers(0, len(al), size=int(off[-1]))]
    drop = (rng.random(n) < 0.25) & (lens > 0)
    data[off[:-1][drop] + (rng.random(int(drop.sum())) * lens[drop]).astype(np.int64)] = ord("Q")
    keep = ~drop
    widx = np.nonzero(keep)[0]
    woff = np.concatenate([[0], np.cumsum(lens[keep])])
    wdata = data[np.repeat(keep, lens)]
    nbytes = len(wdata)
    assert (16 << 20) < nbytes <= (24 << 20) and np.any(lens[keep] == 0) and np.any(lens[keep] == 300)
    batch = M.DeviceBatch(torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda())
    skew, cap = 7, len(data)
    buf = torch.full((skew + cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    lib.mrx_debug_filter_form(1)
    try:
        rc, idx, got_off, dt, ht = _raw_call(M.compile_regex(b"Q"), batch, buf[skew:], cap, flags=M.api.MRX_FILTER_INVERT)
        assert lib.mrx_last_kernel_name() == b"k_filter_gather"
    finally:
        lib.mrx_debug_filter_form(0)
    assert rc == M.api.MRX_OK and dt == [len(widx), nbytes] and ht == dt
    got = _np(buf)
    assert np.all(got[:skew] == 0xA5) and np.all(got[skew + nbytes:] == 0xA5)
    assert np.array_equal(got[skew:skew + nbytes], wdata)
    assert np.array_equal(idx[:len(widx)], widx) and np.array_equal(got_off[:len(widx) + 1], woff)


def test_host_list_wrappers():
    texts = LY.make_texts(b"\\d+", 150, n_long=2) + CANNOT + [b""]
    kept, idx = M.compile_regex(b"\\d+").filter(texts)
    wk, wi = E.expected_lists([b"\\d+"], texts)
    assert kept == wk and isinstance(idx, np.ndarray) and idx.dtype == np.int64 and np.array_equal(idx, wi)
    kept, idx = M.filter_texts(b"\\d+", texts, invert=True)
    wk, wi = E.expected_lists([b"\\d+"], texts, invert=True)
    assert kept == wk and np.array_equal(idx, wi)
    s = M.compile_set(PS.MIXED)
    small = PS._texts(13, 150)
    for mode, inv in (("any", False), ("all", False), ("any", True), ("all", True)):
        kept, idx = s.filter(small, mode=mode, invert=inv)
        wk, wi = E.expected_lists(PS.MIXED, small, mode, inv)
        assert kept == wk and np.array_equal(idx, wi), (mode, inv)
