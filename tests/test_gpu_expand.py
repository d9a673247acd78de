"""expand on the GPU against the oracle (tests/expand_expect.py): the match CSR over the texts, the owners, the records'
CSR and the records' bytes, bit for bit -- the qualifying corpus on every layout, the primitive on hand-made rows
(alignment sweep, segment boundaries against block boundaries, several rounds per wavefront), the edges of the contract
in include/mrx.h (capacities, canaries, asynchronous form, scratch), the host-buffer entry points, the product's own
sub() reassembled from expand's records, and a record batch feeding a second pattern."""
import ctypes as C

import numpy as np
import pytest

import mojo_regex_amd as M
import captures_all_expect as CA
import expand_expect as E
import layouts as LY
from test_gpu_extract import _assert_result, _dev, _np, _scratch_is_returned

pytestmark = pytest.mark.gpu

OK, CAPACITY = M.api.MRX_OK, M.api.MRX_E_CAPACITY

# (the split of the candidates into these two lists is asserted without a GPU: tests/test_expand_host.py)
CORPUS_PAIRS = [(p, t) for p, t in E.candidates() if p not in E.UNQUALIFIED]
HAND_PAIRS = [(p, t) for p, t in E.candidates() if p in E.HAND_TEXTS]


def _ids(pairs):
    return ["%s -> %s" % (p.decode(), t.decode()) for p, t in pairs]


def _check_bound(records, batch, tpl):
    longest = batch.longest()
    if longest is None:
        assert records._max_len is None
    else:
        assert records._max_len == len(tpl) + M.api._template_refs(tpl) * longest
        assert int(np.diff(_np(records.offsets)).max(initial=0)) <= records._max_len


@pytest.mark.parametrize("pat,tpl", CORPUS_PAIRS, ids=_ids(CORPUS_PAIRS))
def test_corpus_on_every_layout(pat, tpl):
    import torch
    rx = M.compile_regex(pat)
    texts = E.corpus_texts(pat)
    assert sum(len(r) for r in E.rows_of(pat, texts)) >= E.MIN_ROWS
    for lay in LY.layouts_for(texts, LY.pattern_poison(pat)):
        batch = lay.device()
        want = E.expected(pat, tpl, lay.texts)
        res = rx.expand(tpl, batch)
        torch.cuda.synchronize()
        _assert_result(res, want, (pat, tpl, lay.name))
        _scratch_is_returned()
        _check_bound(res[0], batch, tpl)
    assert rx.expand(tpl, texts[:20]) == E.lists(E.expected(pat, tpl, texts[:20]))


@pytest.mark.parametrize("pat,tpl", HAND_PAIRS, ids=_ids(HAND_PAIRS))
def test_hand_written_texts_of_the_shapes_without_seeded_rows(pat, tpl):
    rx = M.compile_regex(pat)
    texts = E.HAND_TEXTS[pat] + [b""]
    want = E.expected(pat, tpl, texts)
    assert len(want[1]) >= 2 and len(want[3]) > 0
    for lay in (LY.csr_packed(texts), LY.csr_shifted(texts, 7, LY.pattern_poison(pat)),
                LY.ragged_rows(texts, False, LY.pattern_poison(pat))):
        _assert_result(rx.expand(tpl, lay.device()), want, (pat, lay.name))
    assert M.expand(pat, tpl, texts) == E.lists(want)
    _scratch_is_returned()


def _raw_spans(batch, prefix, rows, tpl, piece_cap, out, out_cap, totals=True, canary=0):
    """mrx_expand_spans_* on the caller's buffers: (rc, owner, out_offsets, d_totals, host totals).  owner and
    out_offsets have `canary` more elements than the capacity says."""
    import torch
    lib = M.load_library()
    owner = torch.full((max(piece_cap, 1) + canary,), -9, dtype=torch.int64, device="cuda")
    off = torch.full((piece_cap + 1 + canary,), -9, dtype=torch.int64, device="cuda")
    dt = torch.full((2,), -9, dtype=torch.int64, device="cuda")
    ht = (C.c_int64 * 2)(-7, -7)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = batch.call(lib, "mrx_expand_spans", (),
                    (prefix.data_ptr(), rows.data_ptr(), int(rows.shape[1]), tpl, len(tpl), piece_cap, owner.data_ptr(),
                     off.data_ptr(), out.data_ptr(), out_cap, dt.data_ptr(), C.cast(ht, C.c_void_p) if totals else None,
                     stream))
    torch.cuda.synchronize()
    return rc, _np(owner), _np(off), _np(dt).tolist(), list(ht)


SWEEP_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 47)


def test_alignment_sweep_on_the_primitive():
    """Records of every sweep length as a literal head of 0..3 bytes, one group and a literal tail; the group's source at
    every alignment 0..15, the output at every alignment 0..15, a canary in front of and behind the output."""
    import torch
    text = bytes((37 * k + 11) % 251 for k in range(200))
    batch = M.DeviceBatch.from_texts([text])
    for head, tail in ((0, 0), (1, 0), (2, 1), (3, 2)):
        tpl = b"<[{"[:head] + b"\\1" + b"}>"[:tail]
        rows = [[(s, s + k - head - tail), (s, s + 50)] for s in range(16) for k in SWEEP_LENGTHS if k >= head + tail]
        want = E.from_rows(tpl, [rows], [text])
        assert sorted(set(np.diff(want[2]).tolist())) == [k for k in SWEEP_LENGTHS if k >= head + tail]
        nbytes = len(want[3])
        prefix, drows = _dev(want[0], np.int64), _dev(rows, np.int32)
        for skew in range(16):
            buf = torch.full((16 + skew + nbytes + 48,), 0xA5, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            rc, owner, off, dt, ht = _raw_spans(batch, prefix, drows, tpl, len(rows), buf[16 + skew:], nbytes)
            assert rc == OK and dt == [len(rows), nbytes] and ht == dt, (head, skew)
            got = _np(buf)
            assert np.all(got[:16 + skew] == 0xA5) and np.all(got[16 + skew + nbytes:] == 0xA5), (head, skew)
            assert np.array_equal(got[16 + skew:16 + skew + nbytes], want[3]), (head, skew)
            assert np.array_equal(owner[:len(rows)], want[1]) and np.array_equal(off, want[2]), (head, skew)
    _scratch_is_returned()


def _random_rows(rng, texts, per_text, g, longest, unset=0.2):
    """per_text(i) rows for text i, each g groups of 0..longest bytes (or without an entry) and a whole-match pair."""
    rows = []
    for i, t in enumerate(texts):
        rs = []
        for _ in range(per_text(i)):
            r = []
            for _ in range(g):
                if rng.random() < unset:
                    r.append((-1, -1))
                else:
                    s = int(rng.integers(0, len(t) + 1))
                    r.append((s, s + int(rng.integers(0, longest + 1))))   # (may reach behind the text: it is cut)
            rs.append(r + [(0, len(t))])
        rows.append(rs)
    return rows


def _spans_case(texts, rows, tpl, g, batches=None):
    want = E.from_rows(tpl, rows, texts)
    flat = np.array([r for rs in rows for r in rs], np.int32).reshape(-1, g + 1, 2)
    for batch in batches or (M.DeviceBatch.from_texts(texts),):
        prefix = _dev(want[0], np.int64)
        records, owner = batch.expand_spans(tpl, prefix, _dev(flat, np.int32))
        _assert_result((records, prefix, owner), want, tpl[:40])
        _check_bound(records, batch, tpl)
    _scratch_is_returned()
    return want


def test_segment_boundaries_against_block_boundaries():
    import torch
    rng = np.random.default_rng(13)
    texts = [bytes(rng.integers(1, 255, size=int(k)).tolist()) for k in rng.integers(0, 40, size=60)]
    rows = _random_rows(rng, texts, lambda i: 0 if i % 7 == 3 else 10, 9, 2)
    # 40 segments: one-byte literals and groups of 0 to 2 bytes in turn
    tpl40 = b"".join(bytes([0x41 + k]) + b"\\%d" % (k % 9 + 1) for k in range(20))
    assert len(CA.O._parse_repl_template(tpl40)) == 40
    lays = (LY.csr_packed(texts), LY.csr_shifted(texts, 7, lambda i, t, k: b"\xEE" * k),
            LY.ragged_rows(texts, False, lambda i, t, k: b"\xEE" * k))
    want = _spans_case(texts, rows, tpl40, 9, [lay.device() for lay in lays])
    assert len(want[3]) > 64 * 16
    # one literal of 300 bytes: records of several blocks each, fed from the literal buffer alone, and with a group
    lit = bytes(rng.integers(1, 255, size=300).tolist()).replace(b"\\", b"/")
    few = [rs[:2] for rs in rows]
    assert np.diff(_spans_case(texts, few, lit, 9)[2]).tolist() == [300] * sum(len(rs) for rs in few)
    _spans_case(texts, few, lit[:150] + b"\\4" + lit[150:], 9)
    # every referenced group without an entry: the records are the literals
    none = [[[(-1, -1)] * 9 + [(0, len(t))] for _ in rs] for rs, t in zip(rows, texts)]
    want = _spans_case(texts, none, b"<\\1|\\2\\9>", 9)
    assert set(E.lists(want)[0]) == {b"<|>"}
    # groups only over rows without an entry: every record is empty
    want = _spans_case(texts, none, b"\\1\\2", 9)
    assert len(want[1]) > 100 and len(want[3]) == 0
    # an empty template with 1000 rows: every offset repeats, no byte
    one = [b"0123456789"]
    rows1k = [[[(k % 10, k % 10 + 1), (0, 10)] for k in range(1000)]]
    want = _spans_case(one, rows1k, b"", 1)
    assert want[2].tolist() == [0] * 1001 and len(want[3]) == 0
    # n = 0 and a batch without rows
    none_rows = torch.zeros((0, 2, 2), dtype=torch.int32, device="cuda")
    records, owner = M.DeviceBatch.from_texts([]).expand_spans(b"x\\1", _dev([0], np.int64), none_rows)
    assert records.n == 0 and _np(records.offsets).tolist() == [0] and owner.numel() == 0
    records, owner = M.DeviceBatch.from_texts(one).expand_spans(b"x\\1", _dev([0, 0], np.int64), none_rows)
    assert records.n == 0 and _np(records.offsets).tolist() == [0] and records.data.numel() == 0
    rx = M.compile_regex(b"(\\d+)")
    records, prefix, owner = rx.expand(b"<\\1>", M.DeviceBatch.from_texts([]))
    assert records.n == 0 and _np(prefix).tolist() == [0] and _np(records.offsets).tolist() == [0]
    assert rx.expand(b"<\\1>", []) == [] and rx.expand(b"<\\1>", [b"", b"ab"]) == [[], []]
    _scratch_is_returned()


def test_several_rounds_per_wavefront():
    lib = M.load_library()
    rng = np.random.default_rng(9)
    texts = [bytes(rng.integers(97, 123, size=40).tolist()) for _ in range(1300)]
    rows = _random_rows(rng, texts, lambda i: 0 if i % 5 == 0 else 5, 3, 9, unset=0.3)   # texts without rows among them
    tpl = b"\\2,\\1;\\3\\2\n"
    want = E.from_rows(tpl, rows, texts)
    assert len(want[1]) > 5000 and len(want[3]) > 64 << 10
    batch = M.DeviceBatch.from_texts(texts)
    prefix = _dev(want[0], np.int64)
    drows = _dev(np.array([r for rs in rows for r in rs], np.int32), np.int32)
    lib.mrx_debug_expand_grid(1)   # 4 wavefronts: about 18 rounds of 64 blocks each
    try:
        records, owner = batch.expand_spans(tpl, prefix, drows)
        assert lib.mrx_last_kernel_name() == b"k_expand_gather"
        _assert_result((records, prefix, owner), want, "one workgroup")
    finally:
        lib.mrx_debug_expand_grid(0)
    records, owner = batch.expand_spans(tpl, prefix, drows)
    _assert_result((records, prefix, owner), want, "full grid")
    _scratch_is_returned()


def _raw_expand(rx, tpl, count, batch, match_cap, out, out_cap, totals=True, canary=0):
    import torch
    prefix = torch.full((batch.n + 1,), -9, dtype=torch.int64, device="cuda")
    owner = torch.full((max(match_cap, 1) + canary,), -9, dtype=torch.int64, device="cuda")
    off = torch.full((match_cap + 1 + canary,), -9, dtype=torch.int64, device="cuda")
    dt = torch.full((2,), -9, dtype=torch.int64, device="cuda")
    ht = (C.c_int64 * 2)(-7, -7)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = batch.call(rx._lib, "mrx_expand", (rx._h, tpl, len(tpl), count),
                    (prefix.data_ptr(), owner.data_ptr(), off.data_ptr(), match_cap, out.data_ptr(), out_cap, dt.data_ptr(),
                     C.cast(ht, C.c_void_p) if totals else None, stream))
    torch.cuda.synchronize()
    return rc, _np(prefix), _np(owner), _np(off), _np(dt).tolist(), list(ht)


def test_capacities():
    import torch
    pat, tpl = b"(\\w+) (\\w+)", b"\\2 \\1\n"
    rx = M.compile_regex(pat)
    texts = E.corpus_texts(pat)
    want = E.expected(pat, tpl, texts)
    pieces, nbytes = len(want[1]), len(want[3])
    assert pieces > 8 and nbytes > 64
    for batch in (M.DeviceBatch.from_texts(texts), LY.ragged_rows(texts, True, lambda i, t, k: (b"a b " * k)[:k]).device()):
        buf = torch.full((nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        # one match short: no data byte, nothing past the capacity, the need in totals[0].  The host knows this shortage
        # from captures_all, so it is reported without `totals` too
        for totals in (True, False):
            rc, prefix, owner, off, dt, ht = _raw_expand(rx, tpl, 0, batch, pieces - 1, buf, nbytes, totals, canary=8)
            assert rc == CAPACITY and dt == [pieces, 0]
            assert ht == (dt if totals else [-7, -7])
            assert prefix[-1] == pieces
            assert np.all(_np(buf) == 0xA5) and np.all(owner[pieces - 1:] == -9) and np.all(off[pieces:] == -9)
        # one byte short: owner, offsets and totals complete, no data byte
        for totals in (True, False):
            rc, prefix, owner, off, dt, ht = _raw_expand(rx, tpl, 0, batch, pieces, buf, nbytes - 1, totals, canary=8)
            assert rc == (CAPACITY if totals else OK) and dt == [pieces, nbytes]
            assert ht == (dt if totals else [-7, -7])
            assert np.array_equal(owner[:pieces], want[1]) and np.array_equal(off[:pieces + 1], want[2])
            assert np.all(_np(buf) == 0xA5) and np.all(owner[pieces:] == -9) and np.all(off[pieces + 1:] == -9)
        # exact fit, also in a larger capacity (the kernels run over the rows found)
        for cap in (pieces, pieces + 100):
            buf.fill_(0xA5)
            rc, prefix, owner, off, dt, ht = _raw_expand(rx, tpl, 0, batch, cap, buf, nbytes, canary=8)
            assert rc == OK and dt == [pieces, nbytes] and ht == dt
            got = _np(buf)
            assert np.array_equal(got[:nbytes], want[3]) and np.all(got[nbytes:] == 0xA5)
            assert np.array_equal(prefix, want[0]) and np.array_equal(owner[:pieces], want[1])
            assert np.array_equal(off[:pieces + 1], want[2]) and np.all(owner[pieces:] == -9) and np.all(off[pieces + 1:] == -9)
        # the primitive, on captures_all's own rows
        mprefix, rows = rx.captures_all(batch)
        assert rows.shape[0] == pieces
        buf.fill_(0xA5)
        for totals in (True, False):
            rc, owner, off, dt, ht = _raw_spans(batch, mprefix, rows, tpl, pieces - 1, buf, nbytes, totals, canary=8)
            assert rc == (CAPACITY if totals else OK) and dt[0] == pieces and 0 <= dt[1] <= nbytes
            assert ht == (dt if totals else [-7, -7]) and np.all(_np(buf) == 0xA5)
            assert np.all(owner[pieces - 1:] == -9) and np.all(off[pieces:] == -9)
            rc, owner, off, dt, ht = _raw_spans(batch, mprefix, rows, tpl, pieces, buf, nbytes - 1, totals, canary=8)
            assert rc == (CAPACITY if totals else OK) and dt == [pieces, nbytes] and np.all(_np(buf) == 0xA5)
            assert ht == (dt if totals else [-7, -7])
            assert np.array_equal(owner[:pieces], want[1]) and np.array_equal(off[:pieces + 1], want[2])
            assert np.all(owner[pieces:] == -9) and np.all(off[pieces + 1:] == -9)
        # totals == NULL on the primitive: nothing read back, d_totals right once the stream has drained
        rc, owner, off, dt, ht = _raw_spans(batch, mprefix, rows, tpl, pieces, buf, nbytes, totals=False, canary=8)
        assert rc == OK and ht == [-7, -7] and dt == [pieces, nbytes]
        got = _np(buf)
        assert np.array_equal(got[:nbytes], want[3]) and np.all(got[nbytes:] == 0xA5)
        assert np.all(owner[pieces:] == -9) and np.all(off[pieces + 1:] == -9)
        # the wrappers grow: the records first, then the bytes
        res = batch.expand_spans(tpl, mprefix, rows, piece_cap=None, out_cap=None)
        _assert_result((res[0], mprefix, res[1]), want, "expand_spans")
        _scratch_is_returned()
    # more bytes out than in, and more than the wrappers' first guess
    fat = b"=" * 500 + b"\\1\\1\\1\\2\\2"
    _assert_result(rx.expand(fat, M.DeviceBatch.from_texts(texts)), E.expected(pat, fat, texts), "outgrown bytes")
    rows_all = rx.captures_all(M.DeviceBatch.from_texts(texts))
    res = M.DeviceBatch.from_texts(texts).expand_spans(fat, *rows_all)
    _assert_result((res[0], rows_all[0], res[1]), E.expected(pat, fat, texts), "outgrown bytes, primitive")
    _scratch_is_returned()


def test_host_buffer_entry_points_and_count():
    lib = M.load_library()
    pat, tpl = b"(\\d+)-(\\d+)", b"\\2/\\1;"
    rx = M.compile_regex(pat)
    rng = np.random.default_rng(3)
    al = np.frombuffer(b"0123456789-- ab", np.uint8)
    texts = [bytes(rng.choice(al, size=int(k)).tolist()) for k in rng.integers(0, 80, size=150)] + [b"10-20 3-4 5-6"]
    data, off = M.pack_texts(texts)
    n = len(texts)
    for count in (0, 1, 2):
        want = E.expected(pat, tpl, texts, count)
        pieces, nbytes = len(want[1]), len(want[3])
        assert pieces > 20
        assert rx.expand(tpl, texts, count) == E.lists(want) and M.expand(pat, tpl, texts, count) == E.lists(want)

        def bufs():
            return (np.full(n + 1, -5, np.int64), np.full(pieces, -5, np.int64), np.full(pieces + 1, -5, np.int64),
                    np.full(nbytes, 0xEE, np.uint8), (C.c_int64 * 2)(-7, -7))

        for pcap, ocap, code in ((pieces, nbytes, OK), (pieces - 1, nbytes, CAPACITY), (pieces, nbytes - 1, CAPACITY)):
            prefix, owner, out_off, out, tot = bufs()
            rc = lib.mrx_expand_batch(rx._h, tpl, len(tpl), count, data.ctypes.data, off.ctypes.data, n, prefix.ctypes.data,
                                      owner.ctypes.data, out_off.ctypes.data, pcap, out.ctypes.data, ocap,
                                      C.cast(tot, C.c_void_p))
            assert rc == code and tot[0] == pieces and np.array_equal(prefix, want[0])
            if pcap == pieces:
                assert tot[1] == nbytes and np.array_equal(owner, want[1]) and np.array_equal(out_off, want[2])
            assert np.array_equal(out, want[3]) if code == OK else np.all(out == 0xEE)
        mprefix, rows = rx.captures_all(texts, count)
        rows = np.ascontiguousarray(rows)
        for pcap, ocap, code in ((pieces, nbytes, OK), (pieces - 1, nbytes, CAPACITY), (pieces, nbytes - 1, CAPACITY)):
            _, owner, out_off, out, tot = bufs()
            rc = lib.mrx_expand_spans_batch(data.ctypes.data, off.ctypes.data, n, mprefix.ctypes.data, rows.ctypes.data, 3, tpl,
                                            len(tpl), pcap, owner.ctypes.data, out_off.ctypes.data, out.ctypes.data, ocap,
                                            C.cast(tot, C.c_void_p))
            assert rc == code and tot[0] == pieces
            if pcap == pieces:
                assert tot[1] == nbytes and np.array_equal(owner, want[1]) and np.array_equal(out_off, want[2])
            assert np.array_equal(out, want[3]) if code == OK else np.all(out == 0xEE)
    _scratch_is_returned()


SUB_PAIRS = [(b"(\\d{3})(\\d{3})(\\d{4})", b"(\\1) \\2-\\3"), (b"(\\w+) (\\w+)", b"\\2 \\1"), (b"(a|ab)(c|bcd)(d*)", b"\\3\\2\\1"),
             (b"x(\\d)?", b"<\\1>"), (b"(\\w+)|(\\d+)", b"[\\1|\\2]")]


@pytest.mark.parametrize("pat,tpl", SUB_PAIRS, ids=_ids(SUB_PAIRS))
def test_sub_is_the_gaps_and_expands_records(pat, tpl):
    """The product's own sub() equals the host reassembly of the gaps between captures_all's whole-match spans and
    expand's device records."""
    rx = M.compile_regex(pat)
    texts = E.corpus_texts(pat) + [b"x", b"x5x", b"6502530000 4155551234"]
    batch = M.DeviceBatch.from_texts(texts)
    sub_off, sub_data = rx.sub_dev(tpl, batch)
    sub_off, raw = _np(sub_off), _np(sub_data).tobytes()
    records, prefix, owner = rx.expand(tpl, batch)
    mprefix, rows = rx.captures_all(batch)
    assert np.array_equal(_np(mprefix), _np(prefix))
    recs = E.lists((_np(prefix), _np(owner), _np(records.offsets), _np(records.data)))
    rows, prefix = _np(rows), _np(prefix)
    assert prefix[-1] >= E.MIN_ROWS
    for i, t in enumerate(texts):
        mine = [[tuple(int(x) for x in pr) for pr in r] for r in rows[prefix[i]:prefix[i + 1]]]
        assert raw[sub_off[i]:sub_off[i + 1]] == E.reassemble(t, mine, recs[i]), (pat, i, t[:60])
    _scratch_is_returned()


def test_records_feed_a_second_pattern():
    from mrx_ref import hybrid as O
    pat, tpl, pat2 = b"(\\w+)@(\\w+)\\.com", b"\\2", b"[a-z]+\\d"
    rng = np.random.default_rng(21)
    al = np.frombuffer(b"abcxyz019_", np.uint8)

    def word():
        return bytes(rng.choice(al, size=int(rng.integers(1, 12))).tolist())

    def addr():
        return word() + b"@" + word() + (b".com" if rng.random() < 0.8 else b".org")

    # (one address per text at most: on several the reference's loop does not always end)
    texts = [(word() + b" " + addr() + b" " + word()) if rng.random() < 0.8 else word() for _ in range(400)]
    rx, rx2 = M.compile_regex(pat), M.compile_regex(pat2)
    want = E.expected(pat, tpl, texts)
    first = [r for row in E.lists(want) for r in row]
    assert len(first) > 200
    for batch in (M.DeviceBatch.from_texts(texts), LY.ragged_rows(texts, False, lambda i, t, k: (b"a@b.com " * k)[:k]).device()):
        records, prefix, owner = rx.expand(tpl, batch)
        _assert_result((records, prefix, owner), want, "first")
        assert records._end_offset == len(want[3]) and records._max_len == 2 + batch.longest()
        s, e = rx2.search(records)
        s, e = _np(s), _np(e)
        for r, p in enumerate(first):
            w = O.search(pat2, p)
            assert (int(s[r]), int(e[r])) == (w if w else (-1, -1)), (r, p)
        assert (s >= 0).any() and (s < 0).any()
    _scratch_is_returned()
