"""Translate and strip on the GPU (include/mrx.h, "translate", "strip"): offsets, bytes, totals and rows bit for bit
against tests/translate_expect.py, on every batch of tests/translate_cases.py (built from the piece length of the testing
hook), in every layout with bytes around the texts that would show, in the same-length form's own
contract (the input's layout, canaries, no read-back), in the asynchronous forms, and in front of distinct, gather_spans
and parse_spans."""
import ctypes as C

import numpy as np
import pytest

import mojo_regex_amd as M
import layouts as LY
import translate_cases as TC
import translate_expect as TE

pytestmark = pytest.mark.gpu

OK, CAPACITY = M.api.MRX_OK, M.api.MRX_E_CAPACITY


def _np(t):
    return t.cpu().numpy()


def _scratch_is_returned():
    assert M.load_library().mrx_debug_scratch_in_use() == 0


def _texts_of(batch):
    """the texts of a batch in either layout, from the device"""
    raw = _np(batch.data).tobytes()
    if batch.offsets is not None:
        off = _np(batch.offsets)
        return [raw[off[i]:off[i + 1]] for i in range(batch.n)]
    lens = _np(batch.lens) if batch.lens is not None else [batch.length] * batch.n
    return [raw[i * batch.stride:i * batch.stride + int(lens[i])] for i in range(batch.n)]


_WANT = {}


def _want(key, texts, params):
    key = (key, len(texts), tuple(sorted(params.items())))
    if key not in _WANT:
        _WANT[key] = TE.expected(texts, **params)
    return _WANT[key]


def _assert_translate(batch, texts, params, where, want=None):
    res = batch.translate(**params)
    woff, wdata, wtot = TE.expected(texts, **params) if want is None else want
    _scratch_is_returned()
    assert res.n == len(texts), where
    if params.get("delete") or params.get("squeeze"):
        assert res.offsets is not None and [res._end_offset, res._max_len] == wtot, (where, wtot)
        assert np.array_equal(_np(res.offsets), woff), where
        assert np.array_equal(_np(res.data)[:wtot[0]], wdata), where
    else:   # the input's layout
        if batch.offsets is not None:
            assert res.offsets is batch.offsets and (res._end_offset, res._max_len) == (batch._end_offset, batch._max_len), where
        else:
            assert (res.offsets, res.stride, res.length, res.lens) == (None, batch.stride, batch.length, batch.lens), where
        assert res.data.numel() == batch.data.numel() and res.data is not batch.data, where
        assert b"".join(_texts_of(res)) == wdata.tobytes(), where
    return res


def _poison(seed):
    """Bytes outside the texts that every parameter set would act on: members of the delete and squeeze sets and
    letters that the tables change."""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(b" \r\tabAB-\"e  \r", np.uint8)
    return lambda i, t, k: al[rng.integers(0, len(al), size=k)].tobytes() if k > 0 else b""


def _strip_poison(i, t, k):
    """An alternation of set bytes and others behind a text: an end that ran on would lie elsewhere."""
    return (b" x \t\"ab1Z" * (k // 9 + 1))[:k]


def test_every_layout_with_every_parameter_set():
    P = TC.piece_length()
    texts = TC.mixed_texts(60, 11, n_long=2, P=P)
    lays = LY.layouts_for(texts, _poison(1))
    with_outside = changed = 0
    for lay in lays:
        for i, t in enumerate(lay.texts):
            outside = lay.outside(i)
            if outside:
                with_outside += 1
                changed += all(TE.translate(t + outside, **p) != TE.translate(t, **p) for p in TE.PARAMETER_SETS)
    assert with_outside > 300 and 2 * changed >= with_outside, (with_outside, changed)   # the outside would show
    for lay in lays:
        batch = lay.device()
        for params in TE.PARAMETER_SETS:
            _assert_translate(batch, lay.texts, params, (lay.name, params))


def test_strip_in_every_layout():
    texts = TC.strip_texts(b" ") + TC.mixed_texts(40, 13, longest=60)
    lays = LY.layouts_for(texts, _strip_poison)
    with_outside = changed = 0
    for lay in lays:
        for i, t in enumerate(lay.texts):
            outside = lay.outside(i)
            if outside:
                with_outside += 1
                changed += TE.strip(t + outside) != TE.strip(t)
    assert with_outside > 300 and 2 * changed >= with_outside, (with_outside, changed)
    for lay in lays:
        batch = lay.device()
        for opts in TE.STRIPS:
            prefix, rows = batch.strip(spans=True, **opts)
            assert np.array_equal(_np(rows), TE.strip_rows(lay.texts, **opts)), (lay.name, opts)
            assert _np(prefix).tolist() == list(range(batch.n + 1))
    _scratch_is_returned()


@pytest.mark.parametrize("piece", [0, 1024], ids=["default_piece", "piece_1024"])
def test_every_case_at_two_piece_lengths(piece):
    lib = M.load_library()
    try:
        P = lib.mrx_debug_translate_piece(piece)
        assert P == (piece or TC.piece_length())
        for name, texts in TC.all_cases(P).items():
            batch = M.DeviceBatch.from_texts(texts)
            for params in (TE.PARAMETER_SETS if piece == 0 else TE.PACKED):   # (the same-length form has no pieces)
                _assert_translate(batch, texts, params, (name, params, P), _want((name, P), texts, params))
    finally:
        assert lib.mrx_debug_translate_piece(0) == TC.piece_length()


def test_strip_cases():
    for opts in TE.STRIPS:
        chars = opts.get("chars")
        s = b" " if not chars else chars[:1]
        for texts in (TC.strip_texts(s), TC.strip_texts(s, b"\n" if chars else b"Z")[::-1], []):
            batch = M.DeviceBatch.from_texts(texts)
            prefix, rows = batch.strip(spans=True, **opts)
            want = TE.strip_rows(texts, **opts)
            assert np.array_equal(_np(rows), want), opts
            assert _np(prefix).tolist() == list(range(len(texts) + 1))
            # strip() is strip(spans=True) followed by gather_spans
            got = batch.strip(**opts)
            assert _texts_of(got) == _texts_of(batch.gather_spans(prefix, rows)[0]) == [t[a:b] for t, ((a, b),) in zip(texts, want)]
    _scratch_is_returned()


def test_the_same_length_form_keeps_the_layout_and_writes_nothing_else():
    import torch
    lib = M.load_library()
    texts = TC.mixed_texts(50, 17, longest=90)
    pz = _poison(3)
    known = M.DeviceBatch.from_texts(texts)
    assert known._end_offset is not None
    for lay in [LY.csr_shifted(texts, s, pz) for s in LY.CSR_SHIFTS] + [LY.ragged_rows(texts, False, pz), LY.whole_rows(texts, 50, pz)]:
        batch = lay.device()
        for table in (TE.LOWER, TE.PERMUTATION):
            out = torch.full((batch.data.numel() + 64,), 0xA5, dtype=torch.uint8, device="cuda")[32:32 + batch.data.numel()]
            whole = out._base if out._base is not None else out
            batch.translate_async((out, None, None), table)
            torch.cuda.synchronize()
            got, src = _np(whole), lay.buf
            a, b = (int(lay.offsets[0]), int(lay.offsets[-1])) if lay.csr else (0, len(lay.texts) * lay.stride)
            assert np.all(got[:32 + a] == 0xA5) and np.all(got[32 + b:] == 0xA5), lay.name   # nothing outside the region
            want = np.frombuffer(src[a:b].tobytes().translate(table), np.uint8)
            for i in range(len(lay.texts)):   # (a fixed pitch's row padding is unspecified)
                s, e = lay.span(i)
                assert np.array_equal(got[32 + s:32 + e], want[s - a:e - a]), (lay.name, i)
    # known bounds: nothing is read back, and the result carries them
    before = lib.mrx_debug_translate_syncs()
    res = known.lower()
    strided = LY.fixed_length(texts, 64, 45, pz)
    res2 = strided.device().upper()
    assert lib.mrx_debug_translate_syncs() == before
    assert res.offsets is known.offsets and (res._end_offset, res._max_len) == (known._end_offset, known._max_len)
    assert _texts_of(res) == [t.lower() for t in texts] and _texts_of(res2) == [t.upper() for t in strided.texts]
    unknown = M.DeviceBatch(known.data, known.offsets)
    assert _texts_of(unknown.upper()) == [t.upper() for t in texts]
    assert lib.mrx_debug_translate_syncs() == before + 1   # the first and last offset, once
    with pytest.raises(M.MrxError):   # a region that does not fit is refused before anything runs
        known.translate_async((torch.empty(known.data.numel() - 1, dtype=torch.uint8, device="cuda"), None, None), TE.LOWER)
    _scratch_is_returned()


def test_async_equals_sync_and_reads_nothing_back():
    import torch
    lib = M.load_library()
    texts = TC.mixed_texts(64, 19, longest=120)
    rows = [(t + b" " * 128)[:128] for t in texts]
    raw = torch.from_numpy(np.frombuffer(b"".join(rows), np.uint8).copy()).cuda()
    known = M.DeviceBatch.from_texts(texts)
    batches = [(M.DeviceBatch.strided(raw, 128, length=128), rows, 0), (known, texts, 0),
               (M.DeviceBatch(known.data, known.offsets), texts, 1)]
    for batch, its_texts, reads in batches:
        for params in TE.PACKED:
            woff, wdata, wtot = TE.expected(its_texts, **params)
            out = (torch.full((wtot[0] + 5,), 0xA5, dtype=torch.uint8, device="cuda"),
                   torch.full((batch.n + 1 + 3,), -7, dtype=torch.int64, device="cuda"), torch.full((2 + 2,), -7, dtype=torch.int64, device="cuda"))
            before = lib.mrx_debug_translate_syncs()
            batch.translate_async(out, **params)
            assert lib.mrx_debug_translate_syncs() - before == reads
            _scratch_is_returned()
            torch.cuda.synchronize()
            data, off, tot = (_np(t) for t in out)
            assert tot.tolist() == wtot + [-7, -7] and np.array_equal(off[:batch.n + 1], woff) and np.all(off[batch.n + 1:] == -7), params
            assert np.array_equal(data[:wtot[0]], wdata) and np.all(data[wtot[0]:] == 0xA5), params
            sync = batch.translate(**params)
            assert np.array_equal(_np(sync.offsets), woff) and np.array_equal(_np(sync.data)[:wtot[0]], wdata)
        # strip on the caller's tensors
        srows = torch.full((batch.n + 2, 1, 2), -7, dtype=torch.int32, device="cuda")
        sprefix = torch.full((batch.n + 1 + 2,), -7, dtype=torch.int64, device="cuda")
        before = lib.mrx_debug_translate_syncs()
        batch.strip_async((sprefix, srows), b" \r")
        assert lib.mrx_debug_translate_syncs() == before
        torch.cuda.synchronize()
        assert np.array_equal(_np(srows)[:batch.n], TE.strip_rows(its_texts, b" \r")) and np.all(_np(srows)[batch.n:] == -7)
        assert _np(sprefix).tolist() == list(range(batch.n + 1)) + [-7, -7]


def test_a_capacity_one_byte_short_writes_no_byte():
    import torch
    texts = TC.mixed_texts(50, 23, n_long=2, P=TC.piece_length())
    for batch in (LY.csr_packed(texts).device(), LY.ragged_rows(texts, False, _poison(2)).device()):
        for params in (dict(delete=b"\r"), dict(squeeze=b" ")):
            woff, wdata, wtot = TE.expected(texts, **params)
            table, dele, sq = M.api._translate_args(**params)
            for short in (1, 0):
                cap = wtot[0] - short
                out = torch.full((cap + 32,), 0xEE, dtype=torch.uint8, device="cuda")
                off = torch.full((batch.n + 1 + 4,), -7, dtype=torch.int64, device="cuda")
                d_tot = torch.full((2 + 2,), -7, dtype=torch.int64, device="cuda")
                tot = (C.c_int64 * 2)(-1, -1)
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                rc = batch.call(M.load_library(), "mrx_translate", (table, dele, sq),
                                (out.data_ptr(), cap, off.data_ptr(), d_tot.data_ptr(), C.cast(tot, C.c_void_p), stream))
                torch.cuda.synchronize()
                assert rc == (CAPACITY if short else OK) and list(tot) == wtot and _np(d_tot).tolist() == wtot + [-7, -7]
                assert np.array_equal(_np(off)[:batch.n + 1], woff) and np.all(_np(off)[batch.n + 1:] == -7)
                got = _np(out)
                assert np.all(got[cap:] == 0xEE) and (np.all(got == 0xEE) if short else np.array_equal(got[:cap], wdata))
    _scratch_is_returned()


def test_translate_and_strip_in_front_of_the_next_call():
    rng = np.random.default_rng(29)
    hosts = [bytes(rng.choice([b"Example.COM", b"example.com", b"EXAMPLE.com", b"Other.org", b"other.ORG", b"third.net"])) for _ in range(300)]
    batch = M.DeviceBatch.from_texts(hosts)
    values, counts, _, _ = batch.lower().distinct()
    want_values, want_counts, _, _ = M.DeviceBatch.from_texts([t.lower() for t in hosts]).distinct()
    assert _texts_of(values) == _texts_of(want_values) and _np(counts).tolist() == _np(want_counts).tolist()
    assert sorted(_texts_of(values)) == [b"example.com", b"other.org", b"third.net"] and int(counts.sum()) == 300
    # a CSV cell stripped before it is parsed: the rows go into parse_spans as they stand
    cells = M.DeviceBatch.from_texts([b"  42 ", b"7", b"\t-13\r\n", b"   ", b" 4 2 "])
    assert _np(cells.parse()[1]).tolist()[0] != M.api.MRX_NUM_OK           # b"  42 " does not parse as it stands
    prefix, rows = cells.strip(spans=True)
    values, status, _ = cells.parse_spans(prefix, rows)
    assert _np(status).tolist()[:3] == [M.api.MRX_NUM_OK] * 3 and _np(values).tolist()[:3] == [42, 7, -13]
    assert _np(status).tolist()[3] == M.api.MRX_NUM_EMPTY and _np(status).tolist()[4] == M.api.MRX_NUM_MALFORMED
    _scratch_is_returned()


def test_the_host_list_functions():
    texts = TC.mixed_texts(80, 31, longest=100)
    for params in TE.PARAMETER_SETS:
        assert M.translate_texts(texts, **params) == [TE.translate(t, **params) for t in texts], params
    assert M.translate_texts([]) == [] and M.strip_texts([]) == []
    assert M.strip_texts(texts) == [t.strip() for t in texts]
    assert M.strip_texts(texts, b" \rab", right=False) == [t.lstrip(b" \rab") for t in texts]
    assert M.strip_texts(texts, left=False) == [t.rstrip() for t in texts]
    assert M.translate_texts(["Grüße", b"ABC"], bytes(range(256)).lower()) == ["grüße".encode(), b"abc"]   # ASCII only, as Python's
    with pytest.raises(M.MrxError):
        M.DeviceBatch.from_texts(texts).translate(b"short")
    with pytest.raises(M.MrxError):
        M.DeviceBatch.from_texts(texts).translate(delete=b"a", squeeze=b"b")
    with pytest.raises(M.MrxError):
        M.DeviceBatch.from_texts(texts).strip(left=False, right=False)
    _scratch_is_returned()
