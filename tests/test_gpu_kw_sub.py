"""Keywords.leftmost / sub / subn on the GPU, bit for bit against re (tests/kw_sub_expect.py): every layout of
tests/layouts.py with the pieces pinned small and at the rule's size, with and without the LDS tier, the piece
boundaries, the right-hand warm-up at a text's end, long and headless texts, an automaton far beyond the LDS tier, the
capacity rules, the round trips and the lazy build of the reversed automaton."""
import ctypes as C

import numpy as np
import pytest

import mojo_regex_amd as M
import kw_sub_expect as SE
import keywords_expect as KE
import layouts as LY

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _poison(entries, seed=0):
    """Bytes around the texts that would make other matches if they were read as text."""
    rng = np.random.default_rng(900 + seed)
    joined = b"".join(entries)

    def pz(i, t, k):
        if k <= 0:
            return b""
        e = entries[int(rng.integers(0, len(entries)))]
        kind = int(rng.integers(0, 3))
        fill = e[int(rng.integers(0, len(e))):] + joined if kind == 0 else (t + e) * (k + 1) if kind == 1 else joined
        while len(fill) < k:
            fill += joined
        return fill[:k]
    return pz


@pytest.fixture(autouse=True)
def _hooks_back():
    yield
    lib = M.load_library()
    lib.mrx_debug_kw_piece(0)
    lib.mrx_debug_kw_tier(1)


def _texts_of(batch):
    raw, off = _np(batch.data).tobytes(), _np(batch.offsets)
    return [raw[off[i]:off[i + 1]] for i in range(batch.n)]


def _check_layout(kw, entries, repls, lay, want_of, what="", counts=(0, 2)):
    """leftmost, sub and subn of one layout against the helper; want_of caches the helper's answers per text tuple."""
    batch = lay.device()
    for count in counts:
        key = (tuple(lay.texts), count)
        if key not in want_of:
            want_of[key] = (SE.leftmost(entries, lay.texts, False, count),) + tuple(
                SE.sub(entries, r, lay.texts, False, count) for r in repls)
        want = want_of[key]
        wp, we, ws = SE.arrays(want[0])
        prefix, ents, spans = kw.leftmost(batch, count)
        assert _np(prefix).tolist() == wp.tolist(), (what, lay.name, count)
        assert _np(ents).tolist() == we.tolist() and _np(spans).tolist() == ws.tolist(), (what, lay.name, count)
        for repl, (wo, wn) in zip(repls, want[1:]):
            res, nsub = kw.subn(repl, batch, count)
            assert _np(nsub).tolist() == wn.tolist(), (what, lay.name, count)
            assert _texts_of(res) == wo, (what, lay.name, count)
            assert res._end_offset == sum(map(len, wo)) and res._max_len == max(map(len, wo), default=0)


@pytest.fixture(scope="module")
def generated():
    rng = np.random.default_rng(78)
    entries, texts = KE.generated(rng, 24, 300)
    assert max(len(e) for e in entries) > 32 and min(len(t) for t in texts) == 0
    repls = [bytes(rng.integers(65, 91, size=int(k)).astype(np.uint8)) for k in rng.integers(0, 71, size=len(entries))]
    repls[0], repls[1] = b"", b"R" * 70
    lays = LY.layouts_for(texts, _poison(entries))
    return entries, texts, lays, (b"<gone>!!", repls), {}


@pytest.mark.parametrize("piece", [16, 0])
def test_generated_entries_in_every_layout(generated, piece):
    entries, texts, lays, repls, cache = generated
    lib = M.load_library()
    kw = M.Keywords(entries)
    lib.mrx_debug_kw_piece(piece)
    for lay in lays:
        _check_layout(kw, entries, repls, lay, cache, "piece %d" % piece)
    assert lib.mrx_last_kernel_name() == b"k_kw_sub_gather"
    assert len(lays) >= 12
    assert kw.sub(b"-", texts[:40]) == SE.sub(entries, b"-", texts[:40])[0]              # lists, through from_texts
    assert kw.leftmost_lists(texts[:40], 1) == SE.leftmost(entries, texts[:40], False, 1)   # ... and the host-buffer form


def test_without_the_lds_tier(generated):
    entries, texts, lays, repls, cache = generated
    lib = M.load_library()
    kw = M.Keywords(entries)
    lib.mrx_debug_kw_tier(0)
    for piece in (16, 0):
        lib.mrx_debug_kw_piece(piece)
        for lay in (lays[2], lays[5]):   # CSR shifted by 7, lens at an unaligned pitch
            _check_layout(kw, entries, repls, lay, cache, "no tier, piece %d" % piece)


def test_piece_boundaries_and_the_right_hand_warm_up():
    lib = M.load_library()
    entries = [b"vwxyz", b"abc", b"wx", b"z"]
    f = b"q" * 64
    texts = [f[:k] + b"vwxyz" + f[:20] for k in range(10, 17)]       # starts at the last 6 positions of a piece and the next's first
    texts += [f[:k] + b"vwxyz" for k in range(10, 17)]               # ... and ends exactly at the text's end
    texts += [f[:14] + b"ab", b"c" + f[:9], f[:15] + b"vwxy", b"z", b"", f[:16] + b"vw", b"xyz"]   # packed neighbours complete an entry
    want = SE.leftmost(entries, texts)
    assert want[14] == [] and want[15] == [] and want[16] == [(2, 16, 18)] and want[19] == [] and want[20] == [(3, 2, 3)]
    kw = M.Keywords(entries)
    lays = LY.layouts_for(texts, _poison(entries, 1))
    # a fixed-pitch row whose padding would complete the entry that its text ends in
    rows = [b"q" * 13 + b"ab" + b"c" * 17, b"q" * 30 + b"vw" + b"xyzvwxyz" * 2]
    lens = np.array([15, 32], np.int32)
    pad = LY.Layout("padding", np.frombuffer(b"".join(r[:48].ljust(48, b"z") for r in rows), np.uint8).copy(),
                    [rows[0][:15], rows[1][:32]], stride=48, lens=lens)
    pad.check()
    assert SE.leftmost(entries, pad.texts) == [[], []]
    cache = {}
    for piece in (16, 32, 0):
        lib.mrx_debug_kw_piece(piece)
        for lay in lays + [pad]:
            _check_layout(kw, entries, (b"#", [b"5five", b"", b"22", b"1"]), lay, cache, "piece %d" % piece, counts=(0,))


def test_long_headless_and_empty_texts():
    lib = M.load_library()
    rng = np.random.default_rng(6)
    letters = np.frombuffer(b"abc", np.uint8)
    entries = sorted({letters[rng.integers(0, 3, size=int(rng.integers(2, 13)))].tobytes() for _ in range(230)})[:200]
    big = letters[rng.integers(0, 3, size=256 * 1024)].tobytes()
    kw = M.Keywords(entries)
    want = SE.leftmost(entries, [big])
    assert len(want[0]) > 20000
    batch = M.DeviceBatch(M.DeviceBatch.from_texts([big]).data, M.DeviceBatch.from_texts([big]).offsets)   # bounds not known
    prefix, ents, spans = kw.leftmost(batch)
    assert _np(prefix).tolist() == [0, len(want[0])]
    assert list(zip(_np(ents).tolist(), *_np(spans).T.tolist())) == want[0]
    assert _texts_of(kw.sub(b"<>", batch)) == SE.sub(entries, b"<>", [big])[0]
    head = M.Keywords([b"a", b"aa", b"aaa"])
    texts = [b"", b"a" * 4099, b"", b"", b"aaaa"]
    lib.mrx_debug_kw_piece(16)                                       # one chain across 257 pieces
    assert head.leftmost_lists(texts) == SE.leftmost([b"a", b"aa", b"aaa"], texts)
    res, nsub = head.subn([b"1", b"22", b"333"], M.DeviceBatch.from_texts(texts))
    assert _texts_of(res) == [b"", b"333" * 1366 + b"1", b"", b"", b"3331"] and _np(nsub).tolist() == [0, 1367, 0, 0, 2]
    lib.mrx_debug_kw_piece(0)
    assert head.sub(b"", [b"", b"", b""]) == [b"", b"", b""]
    empty = M.DeviceBatch.from_texts([])
    prefix, ents, spans = head.leftmost(empty)
    assert _np(prefix).tolist() == [0] and ents.numel() == 0
    res, nsub = head.subn(b"x", empty)
    assert res.n == 0 and _np(res.offsets).tolist() == [0] and nsub.numel() == 0
    none = M.Keywords([])                                            # m == 0: the output is the input
    assert none.sub(b"x", [b"abc", b""]) == [b"abc", b""] and none.leftmost_lists([b"abc"]) == [[]]


def test_a_large_automaton():
    rng = np.random.default_rng(20001)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    entries = [letters[rng.integers(0, 26, size=int(rng.integers(3, 13)))].tobytes() for _ in range(20000)]
    texts = []
    for _ in range(2000):
        t = b""
        while len(t) < 48:
            t += entries[int(rng.integers(0, len(entries)))] if rng.random() < 0.4 else \
                letters[rng.integers(0, 26, size=int(rng.integers(1, 9)))].tobytes()
        texts.append(t[:int(rng.integers(20, 49))])
    repls = [b"<%d>" % j for j in range(len(entries))]
    kw = M.Keywords(entries)
    want = SE.leftmost(entries, texts)
    assert sum(len(w) for w in want) > 2000
    batch = LY.csr_shifted(texts, 7, _poison(entries[:50], 2)).device()
    prefix, ents, spans = kw.leftmost(batch)
    wp, we, ws = SE.arrays(want)
    assert _np(prefix).tolist() == wp.tolist() and _np(ents).tolist() == we.tolist() and _np(spans).tolist() == ws.tolist()
    res, nsub = kw.subn(repls, batch)
    wo, wn = SE.sub(entries, repls, texts)
    assert _texts_of(res) == wo and _np(nsub).tolist() == wn.tolist()


def test_capacity():
    import torch
    lib = M.load_library()
    entries, texts = [b"a", b"ab", b"ba"], [b"aabab", b"", b"bbab", b"xyz"]
    want = SE.leftmost(entries, texts)
    wp, we, ws = SE.arrays(want)
    need = int(wp[-1])
    kw = M.Keywords(entries)
    batch = M.DeviceBatch.from_texts(texts)
    ptr = M.api._ptr
    n = batch.n
    prefix = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    ents = torch.full((need + 4,), -9, dtype=torch.int32, device="cuda")
    spans = torch.full((need + 4, 2), -9, dtype=torch.int32, device="cuda")
    tot = C.c_int64(-1)
    for cap in (0, need - 1):
        rc = lib.mrx_kw_leftmost_dev(kw._h, 0, ptr(batch.data), ptr(batch.offsets), n, ptr(prefix), ptr(ents), ptr(spans), cap,
                                     C.byref(tot), None)
        torch.cuda.synchronize()
        assert rc == M.api.MRX_E_CAPACITY and tot.value == need and _np(prefix).tolist() == wp.tolist()
        assert _np(ents)[cap:].tolist() == [-9] * (need + 4 - cap) and (_np(spans)[cap:] == -9).all()
    rc = lib.mrx_kw_leftmost_dev(kw._h, 0, ptr(batch.data), ptr(batch.offsets), n, ptr(prefix), ptr(ents), ptr(spans), need,
                                 C.byref(tot), None)
    torch.cuda.synchronize()
    assert rc == M.api.MRX_OK and _np(ents)[:need].tolist() == we.tolist() and _np(spans)[:need].tolist() == ws.tolist()
    assert _np(ents)[need:].tolist() == [-9] * 4
    with pytest.raises(M.MrxError):
        kw.leftmost(batch, span_cap=need - 1)
    wo, wn = SE.sub(entries, b"[gone]", texts)
    nbytes = sum(map(len, wo))
    rows = kw._repl_batch(b"[gone]", "cuda")
    out_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    out = torch.full((nbytes + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    nsub = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_tot = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    totals = (C.c_int64 * 3)(-1, -1, -1)
    args = lambda cap: (kw._h, ptr(rows.data), ptr(rows.offsets), 1, 0, ptr(batch.data), ptr(batch.offsets), n, ptr(out_off),
                        ptr(out), cap, ptr(nsub), ptr(d_tot), C.cast(totals, C.c_void_p), None)
    rc = lib.mrx_kw_sub_dev(*args(nbytes - 1))
    torch.cuda.synchronize()
    assert rc == M.api.MRX_E_CAPACITY and list(totals) == [nbytes, max(map(len, wo)), need] == _np(d_tot).tolist()
    assert (_np(out) == 0xEE).all() and _np(nsub).tolist() == wn.tolist()
    assert _np(out_off).tolist() == np.concatenate([[0], np.cumsum([len(w) for w in wo])]).astype(int).tolist()
    rc = lib.mrx_kw_sub_dev(*args(nbytes))                                            # the retry
    torch.cuda.synchronize()
    assert rc == M.api.MRX_OK and _np(out)[:nbytes].tobytes() == b"".join(wo) and (_np(out)[nbytes:] == 0xEE).all()
    assert lib.mrx_kw_sub_dev(kw._h, ptr(rows.data), ptr(rows.offsets), 2, 0, ptr(batch.data), ptr(batch.offsets), n,
                              ptr(out_off), ptr(out), nbytes, None, None, None, None) == M.api.MRX_E_ARGUMENT   # r is 1 or m
    with pytest.raises(M.MrxError):
        kw.sub([b"x", b"y"], batch)
    with pytest.raises(M.MrxError):
        kw.sub(b"[gone]", batch, out_cap=nbytes - 1)
    assert kw.sub(b"[gone]", texts) == wo and M.keywords_sub(entries, b"[gone]", texts, count=1) == \
        SE.sub(entries, b"[gone]", texts, False, 1)[0]


def test_round_trips_and_the_lazy_build():
    entries = [b"Error", b"warn", b"disk full", b"err"]
    texts = [b"an ERROR and an error; Warning: DISK FULL", b"eRrOr", b"nothing here", b"", b"an ERROR and an error; Warning: DISK FULL"]
    kw = M.Keywords(entries, ignore_case=True)
    desc = kw.describe()
    assert kw.contains(texts).tolist() == [True, True, False, False, True]             # before the reversed build
    batch = M.DeviceBatch.from_texts(texts)
    red = kw.sub(b"***", batch)
    wo = SE.sub(entries, b"***", texts, True)[0]
    assert _texts_of(red) == wo and wo[0] == b"an *** and an ***; ***ing: ***"
    assert kw.findall_lists(texts) == KE.findall(entries, texts, True) and kw.describe() == desc
    values, counts = red.distinct()[:2]                                                # no read-back of bounds in between
    assert sorted(_texts_of(values)) == sorted(set(wo))
    assert _np(M.Keywords([b"***"]).count(red)).tolist() == [w.count(b"***") for w in wo]
    per = [b"<E>", b"<W>", b"", b"<e>"]
    assert _texts_of(kw.sub(M.DeviceBatch.from_texts(per), batch)) == _texts_of(kw.sub(per, batch)) == \
        SE.sub(entries, per, texts, True)[0]
    assert _texts_of(kw.sub(M.DeviceBatch.from_texts([b"#"]), batch, count=1)) == SE.sub(entries, b"#", texts, True, 1)[0]
