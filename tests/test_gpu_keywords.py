"""Keywords on the GPU against bytes.find (tests/keywords_expect.py): contains, count and findall bit for bit in every
layout of tests/layouts.py with the pieces pinned small and at the rule's size, the piece boundaries, the capacity
rule, one long text, an automaton far beyond the LDS tier, folding and duplicates, the filter, the round trip through
gather_spans and the agreement with the pattern sets' findall."""
import ctypes as C

import numpy as np
import pytest

import mojo_regex_amd as M
import keywords_expect as KE
import layouts as LY

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _poison(entries, seed=0):
    """Bytes around the texts that would make other hits if they were read as text: the entries themselves, the
    remainder of an entry behind each of its prefixes, and the text once more."""
    rng = np.random.default_rng(500 + seed)
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


def _check_layout(kw, lay, want, what=""):
    """contains, count and findall of one layout against the helper's lists."""
    batch = lay.device()
    prefix, ents, spans = kw.findall(batch)
    wp, we, ws = KE.arrays(want)
    assert _np(prefix).tolist() == wp.tolist(), (what, lay.name)
    assert _np(ents).tolist() == we.tolist(), (what, lay.name)
    assert _np(spans).tolist() == ws.tolist(), (what, lay.name)
    assert _np(kw.count(batch)).tolist() == KE.counts(want).tolist(), (what, lay.name)
    assert _np(kw.contains(batch)).tolist() == (KE.counts(want) > 0).tolist(), (what, lay.name)


@pytest.fixture(scope="module")
def generated():
    rng = np.random.default_rng(77)
    entries, texts = KE.generated(rng, 24, 300)
    assert max(len(e) for e in entries) > 32 and min(len(t) for t in texts) == 0
    lays = LY.layouts_for(texts, _poison(entries))
    wants = {}
    for lay in lays:
        key = tuple(lay.texts)
        if key not in wants:
            wants[key] = KE.findall(entries, lay.texts)
    return entries, texts, lays, wants


@pytest.mark.parametrize("piece", [16, 0])
def test_generated_entries_in_every_layout(generated, piece):
    entries, texts, lays, wants = generated
    lib = M.load_library()
    kw = M.Keywords(entries)
    assert len(kw) == 24 and kw.distinct_count == len(set(entries))
    lib.mrx_debug_kw_piece(piece)
    names = set()
    for lay in lays:
        _check_layout(kw, lay, wants[tuple(lay.texts)], "piece %d" % piece)
        names.add(lay.name)
    assert lib.mrx_last_kernel_name() in (b"k_kw_count", b"k_kw_emit")
    assert {"csr_packed", "csr_shift1", "csr_shift7", "csr_shift15"} <= names and len(names) == len(lays) >= 12


def test_without_the_lds_tier(generated):
    entries, texts, lays, wants = generated
    lib = M.load_library()
    kw = M.Keywords(entries)
    lib.mrx_debug_kw_tier(0)
    for piece in (16, 0):
        lib.mrx_debug_kw_piece(piece)
        for lay in (lays[2], lays[5]):   # CSR shifted by 7, lens at an unaligned pitch
            _check_layout(kw, lay, wants[tuple(lay.texts)], "no tier, piece %d" % piece)


def test_piece_boundaries():
    lib = M.load_library()
    long_e = b"abcabcabcaabbccabcabcabcaabbccabcabc"            # 36 bytes: three pieces of 16, a warm-up of 35
    entries = [b"xyz", long_e, b"abc", b"c", b"zx"]
    f = b"q" * 64
    texts = [
        f[:13] + b"xyz" + f[:20],              # a hit that ends exactly on a piece's last byte (end 16)
        f[:14] + b"xyz" + f[:20],              # ... on the next piece's first byte (end 17)
        f[:15] + b"xyz" + f[:20],              # ... that begins on a piece's last byte
        f[:10] + long_e + f[:10],              # a hit across three pieces
        f[:15] + long_e,                       # ... that ends with the text
        long_e,                                # the whole text
        b"xyz" + f[:30] + b"xyz",              # hits at the text's first and last byte
        b"c", b"zx", b"xyz", b"", b"abc",      # texts shorter than the warm-up
        f[:30] + b"ab",                        # text i ends `ab` ...
        b"c" + f[:5],                          # ... and text i + 1 begins `c`: only `c` occurs here, at 0
        f[:31] + b"xy", b"z" + f[:15] + b"x", b"yz",   # the same across a piece's end, and split entries everywhere
        long_e[:-1], long_e[1:] + b"abc",      # all but one byte of the long entry
    ]
    want = KE.findall(entries, texts)
    assert want[12] == [] and want[13] == [(3, 0, 1)]
    assert want[0] == [(0, 13, 16)] and want[1] == [(0, 14, 17)] and (1, 10, 46) in want[3]
    kw = M.Keywords(entries)
    lays = LY.layouts_for(texts, _poison(entries, 1))
    cache = {}
    for piece in (16, 32, 0):
        lib.mrx_debug_kw_piece(piece)
        for lay in lays:
            key = tuple(lay.texts)
            if key not in cache:
                cache[key] = KE.findall(entries, lay.texts)
            _check_layout(kw, lay, cache[key], "piece %d" % piece)


def test_capacity():
    import torch
    lib = M.load_library()
    entries = [b"a", b"aa", b"ba"]
    texts = [b"aaaa", b"", b"abab", b"bbb", b"baaa"]
    want = KE.findall(entries, texts)
    wp, we, ws = KE.arrays(want)
    total = int(wp[-1])
    assert total == 16
    kw = M.Keywords(entries)
    batch = M.DeviceBatch.from_texts(texts)
    ptr = M.api._ptr
    for cap in (0, 5, total - 1):
        prefix = torch.full((len(texts) + 1,), -1, dtype=torch.int64, device="cuda")
        ents = torch.full((total + 4,), -9, dtype=torch.int32, device="cuda")
        spans = torch.full((total + 4, 2), -9, dtype=torch.int32, device="cuda")
        tot = C.c_int64(-1)
        rc = lib.mrx_kw_findall_dev(kw._h, ptr(batch.data), ptr(batch.offsets), batch.n, ptr(prefix), ptr(ents), ptr(spans),
                                    cap, C.byref(tot), None)
        torch.cuda.synchronize()
        assert rc == M.api.MRX_E_CAPACITY and tot.value == total, cap
        assert b"need 16" in lib.mrx_last_error()
        assert _np(prefix).tolist() == wp.tolist()
        assert _np(ents)[cap:].tolist() == [-9] * (total + 4 - cap)            # nothing at or beyond span_cap
        assert (_np(spans)[cap:] == -9).all()
    rc = lib.mrx_kw_findall_dev(kw._h, ptr(batch.data), ptr(batch.offsets), batch.n, ptr(prefix), ptr(ents), ptr(spans),
                                tot.value, C.byref(tot), None)                       # the retry with the total
    torch.cuda.synchronize()
    assert rc == M.api.MRX_OK and tot.value == total
    assert _np(ents)[:total].tolist() == we.tolist() and _np(spans)[:total].tolist() == ws.tolist()
    assert _np(ents)[total:].tolist() == [-9] * 4 and (_np(spans)[total:] == -9).all()   # the canary rows behind it
    with pytest.raises(M.MrxError):
        kw.findall(batch, span_cap=3)
    assert [len(h) for h in kw.findall_lists(texts)] == KE.counts(want).tolist()     # grows by itself


def test_one_long_text_and_the_small_batches():
    rng = np.random.default_rng(5)
    entries = [b"abca", b"bb", b"cabcab", b"a" * 9, b"abcabcabcabcabcabcabcabc"]
    big = np.frombuffer(b"abc", np.uint8)[rng.integers(0, 3, size=256 * 1024)].tobytes()
    big = big[:1000] + b"abc" * 20 + big[1060:]
    kw = M.Keywords(entries)
    want = KE.findall(entries, [big])
    assert len(want[0]) > 10000
    assert kw.findall_lists([big]) == want                                          # n = 1, the host-buffer form
    batch = M.DeviceBatch(M.DeviceBatch.from_texts([big]).data, M.DeviceBatch.from_texts([big]).offsets)   # bounds not known
    prefix, ents, spans = kw.findall(batch)
    assert _np(prefix).tolist() == [0, len(want[0])]
    assert list(zip(_np(ents).tolist(), *_np(spans).T.tolist())) == want[0]
    assert _np(kw.count(batch)).tolist() == [len(want[0])]
    assert kw.findall_lists([]) == []                                               # n = 0
    empty = M.DeviceBatch.from_texts([])
    prefix, ents, spans = kw.findall(empty)
    assert _np(prefix).tolist() == [0] and ents.numel() == 0 and spans.shape == (0, 2)
    assert kw.count(empty).numel() == 0 and kw.contains(empty).numel() == 0
    assert kw.findall_lists([b"", b"", b""]) == [[], [], []]                        # texts without a byte
    assert kw.count([b"", b"bb", b""]).tolist() == [0, 1, 0]
    assert kw.contains([b"", b"bb", b""]).tolist() == [False, True, False]
    none = M.Keywords([])                                                           # m == 0: nothing occurs
    assert len(none) == 0 and none.count([b"abc", b""]).tolist() == [0, 0]
    assert none.findall_lists([b"abc"]) == [[]]
    assert none.filter([b"abc", b""])[0] == [] and none.filter([b"abc", b""], invert=True)[0] == [b"abc", b""]


def test_a_large_automaton():
    rng = np.random.default_rng(20000)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    entries = [letters[rng.integers(0, 26, size=int(rng.integers(3, 13)))].tobytes() for _ in range(20000)]
    texts = []
    for _ in range(240):
        t = b""
        while len(t) < 200:
            t += entries[int(rng.integers(0, len(entries)))] if rng.random() < 0.4 else \
                letters[rng.integers(0, 26, size=int(rng.integers(1, 9)))].tobytes()
        texts.append(t[:200])
    kw = M.Keywords(entries)
    desc = kw.describe()
    fields = dict(p.split("=") for p in desc.split()[1:])
    assert int(fields["m"]) == 20000 and int(fields["classes"]) == 27 and int(fields["lmax"]) == 12
    assert int(fields["table_bytes"]) > 8 << 20 and int(fields["states"]) * 27 * 4 == int(fields["table_bytes"])
    want = KE.findall(entries, texts)
    assert sum(len(w) for w in want) > 2000
    for lay in (LY.csr_shifted(texts, 7, _poison(entries[:50], 2)), LY.fixed_length(texts, 208, 200, _poison(entries[:50], 3))):
        _check_layout(kw, lay, want if lay.texts == texts else KE.findall(entries, lay.texts))


def test_ignore_case_and_duplicates():
    entries = [b"Error", b"WARN", b"error", b"warn", b"disk full", b"ERROR", b"\xc4b", b"z"]
    texts = [b"an ERROR and an error; Warning: DISK FULL", b"eRrOr", b"nothing here", b"", b"\xe4b \xc4B \xc4b", b"Zz"]
    for ic in (False, True):
        kw = M.Keywords(entries, ignore_case=ic)
        assert len(kw) == 8 and kw.distinct_count == (5 if ic else 8)
        assert ("ignore_case=%d" % ic) in kw.describe()
        want = KE.findall(entries, texts, ic)
        for lay in (LY.csr_packed(texts), LY.ragged_rows(texts, False, _poison(entries, 4))):
            _check_layout(kw, lay, want, "ignore_case %s" % ic)
    folded = M.Keywords(entries, ignore_case=True).findall_lists(texts)
    assert folded[1] == [(0, 0, 5)] and folded[4] == [(6, 3, 5), (6, 6, 8)] and folded[5] == [(7, 0, 1), (7, 1, 2)]
    dup = M.build_keywords([b"ab", b"b", b"ab", b"b"])
    assert dup.distinct_count == 2 and dup.findall_lists([b"abab"]) == [[(0, 0, 2), (1, 1, 2), (0, 2, 4), (1, 3, 4)]]
    dev = M.Keywords(M.DeviceBatch.from_texts(entries), ignore_case=True)           # entries from the device
    assert dev.findall_lists(texts) == folded and dev.distinct_count == 5
    rows = LY.ragged_rows([b"ab", b"b", b"ab"], True, _poison([b"ab"], 5)).device()  # ... at a fixed pitch
    assert M.Keywords(rows).findall_lists([b"abab"]) == [[(0, 0, 2), (1, 1, 2), (0, 2, 4), (1, 3, 4)]]
    with pytest.raises(M.MrxError, match="entry 1 is empty"):
        M.Keywords([b"a", b"", b"c"])


def test_filter(generated):
    import torch
    entries, texts, lays, wants = generated
    few = [b"abca", b"cccb", b"babab"]
    kw = M.Keywords(few)
    ptr = M.api._ptr
    for lay in (lays[0], lays[3], lays[5], lays[-1]):
        hits = KE.findall(few, lay.texts)
        assert 0 < sum(1 for h in hits if h) < len(hits)
        batch = lay.device()
        for invert in (False, True):
            widx, woff, wout = KE.filtered(hits, lay.texts, invert)
            kept, idx = kw.filter(batch, invert=invert)
            assert _np(idx).tolist() == widx.tolist(), (lay.name, invert)
            assert _np(kept.offsets).tolist() == woff.tolist() and _np(kept.data).tobytes() == wout
            n, cap = batch.n, len(wout) + 32
            out = (torch.full((n,), -1, dtype=torch.int64, device="cuda"), torch.full((n + 1,), -1, dtype=torch.int64, device="cuda"),
                   torch.full((cap,), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((2,), -1, dtype=torch.int64, device="cuda"))
            kw.filter_async(batch, out, invert=invert)
            torch.cuda.synchronize()
            assert _np(out[3]).tolist() == [len(widx), len(wout)]
            assert _np(out[0])[:len(widx)].tolist() == widx.tolist() and _np(out[1])[:len(widx) + 1].tolist() == woff.tolist()
            assert _np(out[2])[:len(wout)].tobytes() == wout and (_np(out[2])[len(wout):] == 0x5A).all()
    # filter's capacity rule: indices, offsets and totals complete, no output byte written, MRX_E_CAPACITY with totals
    lay = lays[0]
    batch = lay.device()
    hits = KE.findall(few, lay.texts)
    widx, woff, wout = KE.filtered(hits, lay.texts)
    n, cap = batch.n, len(wout) - 1
    out = (torch.full((n,), -1, dtype=torch.int64, device="cuda"), torch.full((n + 1,), -1, dtype=torch.int64, device="cuda"),
           torch.full((len(wout) + 8,), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((2,), -1, dtype=torch.int64, device="cuda"))
    totals = (C.c_int64 * 2)(-1, -1)
    rc = batch.call(kw._lib, "mrx_kw_filter", (kw._h, 0), (ptr(out[0]), ptr(out[1]), ptr(out[2]), cap, ptr(out[3]),
                                                           C.cast(totals, C.c_void_p), None))
    torch.cuda.synchronize()
    assert rc == M.api.MRX_E_CAPACITY and list(totals) == [len(widx), len(wout)]
    assert _np(out[0])[:len(widx)].tolist() == widx.tolist() and _np(out[1])[:len(widx) + 1].tolist() == woff.tolist()
    assert (_np(out[2]) == 0x5A).all()
    # the one-shot form and lists
    kept, idx = M.keywords_filter(few, texts)
    assert kept == [texts[i] for i in widx.tolist()] and idx.tolist() == widx.tolist()
    kept, idx = M.keywords_filter(few, texts, invert=True)
    assert idx.tolist() == [i for i, h in enumerate(hits) if not h]


def test_round_trip_through_gather_spans(generated):
    entries, texts, lays, wants = generated
    kw = M.Keywords(entries)
    folded = M.Keywords([e.upper() for e in entries], ignore_case=True)
    for lay in (lays[1], lays[4]):
        batch = lay.device()
        for k, lower in ((kw, False), (folded, True)):
            prefix, ents, spans = k.findall(batch)
            pieces, owner = batch.gather_spans(prefix, spans)
            raw, off, e = _np(pieces.data).tobytes(), _np(pieces.offsets), _np(ents)
            assert len(e) == int(_np(prefix)[-1]) > 1000
            for q in range(len(e)):
                got = raw[off[q]:off[q + 1]]
                assert (got.upper() if lower else got) == (entries[e[q]].upper() if lower else entries[e[q]]), q
            assert _np(owner).tolist() == np.repeat(np.arange(batch.n), np.diff(_np(prefix))).tolist()


def test_agreement_with_the_pattern_sets_findall():
    """The set's findall is every member's own findall, the reference's: occurrences that overlap each other are reported
    for a literal on the exact-literal route and skipped for one on the DFA's literal route, which steps over a match.  A
    keyword set reports every occurrence.  The two say the same of an entry exactly when two of its occurrences cannot
    overlap, that is when no proper prefix of it is also its suffix, and such are the entries here."""
    rng = np.random.default_rng(9)
    al = np.frombuffer(b"abcXY019", np.uint8)
    entries = sorted({al[rng.integers(0, len(al), size=int(rng.integers(1, 7)))].tobytes() for _ in range(300)})
    entries = [e for e in entries if not any(e[:k] == e[-k:] for k in range(1, len(e)))][:256]
    assert 100 < len(entries) <= 256 and max(len(e) for e in entries) == 6 and min(len(e) for e in entries) == 1
    texts = [al[rng.integers(0, len(al), size=int(rng.integers(0, 120)))].tobytes() for _ in range(150)]
    texts += [b"abababab", b"aaaaaaaa", b""]
    batch = M.DeviceBatch.from_texts(texts)

    def rows(res):
        prefix, who, spans = (_np(t) for t in res)
        text = np.repeat(np.arange(len(texts)), np.diff(prefix))
        return sorted(zip(text.tolist(), spans[:, 1].tolist(), spans[:, 0].tolist(), who.tolist()))

    got = rows(M.Keywords(entries).findall(batch))
    want = rows(M.compile_set(entries).findall(batch))
    assert len(want) > 5000 and got == want
