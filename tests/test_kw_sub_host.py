"""Keywords.leftmost and Keywords.sub without a GPU: the expectation helper (tests/kw_sub_expect.py) against the literal
loop of the definition and on hand-traced cases, then the walk back, the selection, the rows and the block fill of the
kernels on the CPU (mrx_debug_kw_host_leftmost / mrx_debug_kw_host_sub: the same build, pieces and lanes) against the
helper, the capacity rules, the C ABI's symbols and its argument errors, all of which return before any device call."""
import numpy as np
import pytest

import mojo_regex_amd as M
import kw_sub_expect as SE

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C
OK, E_CAP, E_ARG = M.api.MRX_OK, M.api.MRX_E_CAPACITY, M.api.MRX_E_ARGUMENT


def _host_leftmost(entries, texts, ignore_case=False, count=0, piece=0, cap=None, skew=0):
    """mrx_debug_kw_host_leftmost -> (rc, lists per text, total, prefix)."""
    lib = M.load_library()
    ed, eo = M.pack_texts(entries)
    d, o = M.pack_texts(texts)
    if skew:
        d = np.concatenate([np.full(skew, ord("a"), np.uint8), d])
        o = o + skew
    n = len(texts)
    if cap is None:
        cap = sum(len(t) for t in texts) + 3
    prefix = np.full(n + 1, -1, np.int64)
    ents = np.full(cap + 2, -9, np.int32)
    spans = np.full((cap + 2, 2), -9, np.int32)
    tot = C.c_int64(-1)
    lib.mrx_debug_kw_piece(piece)
    try:
        rc = lib.mrx_debug_kw_host_leftmost(ed.ctypes.data, eo.ctypes.data, len(entries), 1 if ignore_case else 0, count,
                                            d.ctypes.data, o.ctypes.data, n, prefix.ctypes.data, ents.ctypes.data,
                                            spans.ctypes.data, cap, C.byref(tot))
    finally:
        lib.mrx_debug_kw_piece(0)
    assert ents[cap:].tolist() == [-9, -9] and spans[cap:].tolist() == [[-9, -9]] * 2   # nothing behind the capacity
    lists = None
    if rc == OK:
        lists = [[(int(ents[q]), int(spans[q, 0]), int(spans[q, 1])) for q in range(prefix[i], prefix[i + 1])]
                 for i in range(n)]
    else:
        assert (ents == -9).all() and (spans == -9).all()
    return rc, lists, int(tot.value), prefix


def _host_sub(entries, repl, texts, ignore_case=False, count=0, piece=0, cap=None, skew=0):
    """mrx_debug_kw_host_sub -> (rc, outputs, nsub, totals, out_offsets)."""
    lib = M.load_library()
    ed, eo = M.pack_texts(entries)
    rd, ro = M.pack_texts([repl] if isinstance(repl, bytes) else repl)
    rd = np.concatenate([rd, np.zeros(1, np.uint8)])   # (a pointer even for b"")
    d, o = M.pack_texts(texts)
    if skew:
        d = np.concatenate([np.full(skew, ord("a"), np.uint8), d])
        o = o + skew
    n = len(texts)
    if cap is None:
        cap = sum(len(t) for t in SE.sub(entries, repl, texts, ignore_case, count)[0]) + 5
    out_off = np.full(n + 1, -1, np.int64)
    out = np.full(cap + 40, 0xEE, np.uint8)
    nsub = np.full(max(n, 1), -1, np.int32)
    totals = (C.c_int64 * 3)(-1, -1, -1)
    lib.mrx_debug_kw_piece(piece)
    try:
        rc = lib.mrx_debug_kw_host_sub(ed.ctypes.data, eo.ctypes.data, len(entries), 1 if ignore_case else 0, rd.ctypes.data,
                                       ro.ctypes.data, len(ro) - 1, count, d.ctypes.data, o.ctypes.data, n,
                                       out_off.ctypes.data, out.ctypes.data + 3, cap, nsub.ctypes.data,
                                       C.cast(totals, C.c_void_p))
    finally:
        lib.mrx_debug_kw_piece(0)
    body = out[3:]   # (the output at an unaligned address: the first block is written byte by byte)
    assert (out[:3] == 0xEE).all() and (body[cap:] == 0xEE).all()                       # nothing at or beyond out_cap
    texts_out = None
    if rc == OK:
        assert (body[int(totals[0]):] == 0xEE).all()
        raw = body.tobytes()
        texts_out = [raw[out_off[i]:out_off[i + 1]] for i in range(n)]
    elif rc == E_CAP:
        assert (out == 0xEE).all()
    return rc, texts_out, nsub[:n], list(totals), out_off


def test_the_re_form_is_the_loop_of_the_definition():
    rng = np.random.default_rng(20261021)
    for rep in range(300):
        alphabet = b"ab" if rep % 2 else b"abc"
        entries, texts = SE.generated(rng, int(rng.integers(1, 12)), 6, alphabet, max_entry=8, max_text=30)
        ic = rep % 5 == 4
        if ic:
            entries = [e.upper() if k % 2 else e for k, e in enumerate(entries)]
            texts = [t.upper() if k % 3 == 0 else t for k, t in enumerate(texts)]
        for count in (0, 2):
            assert SE.leftmost(entries, texts, ic, count) == SE.leftmost_slow(entries, texts, ic, count), (entries, texts)
            assert SE.leftmost_dict(entries, texts, ic, count) == SE.leftmost_slow(entries, texts, ic, count)


def test_hand_cases_in_the_helper():
    assert SE.leftmost([b"a", b"aa", b"aaa", b"aaaa"], [b"aaaaaa"]) == [[(3, 0, 4), (1, 4, 6)]]
    assert SE.leftmost([b"ab", b"abcd", b"bc"], [b"abcabcd"]) == [[(0, 0, 2), (1, 3, 7)]]
    assert SE.leftmost([b"b", b"ab", b"b", b"ab"], [b"abb"]) == [[(1, 0, 2), (0, 2, 3)]]
    assert SE.sub([b"Ab"], b"<>", [b"xABab aB"], ignore_case=True) == ([b"x<><> <>"], [3])
    assert SE.sub([b"b"], [b"--"], [b"ABab"], ignore_case=True)[0] == [b"A--a--"]
    assert SE.sub([b"a", b"aa"], [b"1", b""], [b"aaa"], count=1)[0] == [b"a"]


HAND = [
    ([b"a", b"aa", b"aaa", b"aaaa"], [b"aaaaaa"], False, [[(3, 0, 4), (1, 4, 6)]]),
    ([b"ab", b"abcd", b"bc"], [b"abcabcd"], False, [[(0, 0, 2), (1, 3, 7)]]),     # longest at an equal start; bc is overlapped
    ([b"b", b"ab", b"b", b"ab"], [b"abb", b""], False, [[(1, 0, 2), (0, 2, 3)], []]),   # duplicates: the lowest index
    ([b"Ab", b"aB"], [b"xABab", b"", b"B"], True, [[(0, 1, 3), (0, 3, 5)], [], []]),
    ([], [b"abc", b""], False, [[], []]),                                          # m == 0
    ([b"abc"], [], False, []),                                                     # n == 0
]


@pytest.mark.parametrize("piece", [0, 1, 2, 16])
def test_hand_cases_on_the_host_lanes(piece):
    for entries, texts, ic, want in HAND:
        assert SE.leftmost(entries, texts, ic) == want
        rc, got, tot, prefix = _host_leftmost(entries, texts, ic, piece=piece)
        assert rc == OK and got == want and tot == sum(len(w) for w in want), (entries, M.load_library().mrx_last_error())
        assert prefix.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(int).tolist()
        for repl in (b"<>", b""):
            rc, outs, nsub, totals, _ = _host_sub(entries, repl, texts, ic, piece=piece)
            wo, wn = SE.sub(entries, repl, texts, ic)
            assert rc == OK and outs == wo and nsub.tolist() == wn.tolist()
            assert totals == [sum(map(len, wo)), max(map(len, wo), default=0), int(wn.sum())]
    # only the comparison folds: the copied bytes keep their case
    rc, outs, _, _, _ = _host_sub([b"b"], b"--", [b"ABab"], True, piece=piece)
    assert outs == [b"A--a--"]


@pytest.mark.parametrize("alphabet", [b"ab", b"abc"])
@pytest.mark.parametrize("piece", [16, 64, 0])
def test_generated_cases_on_the_host_lanes(piece, alphabet):
    rng = np.random.default_rng(20261020 + piece + len(alphabet))
    entries, texts = SE.generated(rng, 60, 200, alphabet)
    assert max(len(e) for e in entries) > 32        # at pieces of 16 the look-back spans several pieces
    m = len(entries)
    repls = [bytes(rng.integers(65, 91, size=int(k)).astype(np.uint8)) for k in rng.integers(0, 71, size=m)]
    repls[0], repls[1] = b"", b"R" * 70
    for count in (0, 1, 3):
        want = SE.leftmost(entries, texts, False, count)
        rc, got, tot, _ = _host_leftmost(entries, texts, count=count, piece=piece, skew=count + 4)
        assert rc == OK and tot == sum(len(w) for w in want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (count, i, texts[i])
        for repl in (b"<redact>", repls):
            wo, wn = SE.sub(entries, repl, texts, False, count)
            rc, outs, nsub, totals, _ = _host_sub(entries, repl, texts, count=count, piece=piece, skew=count + 9)
            assert rc == OK and nsub.tolist() == wn.tolist()
            for i, (g, w) in enumerate(zip(outs, wo)):
                assert g == w, (count, i, texts[i])
            assert totals == [sum(map(len, wo)), max(map(len, wo)), int(wn.sum())]
    # folded, mixed case on both sides
    ents = [e.upper() if k % 2 else e for k, e in enumerate(entries)]
    txts = [t.upper() if k % 3 == 0 else t for k, t in enumerate(texts)]
    rc, got, _, _ = _host_leftmost(ents, txts, True, piece=piece)
    assert got == SE.leftmost(ents, txts, True)
    rc, outs, _, _, _ = _host_sub(ents, repls, txts, True, piece=piece)
    assert outs == SE.sub(ents, repls, txts, True)[0]


def test_the_headless_text_and_the_text_with_a_head_in_every_piece():
    entries, text = [b"a", b"aa", b"aaa"], b"a" * 4099        # one chain across 257 pieces of 16
    want = SE.leftmost(entries, [text])
    assert len(want[0]) == 1367 and want[0][-1] == (0, 4098, 4099)
    rc, got, _, _ = _host_leftmost(entries, [text], piece=16)
    assert rc == OK and got == want
    rc, outs, nsub, _, _ = _host_sub(entries, [b"1", b"22", b"333"], [text, b"", text[:5]], piece=16)
    assert outs == [b"333" * 1366 + b"1", b"", b"33322"] and nsub.tolist() == [1367, 0, 2]
    text = b"ab " * 1400
    entries = [b"ab", b"b ", b"ab a"]
    for piece in (16, 0):
        rc, got, _, _ = _host_leftmost(entries, [text], piece=piece)
        assert rc == OK and got == SE.leftmost(entries, [text])
        rc, outs, _, _, _ = _host_sub(entries, [b"X", b"", b"long replacement " * 3], [text], piece=piece)
        assert outs == SE.sub(entries, [b"X", b"", b"long replacement " * 3], [text])[0]


def test_capacity_on_the_host_lanes():
    lib = M.load_library()
    entries, texts = [b"a", b"ab", b"ba"], [b"aabab", b"", b"bbab", b"xyz"]
    want = SE.leftmost(entries, texts)
    need = sum(len(w) for w in want)
    rc, got, tot, prefix = _host_leftmost(entries, texts, cap=need - 1)
    assert rc == E_CAP and tot == need and prefix.tolist() == [0, 3, 3, 4, 4]
    assert ("need %d" % need).encode() in lib.mrx_last_error()
    rc, got, tot, _ = _host_leftmost(entries, texts, cap=need)                      # the retry
    assert rc == OK and got == want
    wo, wn = SE.sub(entries, b"[gone]", texts)
    nbytes = sum(map(len, wo))
    rc, outs, nsub, totals, out_off = _host_sub(entries, b"[gone]", texts, cap=nbytes - 1)
    assert rc == E_CAP and totals == [nbytes, max(map(len, wo)), need] and nsub.tolist() == wn.tolist()
    assert out_off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in wo])]).astype(int).tolist()
    rc, outs, nsub, totals, _ = _host_sub(entries, b"[gone]", texts, cap=totals[0])  # the retry
    assert rc == OK and outs == wo


SYMBOLS = ("mrx_kw_leftmost_dev", "mrx_kw_leftmost_known_dev", "mrx_kw_leftmost_strided_dev", "mrx_kw_leftmost_batch",
           "mrx_kw_sub_dev", "mrx_kw_sub_known_dev", "mrx_kw_sub_strided_dev", "mrx_kw_sub_batch")
HOOKS = ("mrx_debug_kw_host_leftmost", "mrx_debug_kw_host_sub")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    for name in HOOKS:
        assert name in M.api.TESTING_SYMBOLS and getattr(lib, name) is not None
    assert callable(M.keywords_sub)
    for name in ("leftmost", "leftmost_lists", "sub", "subn"):
        assert callable(getattr(M.Keywords, name))


def test_argument_errors_come_before_any_device_call():
    lib = M.load_library()
    H = FAKE + 64   # a handle that is never dereferenced
    tot = C.c_int64(-7)
    t = C.byref(tot)
    calls = (lambda h, c, n, *o: lib.mrx_kw_leftmost_dev(h, c, FAKE, FAKE, n, *o, None),
             lambda h, c, n, *o: lib.mrx_kw_leftmost_known_dev(h, c, FAKE, FAKE, n, 100, 10, *o, None),
             lambda h, c, n, *o: lib.mrx_kw_leftmost_strided_dev(h, c, FAKE, 64, None, 64, n, *o, None))
    for call in calls:
        assert call(None, 0, 10, FAKE, FAKE, FAKE, 16, t) == E_ARG                   # null handle
        assert call(None, 0, 0, FAKE, FAKE, FAKE, 16, t) == E_ARG
        assert call(H, -1, 10, FAKE, FAKE, FAKE, 16, t) == E_ARG                     # negative count
        assert call(H, 0, -1, FAKE, FAKE, FAKE, 16, t) == E_ARG                      # negative n
        assert call(H, 0, 10, None, FAKE, FAKE, 16, t) == E_ARG                      # null d_text_prefix
        assert call(H, 0, 10, FAKE, None, FAKE, 16, t) == E_ARG
        assert call(H, 0, 10, FAKE, FAKE, None, 16, t) == E_ARG
        assert call(H, 0, 10, FAKE, FAKE, FAKE, -1, t) == E_ARG                      # negative span_cap
        assert call(H, 0, 10, FAKE, FAKE, FAKE + 4, 16, t) == E_ARG                  # d_spans not 8-byte aligned
    assert lib.mrx_kw_leftmost_dev(H, 0, FAKE, None, 10, FAKE, FAKE, FAKE, 16, t, None) == E_ARG
    assert lib.mrx_kw_leftmost_known_dev(H, 0, FAKE, FAKE, 10, -1, 10, FAKE, FAKE, FAKE, 16, t, None) == E_ARG
    assert lib.mrx_kw_leftmost_known_dev(H, 0, FAKE, FAKE, 10, 100, -1, FAKE, FAKE, FAKE, 16, t, None) == E_ARG
    assert lib.mrx_kw_leftmost_strided_dev(H, 0, FAKE, 64, None, 65, 10, FAKE, FAKE, FAKE, 16, t, None) == E_ARG
    assert tot.value == -7
    totals = (C.c_int64 * 3)(-7, -7, -7)
    tp = C.cast(totals, C.c_void_p)
    subs = (lambda h, rd, ro, r, c, n, *o: lib.mrx_kw_sub_dev(h, rd, ro, r, c, FAKE, FAKE, n, *o, None),
            lambda h, rd, ro, r, c, n, *o: lib.mrx_kw_sub_known_dev(h, rd, ro, r, c, FAKE, FAKE, n, 100, 10, *o, None),
            lambda h, rd, ro, r, c, n, *o: lib.mrx_kw_sub_strided_dev(h, rd, ro, r, c, FAKE, 64, None, 64, n, *o, None))
    good = (FAKE, FAKE, 16, FAKE, FAKE, tp)
    for call in subs:
        assert call(None, FAKE, FAKE, 1, 0, 10, *good) == E_ARG                      # null handle
        assert call(None, FAKE, FAKE, 1, 0, 0, *good) == E_ARG
        assert call(H, FAKE, FAKE, -1, 0, 10, *good) == E_ARG                        # negative r
        assert call(H, FAKE, FAKE, 1, -1, 10, *good) == E_ARG                        # negative count
        assert call(H, None, FAKE, 1, 0, 10, *good) == E_ARG                         # null replacements with r > 0
        assert call(H, FAKE, None, 1, 0, 10, *good) == E_ARG
        assert call(H, FAKE, FAKE, 1, 0, -1, *good) == E_ARG                         # negative n
        assert call(H, FAKE, FAKE, 1, 0, 10, None, FAKE, 16, FAKE, FAKE, tp) == E_ARG    # null d_out_offsets
        assert call(H, FAKE, FAKE, 1, 0, 10, FAKE, None, 16, FAKE, FAKE, tp) == E_ARG    # null d_out_data with a capacity
        assert call(H, FAKE, FAKE, 1, 0, 10, FAKE, FAKE, -1, FAKE, FAKE, tp) == E_ARG    # negative out_cap
    assert lib.mrx_kw_sub_dev(H, FAKE, FAKE, 1, 0, FAKE, None, 10, *good, None) == E_ARG
    assert lib.mrx_kw_sub_known_dev(H, FAKE, FAKE, 1, 0, FAKE, FAKE, 10, -1, 10, *good, None) == E_ARG
    assert lib.mrx_kw_sub_known_dev(H, FAKE, FAKE, 1, 0, FAKE, FAKE, 10, 100, -1, *good, None) == E_ARG
    assert lib.mrx_kw_sub_strided_dev(H, FAKE, FAKE, 1, 0, FAKE, 0, None, 0, 10, *good, None) == E_ARG
    assert list(totals) == [-7, -7, -7]
    data, off = M.pack_texts([b"ab", b"c"])
    pre = np.zeros(3, np.int64)
    assert lib.mrx_kw_leftmost_batch(None, 0, data.ctypes.data, off.ctypes.data, 2, pre.ctypes.data, FAKE, FAKE, 16, t) == E_ARG
    assert lib.mrx_kw_leftmost_batch(H, -1, data.ctypes.data, off.ctypes.data, 2, pre.ctypes.data, FAKE, FAKE, 16, t) == E_ARG
    assert lib.mrx_kw_leftmost_batch(H, 0, data.ctypes.data, None, 2, pre.ctypes.data, FAKE, FAKE, 16, t) == E_ARG
    assert lib.mrx_kw_sub_batch(None, FAKE, FAKE, 1, 0, data.ctypes.data, off.ctypes.data, 2, pre.ctypes.data, FAKE, 16, None,
                                None) == E_ARG
    assert lib.mrx_kw_sub_batch(H, FAKE, FAKE, -1, 0, data.ctypes.data, off.ctypes.data, 2, pre.ctypes.data, FAKE, 16, None,
                                None) == E_ARG
    assert lib.mrx_kw_sub_batch(H, None, FAKE, 1, 0, data.ctypes.data, off.ctypes.data, 2, pre.ctypes.data, FAKE, 16, None,
                                None) == E_ARG
    # r is 1 or m: through the hook, which needs no handle
    ed, eo = M.pack_texts([b"a", b"b", b"c"])
    rd, ro = M.pack_texts([b"x", b"y"])
    out_off, out = np.zeros(3, np.int64), np.zeros(64, np.uint8)
    for r in (0, 2):
        assert lib.mrx_debug_kw_host_sub(ed.ctypes.data, eo.ctypes.data, 3, 0, rd.ctypes.data, ro.ctypes.data, r, 0,
                                         data.ctypes.data, off.ctypes.data, 2, out_off.ctypes.data, out.ctypes.data, 64, None,
                                         None) == E_ARG
        assert b"r must be 1 or the number of entries, 3" in lib.mrx_last_error()
    assert lib.mrx_debug_kw_host_sub(ed.ctypes.data, eo.ctypes.data, 3, 0, rd.ctypes.data, ro.ctypes.data, 1, -1,
                                     data.ctypes.data, off.ctypes.data, 2, out_off.ctypes.data, out.ctypes.data, 64, None,
                                     None) == E_ARG
