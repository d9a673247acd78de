"""Keywords without a GPU: the expectation helper (tests/keywords_expect.py) on hand-traced cases, the automaton and the
walk of the kernels on the CPU (mrx_debug_kw_host_findall: the same build, the same pieces, the same walk) against the
helper on generated cases, the C ABI's symbols and its argument errors, all of which return before any device call."""
import numpy as np
import pytest

import mojo_regex_amd as M
import keywords_expect as KE

FAKE = 1 << 40   # a device pointer that is never dereferenced
C = M.api.C


def test_every_occurrence_counts_and_the_longest_comes_first_at_an_end():
    hits = KE.findall([b"a", b"aa", b"aaa", b"aaaa"], [b"aaaaaa"])[0]
    assert len(hits) == 18            # 6 + 5 + 4 + 3
    assert hits[:6] == [(0, 0, 1), (1, 0, 2), (0, 1, 2), (2, 0, 3), (1, 1, 3), (0, 2, 3)]
    assert hits[-4:] == [(3, 2, 6), (2, 3, 6), (1, 4, 6), (0, 5, 6)]
    assert [h[2] for h in hits] == sorted(h[2] for h in hits)
    for a, b in zip(hits, hits[1:]):
        assert (a[2], a[1]) < (b[2], b[1])


def test_nested_entries():
    assert KE.findall([b"he", b"she", b"his", b"hers"], [b"ushers", b"his", b"", b"sh"]) == \
        [[(1, 1, 4), (0, 2, 4), (3, 2, 6)], [(2, 0, 3)], [], []]


def test_duplicates_and_folding_in_the_helper():
    assert KE.findall([b"ab", b"b", b"ab", b"b"], [b"abab"]) == [[(0, 0, 2), (1, 1, 2), (0, 2, 4), (1, 3, 4)]]
    assert KE.findall([b"Ab", b"aB"], [b"xABab"], ignore_case=True) == [[(0, 1, 3), (0, 3, 5)]]
    assert KE.findall([b"Ab", b"aB"], [b"xABab"]) == [[]]
    assert KE.findall([b"\xc4b"], [b"\xe4b\xc4B"], ignore_case=True) == [[(0, 2, 4)]]   # only ASCII is folded
    hits = KE.findall([b"a"], [b"xa", b"x", b"a"])
    assert [a.tolist() for a in KE.filtered(hits, [b"xa", b"x", b"a"])[:2]] == [[0, 2], [0, 2, 3]]
    assert KE.filtered(hits, [b"xa", b"x", b"a"], invert=True)[2] == b"x"


def _host(entries, texts, ignore_case=False, piece=0, cap=None, skew=0):
    """mrx_debug_kw_host_findall -> (rc, lists per text, total, describe)."""
    lib = M.load_library()
    ed, eo = M.pack_texts(entries)
    d, o = M.pack_texts(texts)
    if skew:   # the texts at another alignment
        d = np.concatenate([np.full(skew, ord("a"), np.uint8), d])
        o = o + skew
    n = len(texts)
    if cap is None:
        cap = sum(len(h) for h in KE.findall(entries, texts, ignore_case)) + 3
    prefix = np.full(n + 1, -1, np.int64)
    ents = np.full(cap + 2, -9, np.int32)
    spans = np.full((cap + 2, 2), -9, np.int32)
    tot = C.c_int64(-1)
    desc = C.create_string_buffer(256)
    lib.mrx_debug_kw_piece(piece)
    try:
        rc = lib.mrx_debug_kw_host_findall(ed.ctypes.data, eo.ctypes.data, len(entries), 1 if ignore_case else 0,
                                           d.ctypes.data, o.ctypes.data, n, prefix.ctypes.data, ents.ctypes.data,
                                           spans.ctypes.data, cap, C.byref(tot), desc, 256)
    finally:
        lib.mrx_debug_kw_piece(0)
    assert ents[cap:].tolist() == [-9, -9] and spans[cap:].tolist() == [[-9, -9]] * 2   # nothing behind the capacity
    lists = None
    if rc == M.api.MRX_OK:
        lists = [[(int(ents[q]), int(spans[q, 0]), int(spans[q, 1])) for q in range(prefix[i], prefix[i + 1])]
                 for i in range(n)]
    return rc, lists, int(tot.value), desc.value.decode(), prefix


def test_hand_cases_on_the_host_walk():
    for piece in (0, 1, 2, 16):
        rc, got, tot, _, _ = _host([b"a", b"aa", b"aaa", b"aaaa"], [b"aaaaaa"], piece=piece)
        assert rc == 0 and tot == 18 and got == KE.findall([b"a", b"aa", b"aaa", b"aaaa"], [b"aaaaaa"]), piece
        rc, got, tot, _, _ = _host([b"he", b"she", b"his", b"hers"], [b"ushers", b"", b"hishe"], piece=piece)
        assert rc == 0 and got == KE.findall([b"he", b"she", b"his", b"hers"], [b"ushers", b"", b"hishe"]), piece


@pytest.mark.parametrize("piece", [16, 32, 0])
def test_generated_cases_on_the_host_walk(piece):
    rng = np.random.default_rng(20261020 + piece)
    cases = 0
    for rep in range(60):
        m = int(rng.integers(1, 25))
        entries, texts = KE.generated(rng, m, 60)
        ic = rep % 5 == 4
        if ic:   # mixed case on both sides
            entries = [e.upper() if k % 2 else e for k, e in enumerate(entries)]
            texts = [t.upper() if k % 3 == 0 else t for k, t in enumerate(texts)]
        rc, got, tot, _, _ = _host(entries, texts, ignore_case=ic, piece=piece, skew=rep % 16)
        want = KE.findall(entries, texts, ic)
        assert rc == 0 and tot == sum(len(w) for w in want), (rep, M.load_library().mrx_last_error())
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (rep, i, entries, texts[i])
        cases += len(texts)
    assert cases >= 3000


def test_describe_duplicates_and_folding():
    rc, got, tot, desc, _ = _host([b"he", b"she", b"his", b"hers", b"he"], [b"ushers"])
    assert desc == "keywords: m=5 distinct=4 states=10 classes=6 lmax=4 table_bytes=240 ignore_case=0"
    assert got == [[(1, 1, 4), (0, 2, 4), (3, 2, 6)]]
    rc, got, tot, desc, _ = _host([b"x", b"He", b"she", b"HE", b"hE"], [b"usHErs", b"X"], ignore_case=True)
    assert desc == "keywords: m=5 distinct=3 states=7 classes=5 lmax=3 table_bytes=140 ignore_case=1"
    assert got == [[(2, 1, 4), (1, 2, 4)], [(0, 0, 1)]]
    rc, got, tot, desc, _ = _host([b"He"], [b"he", b"He"])          # without the flag nothing is folded
    assert got == [[], [(0, 0, 2)]]
    # every byte that occurs in no entry shares one class: 2 states (root, "q"), the class of q and the class of the rest
    rc, got, tot, desc, _ = _host([b"q"], [bytes(range(256))])
    assert desc == "keywords: m=1 distinct=1 states=2 classes=2 lmax=1 table_bytes=16 ignore_case=0"
    assert got == [[(0, ord("q"), ord("q") + 1)]]
    rc, got, tot, desc, _ = _host([b"q"], [bytes(range(256))], ignore_case=True)
    assert got == [[(0, ord("Q"), ord("Q") + 1), (0, ord("q"), ord("q") + 1)]]


def test_no_entries_and_no_texts():
    rc, got, tot, desc, prefix = _host([], [b"abc", b""])
    assert rc == 0 and got == [[], []] and tot == 0 and prefix.tolist() == [0, 0, 0]
    assert desc == "keywords: m=0 distinct=0 states=1 classes=1 lmax=0 table_bytes=4 ignore_case=0"
    rc, got, tot, desc, prefix = _host([b"a"], [])
    assert rc == 0 and got == [] and tot == 0 and prefix.tolist() == [0]


def test_capacity_on_the_host_walk():
    entries, texts = [b"a", b"aa"], [b"aaa", b"", b"aa"]
    rc, got, tot, _, prefix = _host(entries, texts, cap=4)
    assert rc == M.api.MRX_E_CAPACITY and tot == 8 and prefix.tolist() == [0, 5, 5, 8]
    assert b"need 8" in M.load_library().mrx_last_error()
    rc, got, tot, _, _ = _host(entries, texts, cap=8)
    assert rc == 0 and got == KE.findall(entries, texts)


def test_the_piece_rule():
    # 8 x (Lmax - 1) rounded up to 16 and 1024 at least, halved towards 2 x (Lmax - 1) (64 at least) for small batches:
    # seen through results that do not change, and through the default of the generated cases above; here the entries
    # are longer than the smallest piece, so a hit spans several pieces at every size
    entries = [b"ab" * 100, b"b" + b"ab" * 70, b"ba"]
    texts = [b"ab" * 400, b"a" + b"ab" * 150 + b"b", b"ab" * 99]
    want = KE.findall(entries, texts)
    for piece in (0, 16, 48, 200, 4096):
        rc, got, tot, _, _ = _host(entries, texts, piece=piece)
        assert rc == 0 and got == want, piece


SYMBOLS = ("mrx_kw_build", "mrx_kw_build_dev", "mrx_kw_free", "mrx_kw_size", "mrx_kw_distinct", "mrx_kw_describe",
           "mrx_kw_contains_dev", "mrx_kw_contains_strided_dev", "mrx_kw_count_dev", "mrx_kw_count_strided_dev",
           "mrx_kw_findall_dev", "mrx_kw_findall_known_dev", "mrx_kw_findall_strided_dev", "mrx_kw_filter_dev",
           "mrx_kw_filter_known_dev", "mrx_kw_filter_strided_dev", "mrx_kw_findall_batch")
HOOKS = ("mrx_debug_kw_piece", "mrx_debug_kw_tier", "mrx_debug_kw_host_findall")


def test_symbols_are_exported():
    lib = M.load_library()
    for name in SYMBOLS:
        assert name in M.api.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    for name in HOOKS:
        assert name in M.api.TESTING_SYMBOLS
        assert getattr(lib, name) is not None
    assert callable(M.build_keywords) and callable(M.keywords_filter)
    for name in ("contains", "count", "findall", "findall_lists", "filter", "filter_async", "describe", "__len__", "__del__"):
        assert callable(getattr(M.Keywords, name))
    assert isinstance(M.Keywords.distinct_count, property)
    assert M.api.MRX_KW_IGNORE_CASE == 1
    lib.mrx_kw_free(None)   # a no-op
    assert lib.mrx_kw_size(None) == 0 and lib.mrx_kw_distinct(None) == 0


def test_build_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    out = C.c_void_p(0x5A5A)
    ref = C.byref(out)
    data, off = M.pack_texts([b"ab", b"", b"c"])
    for build in (lib.mrx_kw_build, lib.mrx_kw_build_dev):
        assert build(FAKE, FAKE, -1, 0, None, ref) == A                            # negative m
        assert build(FAKE, None, 3, 0, None, ref) == A                             # null offsets
        assert build(FAKE, FAKE, 3, 0, None, None) == A                            # null out
        assert build(FAKE, FAKE, 3, 2, None, ref) == A                             # a flag bit that does not exist
        assert build(FAKE, FAKE, 3, 1 | 4, None, ref) == A
        assert build(FAKE, FAKE, 1 << 31, 0, None, ref) == A                       # refused before the offsets are read
        assert b"2^31" in lib.mrx_last_error()
        assert build(FAKE, FAKE, (1 << 31) + 5, 1, None, ref) == A
    assert lib.mrx_kw_build(data.ctypes.data, off.ctypes.data, 3, 0, None, ref) == A   # an empty entry
    assert b"entry 1 is empty" in lib.mrx_last_error()
    assert lib.mrx_kw_build(None, off.ctypes.data, 3, 0, None, ref) == A           # null data of entries with bytes
    bad = np.array([4, 2, 5], np.int64)
    assert lib.mrx_kw_build(data.ctypes.data, bad.ctypes.data, 2, 0, None, ref) == A   # offsets that decrease
    assert out.value == 0x5A5A                                                     # no handle came back
    # the hook refuses the same entries
    pre = np.zeros(2, np.int64)
    assert lib.mrx_debug_kw_host_findall(data.ctypes.data, off.ctypes.data, 3, 0, data.ctypes.data, off.ctypes.data, 1,
                                         pre.ctypes.data, None, None, 0, None, None, 0) == A
    assert b"entry 1 is empty" in lib.mrx_last_error()
    assert lib.mrx_debug_kw_host_findall(data.ctypes.data, off.ctypes.data, 1, 8, data.ctypes.data, off.ctypes.data, 1,
                                         pre.ctypes.data, None, None, 0, None, None, 0) == A


def test_a_table_above_the_limit_is_refused_with_its_size():
    # 11 000 entries of 4 200 bytes that differ in their first bytes: 4.6e7 states x 6 classes x 4 bytes is above 1 GiB,
    # and the count of the states comes before anything of that size is allocated
    lib = M.load_library()
    m, L = 11000, 4200
    rows = np.full((m, L), ord("a"), np.uint8)
    digits = np.frombuffer(b"bcde", np.uint8)
    for k in range(7):
        rows[:, k] = digits[(np.arange(m) >> (2 * k)) & 3]
    off = np.arange(m + 1, dtype=np.int64) * L
    out = C.c_void_p(0x5A5A)
    assert lib.mrx_kw_build(rows.ctypes.data, off.ctypes.data, m, 0, None, C.byref(out)) == M.api.MRX_E_UNSUPPORTED
    msg = lib.mrx_last_error()
    assert b"classes" in msg and b"states" in msg and b"above 1 GiB" in msg, msg
    assert b" x 6 classes" in msg
    assert out.value == 0x5A5A


def test_per_text_and_findall_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    H = FAKE + 64   # a handle that is never dereferenced
    for stem in ("mrx_kw_contains", "mrx_kw_count"):
        csr, strided = getattr(lib, stem + "_dev"), getattr(lib, stem + "_strided_dev")
        assert csr(None, FAKE, FAKE, 10, FAKE, None) == A                          # null handle
        assert csr(None, FAKE, FAKE, 0, FAKE, None) == A                           # ... for no text too
        assert csr(H, FAKE, FAKE, -1, FAKE, None) == A                             # negative n
        assert csr(H, FAKE, None, 10, FAKE, None) == A                             # null d_offsets
        assert csr(H, FAKE, FAKE, 10, None, None) == A                             # null output
        assert strided(None, FAKE, 64, None, 64, 10, FAKE, None) == A
        assert strided(H, FAKE, 64, None, 64, -1, FAKE, None) == A
        assert strided(H, FAKE, 64, None, 64, 10, None, None) == A
        assert strided(H, FAKE, 64, None, 65, 10, FAKE, None) == A                 # a length beyond the pitch
        assert strided(H, FAKE, 0, None, 0, 10, FAKE, None) == A                   # a non-positive pitch
    tot = C.c_int64(-7)
    t = C.byref(tot)
    fa, fk, fs = lib.mrx_kw_findall_dev, lib.mrx_kw_findall_known_dev, lib.mrx_kw_findall_strided_dev
    assert fa(None, FAKE, FAKE, 10, FAKE, FAKE, FAKE, 16, t, None) == A
    assert fa(H, FAKE, FAKE, -1, FAKE, FAKE, FAKE, 16, t, None) == A
    assert fa(H, FAKE, None, 10, FAKE, FAKE, FAKE, 16, t, None) == A
    assert fa(H, FAKE, FAKE, 10, None, FAKE, FAKE, 16, t, None) == A               # null d_text_prefix
    assert fa(H, FAKE, FAKE, 0, None, FAKE, FAKE, 16, t, None) == A                # ... for no text too
    assert fa(H, FAKE, FAKE, 10, FAKE, None, FAKE, 16, t, None) == A               # null d_entries
    assert fa(H, FAKE, FAKE, 10, FAKE, FAKE, None, 16, t, None) == A               # null d_spans
    assert fa(H, FAKE, FAKE, 10, FAKE, FAKE, FAKE, -1, t, None) == A               # negative span_cap
    assert fa(H, FAKE, FAKE, 10, FAKE, FAKE, FAKE + 4, 16, t, None) == A           # d_spans not 8-byte aligned
    assert fk(H, FAKE, FAKE, 10, -1, 10, FAKE, FAKE, FAKE, 16, t, None) == A       # negative known bounds
    assert fk(H, FAKE, FAKE, 10, 100, -1, FAKE, FAKE, FAKE, 16, t, None) == A
    assert fk(H, FAKE, FAKE, 10, 100, 10, FAKE, FAKE, None, 16, t, None) == A
    assert fs(H, FAKE, 64, None, 64, -1, FAKE, FAKE, FAKE, 16, t, None) == A
    assert fs(H, FAKE, 64, None, 65, 10, FAKE, FAKE, FAKE, 16, t, None) == A
    assert fs(H, FAKE, 64, None, 64, 10, None, None, None, 16, None, None) == A
    assert tot.value == -7
    data, off = M.pack_texts([b"ab", b"c"])
    pre = np.zeros(3, np.int64)
    fb = lib.mrx_kw_findall_batch
    assert fb(None, data.ctypes.data, off.ctypes.data, 2, pre.ctypes.data, FAKE, FAKE, 16, t) == A
    assert fb(H, data.ctypes.data, None, 2, pre.ctypes.data, FAKE, FAKE, 16, t) == A
    assert fb(H, data.ctypes.data, off.ctypes.data, -1, pre.ctypes.data, FAKE, FAKE, 16, t) == A
    assert fb(H, data.ctypes.data, off.ctypes.data, 2, None, FAKE, FAKE, 16, t) == A
    assert fb(H, data.ctypes.data, off.ctypes.data, 2, pre.ctypes.data, None, FAKE, 16, t) == A
    assert fb(H, data.ctypes.data, off.ctypes.data, 2, pre.ctypes.data, FAKE, FAKE, -1, t) == A
    assert fb(H, None, off.ctypes.data, 2, pre.ctypes.data, FAKE, FAKE, 16, t) == A
    bad = np.array([4, 2, 0], np.int64)
    assert fb(H, data.ctypes.data, bad.ctypes.data, 2, pre.ctypes.data, FAKE, FAKE, 16, t) == A


def test_filter_argument_errors():
    lib = M.load_library()
    A = M.api.MRX_E_ARGUMENT
    H = FAKE + 64
    tot = (C.c_int64 * 2)(-7, -7)
    tp = C.cast(tot, C.c_void_p)
    calls = (lambda h, f, n, *t: lib.mrx_kw_filter_dev(h, f, FAKE, FAKE, n, *t, None),
             lambda h, f, n, *t: lib.mrx_kw_filter_known_dev(h, f, FAKE, FAKE, n, 100, 10, *t, None),
             lambda h, f, n, *t: lib.mrx_kw_filter_strided_dev(h, f, FAKE, 64, None, 64, n, *t, None))
    good = (FAKE, FAKE, FAKE, 16, FAKE, tp)
    for call in calls:
        assert call(None, 0, 10, *good) == A                                       # null handle
        assert call(None, 0, 0, *good) == A
        assert call(H, 4, 10, *good) == A                                          # unknown flag bits
        assert call(H, 1 | 8, 10, *good) == A
        assert call(H, 0, -1, *good) == A                                          # negative n
        assert call(H, 0, 10, FAKE, FAKE, FAKE, -1, FAKE, tp) == A                 # negative out_cap
        assert call(H, 0, 10, None, FAKE, FAKE, 16, FAKE, tp) == A                 # null d_kept_idx
        assert call(H, 0, 10, FAKE, None, FAKE, 16, FAKE, tp) == A                 # null d_out_offsets
        assert call(H, 0, 10, FAKE, FAKE, None, 16, FAKE, tp) == A                 # null d_out_data with a capacity
        assert call(H, 0, 10, FAKE, FAKE, FAKE, 16, None, tp) == A                 # null d_totals
        assert call(H, 0, 0, FAKE, None, FAKE, 16, FAKE, tp) == A                  # ... for no text too
    assert lib.mrx_kw_filter_dev(H, 0, FAKE, None, 10, *good, None) == A           # null d_offsets
    assert lib.mrx_kw_filter_known_dev(H, 0, FAKE, FAKE, 10, -1, 10, *good, None) == A
    assert lib.mrx_kw_filter_known_dev(H, 0, FAKE, FAKE, 10, 100, -1, *good, None) == A
    assert lib.mrx_kw_filter_strided_dev(H, 0, FAKE, 64, None, 65, 10, *good, None) == A
    assert lib.mrx_kw_filter_strided_dev(H, 0, FAKE, 0, None, 0, 10, *good, None) == A
    assert list(tot) == [-7, -7]
