"""PatternSet.sub on the GPU: output bytes, offsets and replacement counts equal the oracle's restatement
(tests/set_sub_expect.py) bit for bit, on CSR, known-bounds CSR, fixed-pitch and ragged batches and every poisoned layout
of tests/layouts.py; replacements of every size; count; texts longer than the select window; a one-member set against
CompiledRegex.sub where the two contracts agree; and the contract's edges: 256 members, empty batches, capacity, two
streams, scratch that does not grow with the set."""
import numpy as np
import pytest

import layouts as LY
import mojo_regex_amd as M
import set_sub_expect as E
from mrx_ref import hybrid as O
from test_gpu_pattern_set import CONFIG_PATTERNS, SETS, _batches, _texts

pytestmark = pytest.mark.gpu

_CACHE = {}   # oracle findall per (pattern, text)
BIG = bytes(range(256)) * 40   # 10 KB: does not fit the kernel's LDS table


def _repls(k, seed=0):
    """different lengths per member: empty, 1 byte, 64 bytes, a few bytes, and one 10 KB replacement"""
    kinds = [b"", b"#", bytes(range(64)), b"<%d>", b"[r%d]"]
    out = []
    for j in range(k):
        r = kinds[(j + seed) % len(kinds)]
        out.append(r % j if b"%d" in r else r)
    return out


def _host(res):
    return tuple(np.ascontiguousarray(x.cpu().numpy()) for x in res)


def _assert_same(got, want, what, texts=None):
    go, gd, gn = got
    wo, wd, wn = want
    if np.array_equal(go, wo) and np.array_equal(gd, wd) and np.array_equal(gn, wn):
        return
    for i in range(len(wo) - 1):
        g, w = gd[go[i]:go[i + 1]].tobytes(), wd[wo[i]:wo[i + 1]].tobytes()
        if g != w or gn[i] != wn[i]:
            raise AssertionError("%s: text %d %r\n  device %r (%d)\n  want   %r (%d)" % (
                what, i, (texts[i][:100] if texts else None), g[:160], gn[i], w[:160], wn[i]))
    raise AssertionError("%s: same per text, different arrays" % what)


@pytest.fixture(scope="module")
def batches():
    import torch
    texts = _texts(5, 1200)
    out = _batches(texts)
    out["csr_known"] = (M.DeviceBatch.from_texts(texts), texts)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("setname", list(SETS))
def test_set_sub_equals_oracle(batches, setname):
    pats = SETS[setname]
    s = M.compile_set(pats)
    reps = _repls(len(pats))
    for form, (batch, texts) in batches.items():
        for count in ((0, 1, 3) if form == "csr" else (0,)):
            got = _host(s.subn(reps, batch, count=count))
            assert got[1].dtype == np.uint8 and got[2].dtype == np.int32
            _assert_same(got, E.expected_arrays(pats, reps, texts, count, _CACHE),
                         "%s on %s count=%d" % (setname, form, count), texts)
    # host lists, one replacement for every member
    texts = batches["csr"][1][:200]
    outs, nsub = s.subn(b"__", texts)
    want = E.expected_lists(pats, [b"__"] * len(pats), texts, 0, _CACHE)
    assert outs == want[0] and nsub.tolist() == want[1]
    assert s.sub("__", texts) == want[0]


def test_replacement_sizes_and_the_big_replacement(batches):
    pats = SETS["mixed7"]
    s = M.compile_set(pats)
    batch, texts = batches["csr_known"]
    for reps in ([b""] * 7, [b"x"] * 7, [bytes(range(64))] * 7, [BIG] + _repls(6, 2), _repls(6, 1) + [BIG]):
        got = _host(s.subn(reps, batch))
        _assert_same(got, E.expected_arrays(pats, reps, texts, 0, _CACHE), "repl lens %s" % [len(r) for r in reps],
                     texts)


def _layout_set_patterns():
    pats = list(LY.PATTERNS)
    while True:
        ps = M.compile_set(pats)
        try:
            ps.sub(b"", M.DeviceBatch.from_texts([b"ab"]))
            return pats, ps
        except M.UnsupportedPattern as exc:
            pats.pop(int(str(exc).split("member ")[1].split(":")[0]))


def test_set_sub_on_every_layout():
    pats, ps = _layout_set_patterns()
    assert len(pats) >= 15, pats
    k = len(pats)
    reps = _repls(k, 3)
    texts, origin = [], []
    for j, p in enumerate(pats):
        ts = LY.make_texts(p, 12, 1 if j % 8 == 0 else 0, seed=11)
        texts += ts
        origin += [j] * len(ts)
    rngs = [np.random.default_rng(j) for j in range(k)]
    pz = lambda i, t, size: LY.poison(pats[origin[i] if 0 <= i < len(origin) else 0], t, size,  # noqa: E731
                                      rngs[origin[i] if 0 <= i < len(origin) else 0])
    for lay in LY.layouts_for(texts, pz, texts[:160]):
        got = _host(ps.subn(reps, lay.device()))
        _assert_same(got, E.expected_arrays(pats, reps, lay.texts, 0, _CACHE), "layout %s" % lay.name, lay.texts)


def test_texts_longer_than_the_select_window():
    import random
    r = random.Random(3)
    pats = [b"\\d+", b"[a-z]+\\d", b"z*", b"aa", b"[a-c]"]
    reps = [b"<D>", b"", b"-", b"AAAA", bytes(range(64))]
    texts = [bytes(r.choice(b"abcz0123 aa") for _ in range(100_000)) for _ in range(3)]
    texts += [b"a" * 5000, b"", b"q" * 3071, b"0" * 1537]
    s = M.compile_set(pats)
    for count in (0, 3):
        got = _host(s.subn(reps, M.DeviceBatch.from_texts(texts), count=count))
        _assert_same(got, E.expected_arrays(pats, reps, texts, count, _CACHE), "long texts count=%d" % count)


def test_one_member_set_equals_compiled_regex_sub(batches):
    batch, texts = batches["csr_known"]
    for p in CONFIG_PATTERNS:
        want = E.expected_lists([p], [b"<R>"], texts, 0, _CACHE)[0]
        agree = [i for i, t in enumerate(texts) if O.sub(p, b"<R>", t) == want[i]]
        assert len(agree) > len(texts) // 2, p   # a test-data error shows here
        so, sd = M.CompiledRegex(p).sub_dev(b"<R>", batch)
        go, gd = M.compile_set([p]).sub(b"<R>", batch)
        so, sd, go, gd = so.cpu().numpy(), sd.cpu().numpy(), go.cpu().numpy(), gd.cpu().numpy()
        for i in agree:
            assert gd[go[i]:go[i + 1]].tobytes() == sd[so[i]:so[i + 1]].tobytes() == want[i], (p, i)


def test_256_members_empty_batches_and_all_empty_texts():
    import torch
    pats = [b"a%d" % i for i in range(200)] + SETS["gen64"][:56]
    reps = _repls(256)
    texts = [b"a1 a12 a199 xyz", b"", b"a0a1a2a3", b"hello 123 foo@bar.com a55"] * 8
    s = M.compile_set(pats)
    assert len(s) == 256
    got = _host(s.subn(reps, M.DeviceBatch.from_texts(texts)))
    _assert_same(got, E.expected_arrays(pats, reps, texts, 0, _CACHE), "256 members", texts)
    m = M.compile_set(SETS["mixed7"])
    e = M.DeviceBatch(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    o, d, n = m.subn(b"x", e)
    assert o.cpu().tolist() == [0] and d.numel() == 0 and n.numel() == 0
    assert m.sub(b"x", []) == []
    empties = [b""] * 100
    for batch in (M.DeviceBatch.from_texts(empties), M.DeviceBatch.strided(torch.zeros(1600, dtype=torch.uint8,
                                                                                      device="cuda"), 16, length=0)):
        got = _host(m.subn(_repls(7), batch))
        _assert_same(got, E.expected_arrays(SETS["mixed7"], _repls(7), empties, 0, _CACHE), "empty texts")


def test_capacity_and_retry():
    import torch
    lib = M.load_library()
    pats = SETS["mixed7"]
    reps = _repls(7)
    s = M.compile_set(pats)
    texts = _texts(8, 300)
    batch = M.DeviceBatch.from_texts(texts)
    want = E.expected_arrays(pats, reps, texts, 0, _CACHE)
    total = int(want[0][-1])
    arr = (M.api.C.c_char_p * 7)(*reps)
    lens = (M.api.C.c_size_t * 7)(*[len(r) for r in reps])
    ptr = M.api._ptr
    for cap in (total - 1, total):
        out_off = torch.full((batch.n + 1,), -3, dtype=torch.int64, device="cuda")
        out = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        nsub = torch.full((batch.n,), -3, dtype=torch.int32, device="cuda")
        tot = M.api.C.c_int64(0)
        rc = lib.mrx_set_sub_dev(s._h, arr, lens, 0, ptr(batch.data), ptr(batch.offsets), batch.n, ptr(out_off),
                                 ptr(out), cap, ptr(nsub), M.api.C.byref(tot), None)
        torch.cuda.synchronize()
        assert tot.value == total
        assert np.array_equal(out_off.cpu().numpy(), want[0]) and np.array_equal(nsub.cpu().numpy(), want[2])
        assert bool((out[cap:] == 0xAB).all())   # nothing at or beyond the cap
        if cap < total:
            assert rc == M.api.MRX_E_CAPACITY, rc
            assert bool((out == 0xAB).all())
        else:
            assert rc == M.api.MRX_OK, rc
            assert np.array_equal(out[:total].cpu().numpy(), want[1])
    with pytest.raises(M.MrxError):
        s.sub(reps, batch, out_cap=total - 1)
    # the default capacity too small: one retry
    dense = [b"a*", b"[a-z]", b"\\w*"]
    big = [BIG[:3000]] * 3
    texts = [b"abcdefgh" * 40] * 20
    got = _host(M.compile_set(dense).subn(big, M.DeviceBatch.from_texts(texts)))
    _assert_same(got, E.expected_arrays(dense, big, texts, 0, _CACHE), "retry")
    assert M.compile_set(dense).sub(big, texts[:3]) == E.expected_lists(dense, big, texts[:3], 0, _CACHE)[0]


def test_two_sets_on_two_streams(batches):
    import torch
    s1, s2 = M.compile_set(SETS["gen64"]), M.compile_set(SETS["mixed7"])
    r1, r2 = _repls(64), _repls(7, 1)
    batch, _ = batches["csr_known"]
    want1, want2 = _host(s1.subn(r1, batch)), _host(s2.subn(r2, batch))
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        g1 = s1.subn(r1, batch)
    with torch.cuda.stream(b):
        g2 = s2.subn(r2, batch)
    torch.cuda.synchronize()
    _assert_same(_host(g1), want1, "stream a")
    _assert_same(_host(g2), want2, "stream b")


def test_scratch_does_not_grow_with_k(batches):
    import torch
    lib = M.load_library()
    batch, _ = batches["pitch_lens"]
    pats = SETS["gen64"]
    cnt = M.compile_set(pats).count(batch).cpu().numpy().sum(0)
    densest = [pats[j] for j in np.argsort(-cnt, kind="stable")[:4]]
    hits_big, hits_small = int(cnt.sum()), int(np.sort(cnt)[::-1][:4].sum())

    def scratch(ps):
        torch.cuda.synchronize()
        lib.mrx_release_scratch()
        for _ in range(3):   # the arena settles within two calls of a batch shape
            ps.sub(b"x", batch)
        torch.cuda.synchronize()
        return lib.mrx_debug_scratch_bytes()

    big, small = scratch(M.compile_set(pats)), scratch(M.compile_set(densest))
    # what grows is the hits (12 bytes each), not a per-member term
    assert big <= 1.25 * small + 12 * 1.25 * (hits_big - hits_small) + (1 << 20), (big, small, hits_big, hits_small)
