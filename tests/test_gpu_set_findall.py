"""PatternSet.findall on the GPU: the text-major CSR of every member's findall spans equals the oracle's restatement
(tests/set_findall_expect.py) and the members' own findall calls regrouped by text, bit for bit, on CSR, fixed-pitch and
ragged batches, on every poisoned layout of tests/layouts.py, under the switches that move a member's findall to other
kernels; and the contract's edges: capacity, refusals, empty batches, 256 members, two streams, scratch that does not
grow with the set."""
import numpy as np
import pytest

import layouts as LY
import mojo_regex_amd as M
import set_findall_expect as E
from test_gpu_pattern_set import CONFIG_PATTERNS, SETS, _batches, _texts

pytestmark = pytest.mark.gpu

_CACHE = {}   # oracle findall per (pattern, text)


def _host(res):
    return tuple(np.ascontiguousarray(x.cpu().numpy()) for x in res)


def _members_regrouped(pats, batch):
    per = []
    for p in pats:
        rx = M.CompiledRegex(p)
        pre, sp, tot = rx._dev_findall(batch)
        per.append((pre.cpu().numpy(), sp[:tot].cpu().numpy()))
    return E.regroup(per, batch.n)


def _assert_same(got, want, what, texts=None):
    gp, gm, gs = got
    wp, wm, ws = want
    if np.array_equal(gp, wp) and np.array_equal(gm, wm) and np.array_equal(gs, ws):
        return
    for i in range(len(wp) - 1):
        g = list(zip(gm[gp[i]:gp[i + 1]].tolist(), gs[gp[i]:gp[i + 1]].tolist()))
        w = list(zip(wm[wp[i]:wp[i + 1]].tolist(), ws[wp[i]:wp[i + 1]].tolist()))
        if g != w:
            raise AssertionError("%s: text %d %r\n  device %s\n  want   %s" % (
                what, i, (texts[i][:120] if texts else None), g[:12], w[:12]))
    raise AssertionError("%s: same per text, different arrays" % what)


def _check_counts(s, batch, got, what):
    prefix, members, _ = got
    cnt = s.count(batch).cpu().numpy().astype(np.int64)
    assert np.array_equal(np.diff(prefix), cnt.sum(1)), what
    k = cnt.shape[1]
    text_of = np.repeat(np.arange(batch.n), np.diff(prefix))
    per = np.bincount(text_of * k + members, minlength=batch.n * k).reshape(batch.n, k)
    assert np.array_equal(per, cnt), what


@pytest.fixture(scope="module")
def batches():
    import torch
    texts = _texts(5, 1500)
    out = _batches(texts)
    out["csr_known"] = (M.DeviceBatch.from_texts(texts), texts)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("setname", list(SETS))
def test_set_findall_equals_oracle_and_members(batches, setname):
    pats = SETS[setname]
    s = M.compile_set(pats)
    for form, (batch, texts) in batches.items():
        got = _host(s.findall(batch))
        assert got[1].dtype == np.int32 and got[2].shape == (len(got[1]), 2)
        _assert_same(got, E.expected_arrays(pats, texts, _CACHE), "%s on %s vs oracle" % (setname, form), texts)
        _assert_same(got, _members_regrouped(pats, batch), "%s on %s vs members" % (setname, form), texts)
        _check_counts(s, batch, got, "%s on %s" % (setname, form))
    # host lists and findall_lists
    texts = batches["csr"][1][:200]
    hp, hm, hs = s.findall(texts)
    assert isinstance(hp, np.ndarray)
    _assert_same((hp, hm, hs), E.expected_arrays(pats, texts, _CACHE), "%s host" % setname, texts)
    assert s.findall_lists(texts) == E.expected_lists(pats, texts, _CACHE)


def _layout_set_patterns():
    pats = list(LY.PATTERNS)
    while True:
        ps = M.compile_set(pats)
        try:
            ps.findall(M.DeviceBatch.from_texts([b"ab"]))
            return pats, ps
        except M.UnsupportedPattern as exc:
            pats.pop(int(str(exc).split("member ")[1].split(":")[0]))


def test_set_findall_on_every_layout():
    pats, ps = _layout_set_patterns()
    assert len(pats) >= 15, pats
    k = len(pats)
    texts, origin = [], []
    for j, p in enumerate(pats):
        ts = LY.make_texts(p, 12, 1 if j % 8 == 0 else 0, seed=11)
        texts += ts
        origin += [j] * len(ts)
    rngs = [np.random.default_rng(j) for j in range(k)]
    pz = lambda i, t, size: LY.poison(pats[origin[i] if 0 <= i < len(origin) else 0], t, size,  # noqa: E731
                                      rngs[origin[i] if 0 <= i < len(origin) else 0])
    lays = LY.layouts_for(texts, pz, texts[:160])
    by_texts = {}
    for lay in lays:
        got = _host(ps.findall(lay.device()))
        _assert_same(got, E.expected_arrays(pats, lay.texts, _CACHE), "layout %s" % lay.name, lay.texts)
        key = tuple(lay.texts)
        if key in by_texts:
            other, name = by_texts[key]
            _assert_same(got, other, "layout %s vs %s" % (lay.name, name), lay.texts)
        else:
            by_texts[key] = (got, lay.name)


SWITCHES = {
    "force_generic1": ("mrx_debug_force_generic", 1, 0),
    "force_generic2": ("mrx_debug_force_generic", 2, 0),
    "dense_rows": ("mrx_debug_dense_rows", 1, 0),
    "tries_always": ("mrx_debug_tries_always", 1, 0),
    "multiwalk2": ("mrx_debug_multiwalk", 2, 0),
    "multiwalk3": ("mrx_debug_multiwalk", 3, 0),
}


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_set_findall_under_testing_switches(batches, switch):
    name, on, off = SWITCHES[switch]
    lib = M.load_library()
    pats = SETS["mixed7"] + SETS["gen64"][:24]
    s = M.compile_set(pats)
    for form in ("csr", "pitch_lens"):
        batch, texts = batches[form]
        getattr(lib, name)(on)
        try:
            got = _host(s.findall(batch))
        finally:
            getattr(lib, name)(off)
        _assert_same(got, E.expected_arrays(pats, texts, _CACHE), "%s on %s" % (switch, form), texts)


def test_256_members_on_a_small_batch():
    pats = [b"a%d" % i for i in range(200)] + SETS["gen64"][:56]
    texts = [b"a1 a12 a199 xyz", b"", b"a0a1a2a3", b"hello 123 foo@bar.com a55"] * 8
    s = M.compile_set(pats)
    assert len(s) == 256
    got = _host(s.findall(M.DeviceBatch.from_texts(texts)))
    _assert_same(got, E.expected_arrays(pats, texts, _CACHE), "256 members", texts)


def test_empty_batch_all_empty_texts_and_no_match():
    import torch
    s = M.compile_set(SETS["mixed7"])
    e = M.DeviceBatch(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    p, m, sp = s.findall(e)
    assert p.cpu().tolist() == [0] and m.numel() == 0 and sp.shape == (0, 2)
    p, m, sp = s.findall([])
    assert p.tolist() == [0] and len(m) == 0
    empties = [b""] * 100
    for batch in (M.DeviceBatch.from_texts(empties), M.DeviceBatch.strided(torch.zeros(1600, dtype=torch.uint8,
                                                                                       device="cuda"), 16, length=0)):
        got = _host(s.findall(batch))
        _assert_same(got, E.expected_arrays(SETS["mixed7"], empties, _CACHE), "empty texts")
    none = M.compile_set([b"qqq", b"z\\d{9}", b"@@"])
    texts = [b"abc", b"hello world", b"1234"] * 50
    p, m, sp = none.findall(M.DeviceBatch.from_texts(texts))
    assert p.cpu().numpy().tolist() == [0] * 151 and m.numel() == 0


def test_capacity():
    import torch
    lib = M.load_library()
    pats = SETS["mixed7"]
    s = M.compile_set(pats)
    texts = _texts(8, 300)
    batch = M.DeviceBatch.from_texts(texts)
    want = E.expected_arrays(pats, texts, _CACHE)
    total = int(want[0][-1])
    assert total > 10
    ptr = M.api._ptr
    for cap in (total - 1, total):
        prefix = torch.full((batch.n + 1,), -3, dtype=torch.int64, device="cuda")
        members = torch.full((total + 64,), -9, dtype=torch.int32, device="cuda")
        spans = torch.full((total + 64, 2), -9, dtype=torch.int32, device="cuda")
        tot = M.api.C.c_int64(0)
        rc = lib.mrx_set_findall_dev(s._h, ptr(batch.data), ptr(batch.offsets), batch.n, ptr(prefix), ptr(members),
                                     ptr(spans), cap, M.api.C.byref(tot), None)
        torch.cuda.synchronize()
        assert tot.value == total
        assert np.array_equal(prefix.cpu().numpy(), want[0])
        assert bool((members[cap:] == -9).all()) and bool((spans[cap:] == -9).all())   # nothing beyond the cap
        if cap < total:
            assert rc == M.api.MRX_E_CAPACITY, rc
        else:
            assert rc == M.api.MRX_OK, rc
            _assert_same((want[0], members[:total].cpu().numpy(), spans[:total].cpu().numpy()), want, "at capacity")
    # span_cap given to the Python call: no retry
    with pytest.raises(M.MrxError):
        s.findall(batch, span_cap=total - 1)
    # the default capacity too small: one retry
    dense = M.compile_set([b"a*", b"[a-z]", b"\\w*"])
    got = _host(dense.findall(M.DeviceBatch.from_texts([b"abcdefgh" * 40] * 20)))
    _assert_same(got, E.expected_arrays([b"a*", b"[a-z]", b"\\w*"], [b"abcdefgh" * 40] * 20, _CACHE), "retry")


def test_refusal_leaves_outputs_untouched():
    import torch
    s = M.compile_set([b"[a-z]+\\d+", b"(a|b)*a(a|b){5}$"])
    batch = M.DeviceBatch.from_texts([b"abc1", b"zz9"] * 100)
    prefix = torch.full((batch.n + 1,), 7, dtype=torch.int64, device="cuda")
    members = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    spans = torch.full((64, 2), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptr = M.api._ptr
    rc = s._lib.mrx_set_findall_dev(s._h, ptr(batch.data), ptr(batch.offsets), batch.n, ptr(prefix), ptr(members),
                                    ptr(spans), 64, None, None)
    assert rc == M.api.MRX_E_UNSUPPORTED and s._lib.mrx_last_error().startswith(b"member 1: ")
    with pytest.raises(M.UnsupportedPattern, match="^member 1: "):
        s.findall(batch)
    torch.cuda.synchronize()
    assert bool((prefix == 7).all()) and bool((members == 7).all()) and bool((spans == 7).all())


def test_two_sets_on_two_streams(batches):
    import torch
    s1 = M.compile_set(SETS["gen64"])
    s2 = M.compile_set(SETS["mixed7"])
    batch, _ = batches["csr_known"]
    want1, want2 = _host(s1.findall(batch)), _host(s2.findall(batch))
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        g1 = s1.findall(batch)
    with torch.cuda.stream(b):
        g2 = s2.findall(batch)
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

    def scratch(ps):
        torch.cuda.synchronize()
        lib.mrx_release_scratch()
        for _ in range(3):   # the arena settles within two calls of a batch shape
            ps.findall(batch)
        torch.cuda.synchronize()
        return lib.mrx_debug_scratch_bytes()

    big, small = scratch(M.compile_set(pats)), scratch(M.compile_set(densest))
    assert big <= 1.25 * small, (big, small)


def test_full_size_config_patterns():
    import torch
    from mojo_regex_amd.workloads import make_c2_batch
    arr = make_c2_batch(1 << 20, 1024)
    batch = M.DeviceBatch.strided(arr.reshape(-1), 1024, length=1024)
    s = M.compile_set(CONFIG_PATTERNS)
    prefix, members, spans = s.findall(batch)
    # the members' own findall regrouped, on the device: a stable sort by text of the hits laid out member by member
    tex, mem, spn = [], [], []
    for j, p in enumerate(CONFIG_PATTERNS):
        pre, sp, tot = M.CompiledRegex(p)._dev_findall(batch)
        tex.append(torch.repeat_interleave(torch.arange(batch.n, device="cuda"), pre.diff()))
        mem.append(torch.full((tot,), j, dtype=torch.int32, device="cuda"))
        spn.append(sp[:tot].clone())
        del pre, sp
    tex = torch.cat(tex)
    order = torch.sort(tex, stable=True).indices
    want_prefix = torch.zeros(batch.n + 1, dtype=torch.int64, device="cuda")
    want_prefix[1:] = torch.cumsum(torch.bincount(tex, minlength=batch.n), 0)
    assert torch.equal(prefix, want_prefix)
    assert torch.equal(members, torch.cat(mem)[order])
    assert torch.equal(spans, torch.cat(spn)[order])
