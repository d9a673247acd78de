"""Pattern sets on the GPU: every member's column equals that member's own single-pattern _dev call, element for
element, on CSR (unaligned offsets, empty texts) and fixed-pitch batches, under both routes; a sample against the oracle."""
import random

import numpy as np
import pytest

import mojo_regex_amd as M
from mrx_ref import hybrid as O
from pattern_gen import patterns as gen_patterns

pytestmark = pytest.mark.gpu

CONFIG_PATTERNS = [b"hello", b"[a-z]+\\d+", b"\\d+", b"(\\d{3})(\\d{3})(\\d{4})", b"(x|y|foo|bar)+"]
# prefilter, '^', '$', NFA-routed, backtracker, '.*', exact literal
MIXED = [b"[a-z]+@[a-z]+\\.com", b"^[a-z]+", b"\\d+$", b"(a|ab)(c|bcd)(d*)", b"a\\w*$", b".*", b"foo"]


def _ok(p):
    try:
        O.search(p, b"")
        return "support.search=yes" in M.CompiledRegex(p).describe()   # (refused members fail the whole call)
    except Exception:
        return False


GEN = [p.encode() for p in gen_patterns(424242, 160)]
GEN = [p for p in GEN if _ok(p)]
SETS = {"one": [b"[a-z]+\\d+"], "mixed7": MIXED, "gen64": GEN[:64], "gen100": GEN[:100]}


def _texts(seed, n):
    r = random.Random(seed)
    alpha = b"abcxyz0123456789 -@.fohelbr.com"
    out = []
    for i in range(n):
        k = r.random()
        if i % 17 == 0:
            out.append(b"")
        elif k < 0.1:
            out.append(bytes(r.randrange(256) for _ in range(r.randrange(60))))
        else:
            out.append(bytes(r.choice(alpha) for _ in range(r.randrange(0, 300))))
    return out


def _batches(texts):
    import torch
    n = len(texts)
    # CSR, shifted by 3 bytes so that no text starts aligned
    data, off = M.pack_texts(texts)
    d = torch.zeros(data.size + 3, dtype=torch.uint8, device="cuda")
    if data.size:
        d[3:] = torch.from_numpy(data).cuda()
    csr = M.DeviceBatch(d, torch.from_numpy(off + 3).cuda())
    L = 320
    arr = np.zeros((n, L), np.uint8)
    lens = np.zeros(n, np.int32)
    for i, t in enumerate(texts):
        arr[i, :len(t)] = np.frombuffer(t, np.uint8) if t else arr[i, :0]
        lens[i] = len(t)
    dev = torch.from_numpy(arr).cuda().reshape(-1)
    pitch_lens = M.DeviceBatch.strided(dev, L, lens=torch.from_numpy(lens).cuda())
    full = torch.from_numpy(np.ascontiguousarray(arr[:, :256])).cuda().reshape(-1)
    aligned = M.DeviceBatch.strided(full, 256, length=256)
    full_texts = [arr[i, :256].tobytes() for i in range(n)]
    return {"csr": (csr, texts), "pitch_lens": (pitch_lens, texts), "pitch_aligned": (aligned, full_texts)}


def _single(p, op, batch):
    rx = M.CompiledRegex(p)
    if op == "count":
        return rx.count(batch).cpu().numpy()
    s, e = rx._dev_spans(rx._lib.mrx_search_dev, rx._lib.mrx_search_strided_dev, batch)
    return s.cpu().numpy(), e.cpu().numpy()


@pytest.fixture(scope="module")
def batches():
    return _batches(_texts(5, 3000))


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("setname", list(SETS))
def test_set_equals_members_single_calls(batches, setname, route):
    import torch
    lib = M.load_library()
    pats = SETS[setname]
    s = M.compile_set(pats)
    lib.mrx_debug_set_route(route)
    try:
        for form, (batch, texts) in batches.items():
            c = s.count(batch).cpu().numpy()
            st, en = s.search(batch)
            st, en = st.cpu().numpy(), en.cpu().numpy()
            mt = s.matches(batch).cpu().numpy()
            torch.cuda.synchronize()
            assert c.shape == (batch.n, len(pats)) and mt.dtype == bool
            for j, p in enumerate(pats):
                wc = _single(p, "count", batch)
                ws, we = _single(p, "search", batch)
                assert np.array_equal(c[:, j], wc), (form, p, np.nonzero(c[:, j] != wc)[0][:5])
                assert np.array_equal(st[:, j], ws) and np.array_equal(en[:, j], we), (form, p)
                assert np.array_equal(mt[:, j], ws >= 0), (form, p)
                for i in range(0, batch.n, 397):
                    w = O.search(p, texts[i])
                    assert (st[i, j], en[i, j]) == (w if w else (-1, -1)), (form, p, texts[i])
                    assert c[i, j] == len(O.findall(p, texts[i])), (form, p, texts[i])
    finally:
        lib.mrx_debug_set_route(0)


def test_all_streamable_set_runs_the_set_kernel(batches):
    lib = M.load_library()
    s = M.compile_set([b"[a-z]+\\d+", b"\\d+", b"foo", b"[a-c]+x"])
    assert "own" not in s.describe().split("\n", 1)[1]
    batch, _ = batches["pitch_aligned"]
    lib.mrx_debug_set_route(1)
    try:
        for op in (s.count, s.search, s.matches):
            op(batch)
            assert lib.mrx_last_kernel_name() == b"k_set_scan"
    finally:
        lib.mrx_debug_set_route(0)
    s.count(batch)   # the route rule: the members' own calls (measured faster, profiles/set_scan.md)
    assert lib.mrx_last_kernel_name() == b"k_set_member_loop"


def test_full_size_config_patterns():
    import torch
    from mojo_regex_amd.workloads import make_c2_batch
    arr = make_c2_batch(1 << 16, 1024)
    batch = M.DeviceBatch.strided(arr.reshape(-1), 1024, length=1024)
    s = M.compile_set(CONFIG_PATTERNS)
    c = s.count(batch)
    st, en = s.search(batch)
    mt = s.matches(batch)
    torch.cuda.synchronize()
    for j, p in enumerate(CONFIG_PATTERNS):
        rx = M.CompiledRegex(p)
        assert torch.equal(c[:, j], rx.count(batch)), p
        ws, we = rx._dev_spans(rx._lib.mrx_search_dev, rx._lib.mrx_search_strided_dev, batch)
        assert torch.equal(st[:, j], ws) and torch.equal(en[:, j], we), p
        assert torch.equal(mt[:, j], ws >= 0), p


def test_empty_batch_and_two_streams(batches):
    import torch
    s1 = M.compile_set(SETS["gen64"])
    s2 = M.compile_set(MIXED)
    e = M.DeviceBatch(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert s1.count(e).shape == (0, len(s1))
    assert s1.search(e)[0].shape == (0, len(s1))
    assert s1.matches(e).shape == (0, len(s1))
    batch, _ = batches["csr"]
    want1, want2 = s1.count(batch).clone(), s2.count(batch).clone()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        g1 = s1.count(batch)
    with torch.cuda.stream(b):
        g2 = s2.count(batch)
    torch.cuda.synchronize()
    assert torch.equal(g1, want1) and torch.equal(g2, want2)


def test_member_refusal_fails_before_any_output():
    import torch
    # '$' on the LazyDFA search with more states than the per-text cache tracks: search refused for that member
    s = M.compile_set([b"[a-z]+\\d+", b"(a|b)*a(a|b){5}$"])
    batch = M.DeviceBatch.from_texts([b"abc1", b"zz9"] * 100)
    out = torch.full((batch.n, 2), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for fn in (s._lib.mrx_set_count_dev,):
        rc = fn(s._h, M.api._ptr(batch.data), M.api._ptr(batch.offsets), batch.n, M.api._ptr(out), None)
        assert rc == 2 and s._lib.mrx_last_error().startswith(b"member 1: "), rc
    with pytest.raises(M.UnsupportedPattern, match="^member 1: "):
        s.search(batch)
    torch.cuda.synchronize()
    assert bool((out == 7).all())
