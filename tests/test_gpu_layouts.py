"""Bytes outside a text never change its result, on every device entry point.

Every entry point takes the same texts as CSR, fixed pitch with one `length`, and fixed pitch with per-text `lens`.
tests/layouts.py builds each of them with out-of-text bytes chosen to change the answer if a kernel read them (the
pattern's own bytes, the text repeated; test_layout_poison_host.py checks that they would).  Every operation, on
every layout, under every testing switch that moves the bytes to another kernel, must reproduce the oracle's answer
text by text -- computed once per (pattern, text, operation) and cached here -- and the layouts of the same texts
must agree with each other bit for bit.  The last test checks that the switches really reached the kernels they
exist for.
"""
import collections
import contextlib
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mojo_regex_amd as M  # noqa: E402
from mrx_ref import hybrid as O  # noqa: E402  (oracle: checker only)

import layouts as LY  # noqa: E402
from test_gpu_parity import (dynamic_texts, fused_findall, generic_kernels, litscan_pieces, long_text_kernels,  # noqa: E402
                             multiwalk, no_streaming_kernels, stream_bits, subs_group)

N_TEXTS, N_LONG, N_ROWS = 300, 8, 64

# plan family -> test on describe(); every family must be among LY.PATTERNS
FAMILIES = {
    "streamable, byte columns": lambda d: "device.streamable=yes" in d and ("st_kind=1 " in d or "st_kind=3 " in d),
    "streamable, class table": lambda d: "device.streamable=yes" in d and "st_kind=2 " in d,
    "exact literal": lambda d: "exact_literal=1" in d,
    "pure literal": lambda d: "pure_literal=1" in d,
    "prefilter": lambda d: "prefilter=1" in d and "exact_literal=0" in d,
    "'^' on the DFA": lambda d: "start_anchor=1 end_anchor=0" in d,
    "'$' on the anchored DFA": lambda d: "end_anchor=1" in d and "engine_type=DFA" in d,
    "'$' on the LazyDFA search": lambda d: "device.lazy_end_cache=yes" in d,
    "stepper, multi-walk": lambda d: "device.steppable=yes" in d and "multiwalk=yes" in d,
    "pending-tries walk": lambda d: "tries_walk=yes" in d,
    "required-byte route": lambda d: "required-byte route" in d,
    "backward marks": lambda d: "backset=yes" in d and "multiwalk=no" in d,
    "empty matches": lambda d: "empty_matches=1" in d,
    "bitset NFA": lambda d: "device.bitset=yes" in d,
    "backtracker route": lambda d: "backtracking matcher route" in d,
    "'.*'": lambda d: "'.*' shortcut" in d,
    "fixed-width groups": lambda d: "device.sub_groups=fixed" in d,
    "general groups": lambda d: "device.backtrack=yes" in d and " groups=0 " not in d and "device.sub_groups=fixed" not in d,
}

# (kernel, context) pairs every layout call made: the reach test reads them
REACHED = collections.defaultdict(set)
# (pattern, operation) -> the refusal message, for operations a pattern refuses on every layout alike
REFUSED = {}
# patterns (and "set") whose forced-route runs are complete
ROUTES_DONE = set()


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path has no fallback")


# ---- the oracle, once per (pattern, operation, text, argument) ----------------------------------------------------
_ORACLE = {}


def oracle(pat, op, t, arg=None):
    key = (pat, op, t, arg)
    v = _ORACLE.get(key)
    if v is None:
        orx = O.compile_regex(pat)
        if op == "findall":
            v = tuple(O.findall(pat, t))
        elif op == "search":
            v = O.search(pat, t) or (-1, -1)
        elif op == "match_first":
            v = O.match_first(pat, t) or (-1, -1)
        elif op == "is_match":
            v = bool(orx.is_match(t, 0))
        elif op == "match_first_at":
            v = (orx.match_first(t, arg) if arg >= 0 else None) or (-1, -1)
        elif op == "search_at":
            v = (orx.match_next(t, arg) if arg >= 0 else None) or (-1, -1)
        elif op == "is_match_at":
            v = bool(orx.is_match(t, arg)) if arg >= 0 else False
        elif op == "sub":
            try:
                v = orx.sub(arg[0], t, arg[1])
            except O.ReferenceDoesNotTerminate:   # the prefilter hands back a match in front of pos: no answer
                v = "none"
        elif op == "captures":
            g = arg
            want = [(-1, -1)] * (g + 1)
            if orx.fixed_total_width >= 0:
                caps = orx.captures_fixed(t)
                for gid, gs, ge in caps or ():
                    want[gid - 1 if gid else g] = (gs, ge)
            else:
                m, groups = orx.matcher.nfa_matcher.backtrack.match_next_with_groups(t, 0)
                if m is not None:
                    for gid, gs, ge in groups:
                        if 1 <= gid <= g:
                            want[gid - 1] = (gs, ge)      # the last entry of a group wins (matcher.mojo:1797-1802)
                    want[g] = m
            v = tuple(want)
        else:
            raise ValueError(op)
        _ORACLE[key] = v
    return v


def want_array(pat, op, texts, args=None):
    """The oracle's answers for a batch in the device's output form."""
    if op in ("findall", "count"):
        lists = [oracle(pat, "findall", t) for t in texts]
        prefix = np.zeros(len(texts) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in lists], out=prefix[1:])
        if op == "count":
            return np.diff(prefix).astype(np.int32)
        spans = np.array([s for x in lists for s in x], dtype=np.int32).reshape(-1, 2)
        return prefix, spans
    if args is None:
        args = [None] * len(texts)
    vals = [oracle(pat, op, t, a) for t, a in zip(texts, args)]
    if op.startswith("is_match"):
        return np.array(vals, dtype=np.uint8)
    return np.array(vals, dtype=np.int32).reshape(len(texts), -1)


# ---- one device call, its result in host form, and the kernel that ran ------------------------------------------
def run(rx, op, batch, start=None):
    if op == "findall":
        pre, sp, tot = rx._dev_findall(batch)
        return pre.cpu().numpy(), sp[:tot].cpu().numpy()
    if op == "count":
        return rx.count(batch).cpu().numpy()
    if op == "is_match":
        return rx.is_match(batch).cpu().numpy()
    if op in ("search", "match_first"):
        s, e = (rx.match_next if op == "search" else rx.match_first)(batch)
        return np.stack([s.cpu().numpy(), e.cpu().numpy()], axis=1)
    if op.endswith("_at"):
        got = rx._at(op[:-3], batch, start)
        if op == "is_match_at":
            return got.cpu().numpy()
        return np.stack([got[0].cpu().numpy(), got[1].cpu().numpy()], axis=1)
    raise ValueError(op)


def first_difference(got, want, n):
    """Index of the first text whose answer differs (findall: by CSR)."""
    if isinstance(want, tuple):
        gp, gs = got
        wp, ws = want
        for i in range(n):
            if gp[i + 1] - gp[i] != wp[i + 1] - wp[i] or not np.array_equal(gs[gp[i]:gp[i + 1]], ws[wp[i]:wp[i + 1]]):
                return i
        return -1
    bad = np.nonzero((np.asarray(got).reshape(n, -1) != np.asarray(want).reshape(n, -1)).any(axis=1))[0]
    return int(bad[0]) if len(bad) else -1


def same(got, want):
    if isinstance(want, tuple):
        return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return np.array_equal(np.asarray(got), np.asarray(want))


def expect_equal(got, want, lay, what):
    if same(got, want):
        return
    i = first_difference(got, want, len(lay.texts))
    t = lay.texts[i] if i >= 0 else None
    if i >= 0 and isinstance(want, tuple):
        g = got[1][got[0][i]:got[0][i + 1]].tolist()
        w = want[1][want[0][i]:want[0][i + 1]].tolist()
    elif i >= 0:
        g, w = np.asarray(got).reshape(len(lay.texts), -1)[i].tolist(), np.asarray(want).reshape(len(lay.texts), -1)[i].tolist()
    else:
        g = w = "(same per text, different CSR)"
    raise AssertionError("%s: text %d (len %s) %r\n  device %s\n  oracle %s\n  outside %r" % (
        what, i, None if t is None else len(t), (t or b"")[:200], g, w, lay.outside(i, 32) if i >= 0 else b""))


def kernel():
    return M.load_library().mrx_last_kernel_name().decode()


# ---- per-pattern batches --------------------------------------------------------------------------------------------
class Case:
    def __init__(self, pat):
        self.pat = pat
        self.rx = M.compile_regex(pat)
        self.texts = LY.make_texts(pat, N_TEXTS, N_LONG)
        self.layouts = LY.layouts_for(self.texts, LY.pattern_poison(pat), self.texts[:N_ROWS])
        self.batches = [lay.device() for lay in self.layouts]

    def base(self):
        """The layouts of `texts` themselves (CSR, shifted CSR, lens rows)."""
        return [(lay, b) for lay, b in zip(self.layouts, self.batches) if lay.texts == self.texts]


_CASES = {}


def case(pat):
    if pat not in _CASES:
        _CASES[pat] = Case(pat)
    return _CASES[pat]


def call(c, op, lay, batch, route, start=None):
    """run() on one layout; a refusal is returned as ("refused", message) and must be the same on every layout."""
    try:
        got = run(c.rx, op, batch, start)
    except M.UnsupportedPattern as exc:
        msg = str(exc)
        prev = REFUSED.setdefault((c.pat, op), msg)
        assert prev == msg, (c.pat, op, lay.name, prev, msg)
        return None
    assert (c.pat, op) not in REFUSED, (c.pat, op, lay.name, "refused on another layout", REFUSED[(c.pat, op)])
    REACHED[kernel()].add((c.pat, lay.name, route, op))
    return got


OPS = ("findall", "count", "search", "match_first", "is_match")


def test_every_plan_family_is_present():
    _need_gpu()
    found = collections.defaultdict(list)
    for p in LY.PATTERNS:
        d = M.compile_regex(p).describe()
        for fam, test in FAMILIES.items():
            if test(d):
                found[fam].append(p)
    missing = [f for f in FAMILIES if not found[f]]
    assert not missing, (missing, dict(found))
    assert any(p in LY.PATTERNS for p in (b"aaaaaaaaaaaaaaaaaaaaaa", b"xyxyxyxyxyxyxyxyxyxyxyxyxy"))  # self-overlapping
    assert any(M.compile_regex(p).num_groups and O.compile_regex(p).fixed_total_width < 0 for p in LY.PATTERNS)


@pytest.mark.parametrize("pat", LY.PATTERNS)
def test_every_layout_equals_the_oracle(pat):
    """findall, count, search, match_first and is_match on all twelve layouts; the layouts of the same texts agree bit
    for bit."""
    _need_gpu()
    c = case(pat)
    for op in OPS:
        ref = None
        for lay, b in zip(c.layouts, c.batches):
            got = call(c, op, lay, b, "default")
            if got is None:
                continue
            expect_equal(got, want_array(pat, op, lay.texts), lay, "%r %s on %s" % (pat, op, lay.name))
            if lay.texts == c.texts:
                if ref is None:
                    ref = got
                assert same(got, ref), (pat, op, lay.name)
    assert (pat, "findall") not in REFUSED and (pat, "match_first") not in REFUSED, REFUSED


@pytest.mark.parametrize("pat", LY.PATTERNS)
def test_start_argument_on_every_layout(pat):
    """match_first / search / is_match from a start: one start for all texts (0, 3, -1) and one per text (0, len,
    len + 1, -1 and others), on the layouts of the pattern's own texts."""
    _need_gpu()
    c = case(pat)
    n = len(c.texts)
    rng = np.random.default_rng(zlib.crc32(pat) + 3)
    lens = np.array([len(t) for t in c.texts], dtype=np.int64)
    per_text = np.select([np.arange(n) % 5 == k for k in range(4)], [np.zeros(n), lens, lens + 1, -np.ones(n)],
                         rng.integers(0, lens + 1)).astype(np.int32)
    for op in ("match_first_at", "search_at", "is_match_at"):
        for start in (0, 3, -1, per_text):
            args = list(per_text.tolist()) if isinstance(start, np.ndarray) else [start] * n
            for lay, b in c.base():
                try:
                    got = run(c.rx, op, b, start)
                except M.UnsupportedPattern as exc:
                    # the reference runs these on its backtracking matcher with absolute positions (mrx.h)
                    assert "start != 0 on an operation" in str(exc) or "per-text transition cache" in str(exc), exc
                    assert "per-text transition cache" in str(exc) or isinstance(start, np.ndarray) or start != 0
                    continue
                REACHED[kernel()].add((pat, lay.name, "default", op))
                expect_equal(got, want_array(pat, op[:-3] + "_at", lay.texts, args), lay,
                             "%r %s start=%s on %s" % (pat, op, "per-text" if isinstance(start, np.ndarray) else start,
                                                        lay.name))


# (the bitset-NFA pattern's groups are incidental, and the backtracking oracle takes minutes on its long texts)
@pytest.mark.parametrize("pat", [p for p in LY.PATTERNS if M.compile_regex(p).num_groups > 0
                                 and "device.bitset=yes" not in M.compile_regex(p).describe()])
def test_captures_on_every_layout(pat):
    """captures_dev / captures_strided_dev against captures_fixed (fixed-width groups) or the backtracking oracle."""
    _need_gpu()
    c = case(pat)
    g = c.rx.num_groups
    for lay, b in zip(c.layouts, c.batches):
        try:
            got = c.rx.captures_dev(b).cpu().numpy()
        except M.UnsupportedPattern as exc:
            REFUSED.setdefault((pat, "captures"), str(exc))
            assert REFUSED[(pat, "captures")] == str(exc)
            continue
        REACHED[kernel()].add((pat, lay.name, "default", "captures"))
        want = np.array([oracle(pat, "captures", t, g) for t in lay.texts], dtype=np.int32).reshape(got.shape)
        expect_equal(got.reshape(len(lay.texts), -1), want.reshape(len(lay.texts), -1), lay,
                     "%r captures on %s" % (pat, lay.name))


def _sub_templates(c):
    return [b"<#>"] + ([b"[\\1]" if c.rx.num_groups < 2 else b"\\2|\\1"] if c.rx.num_groups else [])


@pytest.mark.parametrize("pat", LY.PATTERNS)
def test_sub_on_every_layout(pat):
    """sub_dev with a literal template and (patterns with groups) a group template, count 0 and 1, with the
    default lanes per text, k_subs_emit for every text (0) and 16 lanes."""
    _need_gpu()
    c = case(pat)
    for lanes_ctx, route in ((contextlib.nullcontext, "default"), (lambda: subs_group(0), "subs0"),
                             (lambda: subs_group(16), "subs16")):
        for repl in _sub_templates(c):
            for count in (0, 1):
                for lay, b in zip(c.layouts, c.batches):
                    with lanes_ctx():
                        try:
                            off, out = c.rx.sub_dev(repl, b, count)
                        except M.UnsupportedPattern as exc:
                            REFUSED.setdefault((pat, "sub", repl), str(exc))
                            assert REFUSED[(pat, "sub", repl)] == str(exc)
                            continue
                        REACHED[kernel()].add((pat, lay.name, route, "sub"))
                    off, raw = off.cpu().numpy(), out.cpu().numpy().tobytes()
                    for i, t in enumerate(lay.texts):
                        if b"\\" in repl and len(t) >= 2048:   # (the group oracle backtracks for seconds per long text)
                            continue
                        w = oracle(pat, "sub", t, (repl, count))
                        if w != "none":
                            assert raw[off[i]:off[i + 1]] == w, (pat, repl, count, route, lay.name, i, t[:200],
                                                                 raw[off[i]:off[i + 1]][:200], w[:200])


@pytest.mark.parametrize("pat", LY.PATTERNS)
def test_split_ranges_on_every_layout(pat):
    """split_dev, maxsplit 0 and 2: the raw (start, end) ranges, 0 <= start <= end <= len, equal to the ranges
    derived from the oracle's findall."""
    _need_gpu()
    c = case(pat)
    for maxsplit in (0, 2):
        for lay, b in zip(c.layouts, c.batches):
            prefix, pieces, total = c.rx.split_dev(b, maxsplit)
            REACHED[kernel()].add((pat, lay.name, "default", "split"))
            pre, pc = prefix.cpu().numpy(), pieces[:total].cpu().numpy()
            for i, t in enumerate(lay.texts):
                got = [tuple(r) for r in pc[pre[i]:pre[i + 1]].tolist()]
                want = LY.split_ranges(oracle(pat, "findall", t), len(t), maxsplit)
                assert got == want, (pat, maxsplit, lay.name, i, t[:200], got[:8], want[:8])


@contextlib.contextmanager
def tries_always():
    lib = M.load_library()
    lib.mrx_debug_tries_always(1)
    try:
        yield
    finally:
        lib.mrx_debug_tries_always(0)


@contextlib.contextmanager
def dynamic_texts_only():
    """k_stream_dyn for ragged CSR batches, with the long-text treatments off: they would take the batch's outliers."""
    with long_text_kernels(2), dynamic_texts(1):
        yield


# route -> (context, does it apply to this layout)
ROUTES = {
    "default": (contextlib.nullcontext, lambda lay: True),
    "generic1": (no_streaming_kernels, lambda lay: True),
    "generic2": (generic_kernels, lambda lay: True),
    "long1": (lambda: long_text_kernels(1), lambda lay: True),
    "long3": (lambda: long_text_kernels(3), lambda lay: True),
    "dyn1": (dynamic_texts_only, lambda lay: lay.csr),
    "fused2": (lambda: fused_findall(2), lambda lay: True),
    "bits1": (lambda: stream_bits(True), lambda lay: not lay.csr and lay.stride % 16 == 0 and lay.stride <= 1024),
    "mw2": (lambda: multiwalk(2), lambda lay: True),
    "mw3": (lambda: multiwalk(3), lambda lay: True),
    "litscan1": (lambda: litscan_pieces(1), lambda lay: True),
    "tries1": (tries_always, lambda lay: True),
}
ROUTE_LAYOUTS = ("csr_packed", "csr_shift7", "rows48", "rows50", "fixed64_len45")


@pytest.mark.parametrize("pat", LY.PATTERNS)
def test_forced_routes_equal_the_oracle(pat):
    """findall, count and search under every switch that hands the bytes to another kernel, each against the oracle."""
    _need_gpu()
    c = case(pat)
    pairs = [(lay, b) for lay, b in zip(c.layouts, c.batches) if lay.name in ROUTE_LAYOUTS or lay.lens is not None]
    assert len(pairs) == len(ROUTE_LAYOUTS) + 2
    for route, (ctx, applies) in ROUTES.items():
        for op in ("findall", "count", "search"):
            for lay, b in pairs:
                if not applies(lay):
                    continue
                with ctx():
                    got = call(c, op, lay, b, route)
                if got is not None:
                    expect_equal(got, want_array(pat, op, lay.texts), lay, "%r %s on %s under %s" % (pat, op, lay.name, route))
    ROUTES_DONE.add(pat)


def test_pattern_sets_on_every_layout():
    """compile_set over the list's members that take search and count: count, search and matches under both routes
    (the shared pass k_set_scan for every eligible member, and every member's own call)."""
    _need_gpu()
    pats = list(LY.PATTERNS)
    while True:
        ps = M.compile_set(pats)
        try:
            ps.count(M.DeviceBatch.from_texts([b"ab"]))
            ps.search(M.DeviceBatch.from_texts([b"ab"]))
            break
        except M.UnsupportedPattern as exc:
            j = int(str(exc).split("member ")[1].split(":")[0])
            pats.pop(j)
    assert len(pats) >= 15, pats
    k = len(pats)
    texts, origin = [], []
    for j, p in enumerate(pats):
        ts = LY.make_texts(p, 24, 1 if j % 8 == 0 else 0, seed=11)
        texts += ts
        origin += [j] * len(ts)
    rngs = [np.random.default_rng(j) for j in range(k)]
    pz = lambda i, t, size: LY.poison(pats[origin[i] if 0 <= i < len(origin) else 0], t, size,  # noqa: E731
                                      rngs[origin[i] if 0 <= i < len(origin) else 0])
    lays = LY.layouts_for(texts, pz, texts[:N_ROWS])
    lib = M.load_library()
    for lay in lays:
        b = lay.device()
        wc = np.array([[len(oracle(p, "findall", t)) for p in pats] for t in lay.texts], dtype=np.int32)
        ws = np.array([[oracle(p, "search", t) for p in pats] for t in lay.texts], dtype=np.int32)
        for route in (1, 2):
            lib.mrx_debug_set_route(route)
            try:
                cnt = ps.count(b).cpu().numpy()
                REACHED[kernel()].add(("set", lay.name, "set_route%d" % route, "count"))
                s, e = ps.search(b)
                REACHED[kernel()].add(("set", lay.name, "set_route%d" % route, "search"))
                hits = ps.matches(b).cpu().numpy()
                REACHED[kernel()].add(("set", lay.name, "set_route%d" % route, "matches"))
                got_s = np.stack([s.cpu().numpy(), e.cpu().numpy()], axis=2)
            finally:
                lib.mrx_debug_set_route(0)
            for i in np.nonzero((cnt != wc).any(axis=1) | (got_s != ws).any(axis=(1, 2)) | (hits != (ws[:, :, 0] >= 0)).any(axis=1))[0][:1]:
                j = int(np.nonzero((cnt[i] != wc[i]) | (got_s[i] != ws[i]).any(axis=1) | (hits[i] != (ws[i, :, 0] >= 0)))[0][0])
                raise AssertionError("set route %d on %s: text %d %r member %r: count %d/%d search %s/%s matches %s" % (
                    route, lay.name, i, lay.texts[i][:200], pats[j], cnt[i, j], wc[i, j], got_s[i, j].tolist(),
                    ws[i, j].tolist(), hits[i, j]))
    ROUTES_DONE.add("set")


# kernels a poisoned layout must have reached (a routing change that turns a forced context into a no-op fails here)
MUST_REACH = [
    "k_stream_findall", "k_stream_findall_fused", "k_stream_bits", "k_stream_findall_pieces", "k_stream_findall_dyn",
    "k_stream_search", "k_stream_first", "k_stream_count",
    "k_mwalk", "k_backscan+k_step_count", "k_step_count", "k_req_wave",
    "k_findall_count", "k_match",
    "k_set_scan", "k_set_member_loop",
]


def test_forced_contexts_reached_their_kernels():
    """Runs last: every listed kernel ran on a poisoned layout (the tests above recorded mrx_last_kernel_name())."""
    _need_gpu()
    for p in LY.PATTERNS:              # (when run on its own: the runs that record the kernels)
        if p not in ROUTES_DONE:
            test_forced_routes_equal_the_oracle(p)
    if "set" not in ROUTES_DONE:
        test_pattern_sets_on_every_layout()
    reached = {k for k, ctx in REACHED.items() if any(c[1] != "csr_packed" for c in ctx)}
    missing = [k for k in MUST_REACH if k not in reached]
    assert not missing, (missing, sorted(REACHED))
