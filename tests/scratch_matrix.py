"""The calls at which the bookkeeping of per-call device scratch can go wrong: every entry point on three small batch
shapes, the routes forced with the switches of include/mrx_testing.h, sub's two retries and the refused calls.

cases(scale) gives one Case per call; Case.run(check) makes the call and, with check, compares its result with the
oracle (the helpers of test_gpu_layouts.py and the *_expect.py modules) or expects the refusal it names.
test_gpu_scratch_scope.py asserts that nothing is in use after each of them; tools/scratch_footprint.py prints what the
arena holds after each of them."""
import contextlib
from typing import Callable, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

import mojo_regex_amd as M
from mrx_ref import hybrid as O

import captures_all_expect as CE
import filter_expect as FE
import set_findall_expect as SFE
import set_sub_expect as SSE
import test_gpu_layouts as GL
from test_gpu_pattern_set import MIXED

STREAM, STEPPER = b"[a-z]+\\d+", b"\\d{3}-\\d{4}"             # the two plans of smoke()'s long-text run
MULTIWALK, MARKS, BITSET = b"\\w+\\d{2}", b"[A-Z]{10,20}[0-9]{15,25}|ab", b"(a|b)*a(a|b){12}"
BACKTRACK, PREFILTER = b"hello.*", b"\\w+@\\w+\\.com"         # bt_prepass(); the memchr prefilter's view
FIXED_GROUPS, CHAIN_GROUPS, GENERAL_GROUPS = b"(\\d{3})(\\d{3})(\\d{4})", b"(\\w+) (\\w+)", b"(a|ab)(c|bcd)(d*)"
REACH = b"x(\\d)?"                                             # a group that reaches behind a text ending in "x"
NO_SEARCH = b"(a|b)*a(a|b){5}$"                                # search is refused (describe(): support.search)

Switch = Optional[Tuple[str, int, int]]   # (hook of include/mrx_testing.h, value, value that restores the default)


class Case(NamedTuple):
    name: str
    switch: Switch
    run: Callable[[bool], None]


@contextlib.contextmanager
def switched(switch: Switch):
    lib = M.load_library()
    if switch:
        getattr(lib, switch[0])(switch[1])
    try:
        yield
    finally:
        if switch:
            getattr(lib, switch[0])(switch[2])


def make_batches(scale: int = 1):
    """name -> (DeviceBatch, texts): 130 CSR texts of 0..200 bytes (two full wavefronts and a remainder, an empty text
    among them), 128 x 64 bytes and 64 x 2048 bytes at a fixed pitch; `scale` multiplies the number of texts."""
    rng = np.random.default_rng(20261017)
    al = np.frombuffer(b"abcxyzAB0189 -@.", dtype=np.uint8)
    words = [b"hello world", b"555-1234", b"ab12", b"foo@bar.com", b"5551234567", b"ABCDEFGHIJKL012345678901234567", b"abx"]

    def text(k):
        t = bytearray(al[rng.integers(0, len(al), size=k)].tobytes())
        for _ in range(k // 40 + 1):
            w = words[int(rng.integers(0, len(words)))]
            if len(w) <= k:
                a = int(rng.integers(0, k - len(w) + 1))
                t[a:a + len(w)] = w
        return bytes(t)

    ragged = [text(int(rng.integers(0, 201))) for _ in range(130 * scale)]
    ragged[5], ragged[64] = b"", b"a" * 200
    out = {"csr": (M.DeviceBatch(*(torch.from_numpy(a).cuda() for a in M.pack_texts(ragged))), ragged)}
    for name, n, L in (("p64", 128 * scale, 64), ("p2048", 64 * scale, 2048)):
        rows = [text(L) for _ in range(n)]
        d = torch.from_numpy(np.frombuffer(b"".join(rows), dtype=np.uint8).copy()).cuda()
        out[name] = (M.DeviceBatch.strided(d, L, length=L), rows)
    torch.cuda.synchronize()
    return out


def _np(t):
    return t.cpu().numpy()


# refused by contract (run_at): '^' and the literal prefilter's look-back of the backtracking matcher need absolute positions
REFUSED_AT = {(BACKTRACK, "search_at"): "start != 0 on an operation the reference runs on its backtracking matcher"}


# the backtracker-routed plan runs the lane-per-text kernels, behind bt_prepass()'s literal pass (pinned with describe())
BACKTRACK_KERNELS = {"search": b"k_match", "findall": b"k_findall_count", "count": b"k_findall_count"}


def _span_ops(pat, batch, texts, op, check):
    starts = (np.arange(len(texts), dtype=np.int32) % 7) if op.endswith("_at") else None
    if (pat, op) in REFUSED_AT:   # a refused call of its own: the refusal is what is checked
        try:
            GL.run(M.compile_regex(pat), op, batch, starts)
        except M.UnsupportedPattern as e:
            assert str(e).startswith(REFUSED_AT[(pat, op)]), e
            return
        raise AssertionError("%r %s was not refused" % (pat, op))
    got = GL.run(M.compile_regex(pat), op, batch, starts)
    if check:
        want = GL.want_array(pat, op, texts, None if starts is None else [int(s) for s in starts])
        assert GL.same(got, want), (pat, op, GL.first_difference(got, want, len(texts)))
        if pat == BACKTRACK and op in BACKTRACK_KERNELS:
            assert "backtracking matcher route" in M.compile_regex(pat).describe()
            assert M.load_library().mrx_last_kernel_name() == BACKTRACK_KERNELS[op], (op, M.load_library().mrx_last_kernel_name())


def _captures(pat, batch, texts, check):
    rx = M.compile_regex(pat)
    got = _np(rx.captures_dev(batch))
    if check:
        want = GL.want_array(pat, "captures", texts, [rx.num_groups] * len(texts))
        assert np.array_equal(got.reshape(len(texts), -1), want), (pat, "captures")


def _split(pat, batch, texts, check):
    prefix, pieces, total = M.compile_regex(pat).split_dev(batch, 2)
    if check:
        prefix, pieces = _np(prefix), _np(pieces)
        for i, t in enumerate(texts):
            got = [t[a:b] for a, b in pieces[prefix[i]:prefix[i + 1]]]
            assert got == O.split(pat, t, 2), (pat, "split", i)


def _sub(pat, repl, batch, texts, check, count=0, rx=None, kernel=None):
    off, out = (rx or M.compile_regex(pat)).sub_dev(repl, batch, count)
    if check:
        if kernel:   # the route the case is about
            assert M.load_library().mrx_last_kernel_name() == kernel, (pat, M.load_library().mrx_last_kernel_name())
        off, raw = _np(off), _np(out).tobytes()
        for i, t in enumerate(texts):
            assert raw[off[i]:off[i + 1]] == GL.oracle(pat, "sub", t, (repl, count)), (pat, repl, "sub", i)


def _sub_second_attempt(batch, texts, check):
    """Pattern `a` on texts of 200 x `a`: more matches than the first attempt's bytes / 8 + n + 64 spans.  A handle of
    its own, so that no earlier call has left the density hint that would size the first attempt for them."""
    nbytes, n = sum(len(t) for t in texts), len(texts)
    assert all(set(t) == {ord("a")} for t in texts) and nbytes > nbytes // 8 + n + 64
    _sub(b"a", b"bc", batch, texts, check, rx=M.CompiledRegex(b"a"), kernel=b"k_subs_wave")   # (still the spans route)


def _captures_all(pat, batch, texts, check):
    rx = M.compile_regex(pat)
    prefix, groups = rx.captures_all(batch)
    if check:
        prefix, groups = _np(prefix), _np(groups)
        for i, t in enumerate(texts):
            want = CE.expected_rows(pat, t, 0, rx.num_groups)
            assert [[tuple(int(x) for x in p) for p in row] for row in groups[prefix[i]:prefix[i + 1]]] == want, (pat, i)


def _filter(pat, batch, texts, check):
    kb, idx = M.compile_regex(pat).filter(batch)
    if check:
        widx, woff, wdata = FE.expected([pat], texts)
        assert np.array_equal(_np(idx), widx) and np.array_equal(_np(kb.offsets), woff) and np.array_equal(_np(kb.data), wdata)


_SET_CACHE = {}


def _set(op, batch, texts, check):
    s = M.compile_set(MIXED)
    if op == "matches":
        got = _np(s.matches(batch))
        if check:
            for j, p in enumerate(MIXED):
                want = np.array([GL.oracle(p, "search", t) != (-1, -1) for t in texts])
                assert np.array_equal(got[:, j], want), ("set matches", p)
    elif op == "findall":
        got = tuple(_np(x) for x in s.findall(batch))
        if check:
            want = SFE.expected_arrays(MIXED, texts, _SET_CACHE)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), "set findall"
    else:
        reps = [b"<%d>" % j for j in range(len(MIXED))]
        got = tuple(_np(x) for x in s.subn(reps, batch))
        if check:
            want = SSE.expected_arrays(MIXED, reps, texts, 0, _SET_CACHE)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), "set sub"


def _refused(kind, batches, check):
    """One refused call; with check, the refusal itself is what is asserted."""
    lib = M.load_library()
    batch, texts = batches["csr"]
    rx = M.compile_regex(STREAM)
    n = batch.n
    stream = rx._stream_ptr()
    prefix = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    spans = torch.empty((max(8, int(batch.data.numel())), 2), dtype=torch.int32, device="cuda")
    total = M.api.C.c_int64(-7)
    if kind == "span capacity of 8":
        rc = lib.mrx_findall_dev(rx._h, batch.data.data_ptr(), batch.offsets.data_ptr(), n, prefix.data_ptr(),
                                 spans.data_ptr(), 8, M.api.C.byref(total), stream)
        need = sum(len(GL.oracle(STREAM, "findall", t)) for t in texts) if check else total.value
        want = (M.api.MRX_E_CAPACITY, b"span buffer too small: need %d" % need)
    elif kind == "offsets[n] = -5":
        off = batch.offsets.clone()
        off[n] = -5
        rc = lib.mrx_findall_dev(rx._h, batch.data.data_ptr(), off.data_ptr(), n, prefix.data_ptr(), spans.data_ptr(),
                                 spans.shape[0], M.api.C.byref(total), stream)
        want = (M.api.MRX_E_ARGUMENT, b"offsets[n] is negative")
    elif kind == "null offsets":
        s = torch.empty(n, dtype=torch.int32, device="cuda")
        rc = lib.mrx_search_dev(rx._h, batch.data.data_ptr(), None, n, s.data_ptr(), s.data_ptr(), stream)
        want = (M.api.MRX_E_ARGUMENT, b"null offsets")
    elif kind == "unsupported search":
        assert "support.search=yes" not in M.compile_regex(NO_SEARCH).describe()
        s = torch.empty(2 * n, dtype=torch.int32, device="cuda")
        rc = lib.mrx_search_dev(M.compile_regex(NO_SEARCH)._h, batch.data.data_ptr(), batch.offsets.data_ptr(), n, s.data_ptr(),
                                s.data_ptr() + 4 * n, stream)
        want = (M.api.MRX_E_UNSUPPORTED, None)
    else:   # a sub output capacity that is too small
        out_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        out = torch.empty(16, dtype=torch.uint8, device="cuda")
        rc = lib.mrx_sub_dev(rx._h, b"<>", 2, 0, batch.data.data_ptr(), batch.offsets.data_ptr(), n, out_off.data_ptr(),
                             out.data_ptr(), 16, M.api.C.byref(total), stream)
        need = sum(len(GL.oracle(STREAM, "sub", t, (b"<>", 0))) for t in texts) if check else total.value
        want = (M.api.MRX_E_CAPACITY, b"output buffer too small: need %d" % need)
    torch.cuda.synchronize()
    if check:
        assert rc == want[0], (kind, rc, lib.mrx_last_error())
        assert want[1] is None or lib.mrx_last_error() == want[1], (kind, lib.mrx_last_error())


SPAN_OPS = ("match_first", "search", "is_match", "match_first_at", "search_at", "is_match_at", "findall", "count")


class _Lazy(dict):
    """The batches, uploaded when the first case runs (listing the cases needs no device)."""

    def __init__(self, scale):
        super().__init__()
        self.scale = scale

    def __missing__(self, key):
        self.update(make_batches(self.scale))
        texts = self["csr"][1]
        # sub's two retries: more matches than bytes / 8 + n + 64, and a group that reaches behind its text
        for name, tx in (("many", [b"a" * 200] * len(texts)), ("behind", [t[:-1] + b"x" if t else b"x" for t in texts])):
            self[name] = (M.DeviceBatch(*(torch.from_numpy(a).cuda() for a in M.pack_texts(tx))), tx)
        return self[key]


def cases(scale: int = 1) -> List[Case]:
    B = _Lazy(scale)
    out: List[Case] = []

    def add(name, switch, fn):
        out.append(Case(name + ("" if not switch else " [%s(%d)]" % (switch[0][len("mrx_debug_"):], switch[1])), switch, fn))

    def span_ops(pat, shapes, switch=None, ops=SPAN_OPS):
        for shape in shapes:
            for op in ops:
                add("%s %s %s" % (op, pat.decode(), shape), switch,
                    lambda check, pat=pat, shape=shape, op=op: _span_ops(pat, *B[shape], op, check))

    def results(pat, shapes, switch=None):   # the calls that size a result on the device
        for shape in shapes:
            add("split %s %s" % (pat.decode(), shape), switch, lambda check, pat=pat, shape=shape: _split(pat, *B[shape], check))
            add("sub %s %s" % (pat.decode(), shape), switch, lambda check, pat=pat, shape=shape: _sub(pat, b"<>", *B[shape], check))
            add("filter %s %s" % (pat.decode(), shape), switch, lambda check, pat=pat, shape=shape: _filter(pat, *B[shape], check))

    # every entry point, default routes
    for pat in (STREAM, STEPPER, MULTIWALK, MARKS, BITSET, BACKTRACK, PREFILTER):
        span_ops(pat, ("csr", "p64"))
    for pat in (STREAM, STEPPER, BACKTRACK):
        results(pat, ("csr", "p64"))
    for pat in (STREAM, STEPPER, MULTIWALK):   # 2 KiB rows: the wide-slot rows of the stepper, findall's event rows below
        span_ops(pat, ("p2048",), ops=("search", "findall", "count"))
    for pat in (FIXED_GROUPS, CHAIN_GROUPS, GENERAL_GROUPS, REACH):
        for shape in ("csr", "p64"):
            add("captures %s %s" % (pat.decode(), shape), None, lambda check, pat=pat, shape=shape: _captures(pat, *B[shape], check))
            add("captures_all %s %s" % (pat.decode(), shape), None,
                lambda check, pat=pat, shape=shape: _captures_all(pat, *B[shape], check))
    for pat, repl in ((FIXED_GROUPS, b"\\2-\\1"), (CHAIN_GROUPS, b"\\2 \\1"), (GENERAL_GROUPS, b"\\3\\2\\1")):
        add("sub %s %s csr" % (pat.decode(), repl.decode()), None, lambda check, pat=pat, repl=repl: _sub(pat, repl, *B["csr"], check))
    for op in ("matches", "findall", "sub"):
        for shape in ("csr", "p64"):
            add("set %s %s" % (op, shape), None, lambda check, op=op, shape=shape: _set(op, *B[shape], check))
    # forced routes
    long1 = ("mrx_debug_long_text_kernels", 1, 0)   # pieces with C = 200
    for pat in (STREAM, STEPPER):
        span_ops(pat, ("csr", "p2048"), long1, ops=("search", "findall", "count"))
        results(pat, ("csr", "p2048"), long1)
    for level in (1, 2):
        sw = ("mrx_debug_force_generic", level, 0)
        for pat in (STREAM, STEPPER, BACKTRACK):
            span_ops(pat, ("csr",), sw, ops=("match_first", "search", "findall", "count"))
        results(STREAM, ("csr",), sw)
        add("captures_all %s csr" % CHAIN_GROUPS.decode(), sw, lambda check: _captures_all(CHAIN_GROUPS, *B["csr"], check))
        add("set findall csr", sw, lambda check: _set("findall", *B["csr"], check))
    for sw, shapes in ((("mrx_debug_fused_findall", 2, 0), ("csr", "p64", "p2048")), (("mrx_debug_dynamic_texts", 1, 0), ("csr",)),
                       (("mrx_debug_dense_rows", 1, 0), ("p2048",))):
        span_ops(STREAM, shapes, sw, ops=("findall", "count", "search"))
        add("sub %s %s" % (STREAM.decode(), shapes[0]), sw, lambda check, shape=shapes[0]: _sub(STREAM, b"<>", *B[shape], check))
    for pat in (MULTIWALK, MARKS, STEPPER):
        span_ops(pat, ("csr", "p2048"), ("mrx_debug_multiwalk", 2, 0), ops=("search", "findall", "count"))
    # sub's two retries: more matches than bytes / 8 + n + 64 (the second attempt), a group behind its text (the generic form)
    add("sub a, 200 x a: second attempt", None, lambda check: _sub_second_attempt(*B["many"], check))
    add("sub x(\\d)? \\1, texts ending in x: generic form", None, lambda check: _sub(REACH, b"\\1", *B["behind"], check, kernel=b"k_sub_size"))
    add("captures_all x(\\d)?, texts ending in x", None, lambda check: _captures_all(REACH, *B["behind"], check))
    # refused calls
    for kind in ("span capacity of 8", "offsets[n] = -5", "null offsets", "unsupported search", "sub output capacity of 16"):
        add("refused: " + kind, None, lambda check, kind=kind: _refused(kind, B, check))
    return out
