"""captures_all's three routes on the GPU, each held to the oracle on generated patterns (tests/capall_gen.py) with no
text beyond 4096 bytes in the batch, so that the kernel that runs is the one the plan names (`device.capall=` of
describe()): k_capall_chain, k_capall_fixed or k_capall_emit.  Also the chain kernel's tile edges, the span capacity's
first guess and hint, and what stands on the rows: extract(group=), expand, value_counts(group=) and sub()."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mojo_regex_amd as M  # noqa: E402
import capall_gen as G  # noqa: E402
import captures_all_expect as CA  # noqa: E402
import expand_expect as E  # noqa: E402
import extract_expect as X  # noqa: E402
import layouts as LY  # noqa: E402
from test_gpu_extract import _assert_result  # noqa: E402
from test_gpu_parity import generic_kernels  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _oracle_c_backtracker():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with G.c_backtracker():
        yield


def _rows_of(prefix, groups, i):
    return [[(int(a), int(b)) for a, b in r] for r in groups[int(prefix[i]):int(prefix[i + 1])].tolist()]


def _run(rx, batch, count, kernel, where):
    """captures_all on a device batch: (prefix, groups) as numpy arrays and as device tensors; the kernel is asserted."""
    p, g = rx.captures_all(batch, count)
    name = M.load_library().mrx_last_kernel_name()
    assert name == kernel, (where, name, kernel)
    pn, gn = p.cpu().numpy(), g.cpu().numpy()
    assert pn.shape == (batch.n + 1,) and gn.shape == (int(pn[-1]), rx.num_groups + 1, 2), where
    return pn, gn, p, g


def _against_oracle(case, count, pn, gn):
    checked = 0
    for i, want in enumerate(case.rows_for(count)):
        if want is None:
            continue
        assert _rows_of(pn, gn, i) == want, (case.pat, case.route, count, i, case.texts[i])
        checked += 1
    assert checked > 0, (case.pat, count)


def _generated(case, ran):
    """One generated pattern at every count: the kernel of its route, the rows against the oracle text by text and, on
    the chain route, against the lane-per-text interpreter bit for bit."""
    rx = M.compile_regex(case.pat)
    assert rx.num_groups == case.g, case.pat
    batch = M.DeviceBatch.from_texts(case.texts)
    for count in G.COUNTS:
        pn, gn, p, g = _run(rx, batch, count, G.KERNEL[case.route], (case.pat, count))
        _against_oracle(case, count, pn, gn)
        if case.route == "chain":
            with generic_kernels():
                _, _, p2, g2 = _run(rx, batch, count, b"k_capall_emit", (case.pat, count, "generic"))
            assert torch.equal(p, p2) and torch.equal(g, g2), (case.pat, count)
    ran[case.route].append(case)


def test_generated_chains_on_the_chain_route_equal_the_oracle():
    ran = collections.defaultdict(list)
    for case in G.cases("chain"):
        if case.route == "chain":
            _generated(case, ran)
    cen = G.chain_census(G.cases("chain"))   # (the declined share is the family's; the rest counts what ran)
    assert cen == dict(G.chain_census(ran["chain"]), chain_declined=cen["chain_declined"])
    print("generated chains: %d on k_capall_chain; with %d rows or more: %s" % (len(ran["chain"]), G.MIN_ROWS, cen))
    G.check_chain_census(cen)


OFF_CHAIN_PARTS = 4


@pytest.mark.parametrize("part", range(OFF_CHAIN_PARTS))
def test_generated_chains_off_the_chain_route_equal_the_oracle(part):
    """The generated chains whose plan is not the chain route's (programs that backtrack among them, on the interpreter's
    full backtracker), every one of them, a quarter per case of this test."""
    ran = collections.defaultdict(list)
    rest = [c for c in G.cases("chain") if c.route != "chain"]
    assert len(rest) >= 200
    for case in rest[part::OFF_CHAIN_PARTS]:
        _generated(case, ran)
    backtracking = sum(" chain=1" not in M.compile_regex(c.pat).describe() for c in ran["general"])
    print("generated chains, part %d: %d on k_capall_emit (%d of them programs that backtrack), %d on k_capall_fixed"
          % (part, len(ran["general"]), backtracking, len(ran["fixed"])))
    assert not ran["chain"] and len(ran["general"]) + len(ran["fixed"]) == len(rest[part::OFF_CHAIN_PARTS])
    assert backtracking >= 20, backtracking   # (129 of the 388 generated chains: a quarter of them, with a margin)


def test_generated_fixed_width_forms_on_their_route_equal_the_oracle():
    """The rows are raw (a window may reach behind its text); extract(group=j) is where the clamp acts."""
    ran = collections.defaultdict(list)
    for case in G.cases("fixed"):
        _generated(case, ran)
        rx = M.compile_regex(case.pat)
        texts = [t for t, r in zip(case.texts, case.rows_for(0)) if r is not None]
        batch = M.DeviceBatch.from_texts(texts)
        for j in range(case.g + 1):
            _assert_result(rx.extract(batch, group=j), X.expected_group(case.pat, texts, j), (case.pat, j))
    cen = G.fixed_census(ran["fixed"] + ran["general"])
    print("generated fixed-width forms: %d on k_capall_fixed, %d on k_capall_emit; with %d rows or more: %s"
          % (len(ran["fixed"]), len(ran["general"]), G.MIN_ROWS, cen))
    assert not ran["chain"]
    G.check_fixed_census(cen)


# ---- tile edges of k_capall_chain ------------------------------------------------------------------------------------
# pattern -> (units: a match and a byte no leaf takes, of several lengths; tail: a match that ends the long text)
TILE_PATTERNS = {
    b"(\\w+) (\\w+)": ([b"ab cd;", b"a b;", b"hello w0rld_;;"], b"ab cd"),
    b"((\\w+)-(\\d+))": ([b"ab-12;", b"a-1;", b"x_y-2026 ;"], b"ab-12"),
    b"(?:([a-z])(\\d+)) ": ([b"a12 ;", b"b7 ", b"zz2026 ;;"], b"a12 "),
    b"([a-c]{2,3})(x+)(\\d)": ([b"abxx1;", b"abcx7", b"ccxxxx0;;"], b"abcx1"),
    b"([a-z]+)-(\\d{2,4})": ([b"ab-123;", b"a-12;", b"hello-2026;;"], b"ab-12"),
    b"([a-zA-Z0-9._%+-]+)@([a-zA-Z0-9.-]+)": ([b"a_b@cd.e;", b"a@b;", b"first.last+tag@example-host.org;;"], b"a@b.c"),
}
TILE_LENGTHS = (2047, 2048, 2049, 4095, 4096, 4097)


def _long_text(pat, length, seed):
    units, tail = TILE_PATTERNS[pat]
    rng = np.random.default_rng(seed)
    body = b""
    while len(body) < length:
        body += units[int(rng.integers(len(units)))]
    return body[:length - len(tail) - 1] + b";" + tail


_tile_rows = {}   # (pattern, text) -> the oracle's rows, computed once


def _tile_want(pat, text, g):
    key = (pat, text)
    if key not in _tile_rows:
        _tile_rows[key] = CA.expected_rows(pat, text, 0, g)
    return _tile_rows[key]


@pytest.mark.parametrize("pat", list(TILE_PATTERNS), ids=[p.decode() for p in TILE_PATTERNS])
def test_chain_tile_edges(pat):
    """One text of exactly L bytes whose last match ends at its last byte, first in the buffer at every alignment, among
    short texts: L up to 4096 is the chain kernel's (its 2048 and 4096 tile forms to their last byte), 4097 hands the
    whole batch to the interpreter."""
    rx = M.compile_regex(pat)
    assert G.route_of(rx.describe()) == "chain"
    g = rx.num_groups
    units, tail = TILE_PATTERNS[pat]
    many = units[0] * 130
    short = LY.make_texts(pat, 16, n_long=0) + [b"", units[0] + tail, b";;;;", tail, many]
    assert len(_tile_want(pat, many, g)) > 128               # a lane of the wavefront takes three rows
    assert _tile_want(pat, short[-3], g) == [] and _tile_want(pat, short[-4], g) and _tile_want(pat, short[-2], g)
    pz = LY.pattern_poison(pat)
    for length in TILE_LENGTHS:
        long_text = _long_text(pat, length, length)
        want_long = _tile_want(pat, long_text, g)
        assert len(long_text) == length and want_long[-1][-1][1] == length
        texts = [long_text] + short
        kernel = b"k_capall_chain" if length <= 4096 else b"k_capall_emit"
        for shift in (range(16) if length in (2048, 4096) else (0, 1, 15)):
            lay = LY.csr_shifted(texts, shift, pz)
            lay.check()
            batch = lay.device()
            assert (batch.data.data_ptr() + shift) % 16 == shift
            pn, gn, _, _ = _run(rx, batch, 0, kernel, (pat, length, shift))
            for i, t in enumerate(texts):
                assert _rows_of(pn, gn, i) == _tile_want(pat, t, g), (pat, length, shift, i, t[:60])


# ---- span capacity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pat,route,dense,sparse", [
    (b"(\\d)", "fixed", b"0123456789" * 60, b"no digit here, none at all; then 7 and much later 42 "),
    (b"([a-z])(\\d)", "chain", b"a1b2c3d4e5" * 60, b"words without digits behind them, then q7 and ;; z9 "),
], ids=["fixed", "chain"])
def test_span_capacity_first_guess_then_the_hint(pat, route, dense, sparse):
    """Nearly every byte begins a match: the first guess of the span capacity (a match per 8 bytes) is too small and the
    call repeats its findall; the second call sizes the spans by the handle's hint; a sparse batch follows."""
    rx = M.CompiledRegex(pat)   # (a fresh handle: no hint yet)
    assert G.route_of(rx.describe()) == route
    g = rx.num_groups
    dense_texts = [dense[k:k + 400 + 7 * k] for k in range(40)] + [b""]
    sparse_texts = [sparse * (1 + k % 5) for k in range(40)] + [b"", dense[:64]]
    assert sum(len(t) for t in dense_texts) >= 8192
    for texts, least in ((dense_texts, 0.45), (dense_texts, 0.45), (sparse_texts, 0.0), (dense_texts, 0.45)):
        batch = M.DeviceBatch.from_texts(texts)
        pn, gn, _, _ = _run(rx, batch, 0, G.KERNEL[route], (pat, len(texts)))
        assert int(pn[-1]) >= least * sum(len(t) for t in texts)
        for i, t in enumerate(texts):
            assert _rows_of(pn, gn, i) == CA.expected_rows(pat, t, 0, g), (pat, i, t[:40])


# ---- what stands on the rows -----------------------------------------------------------------------------------------
def _templates(g):
    lacking = b"[\\%d:\\1]" % (g + 1) if g < 9 else b"[\\1]"
    return [E.all_groups_template(g), lacking]


@pytest.mark.parametrize("family", ["chain", "fixed"])
def test_expand_value_counts_and_sub_on_generated_patterns(family):
    """Every fourth generated pattern: expand and value_counts(group=1) against the oracle, and sub() with the same
    template against the product's own captures_all rows (k_subc_emit and k_capall_chain held to each other)."""
    by_route = collections.Counter()
    for case in G.cases(family)[::4]:
        rx = M.compile_regex(case.pat)
        keep = [i for i, r in enumerate(case.rows_for(0)) if r is not None]
        texts = [case.texts[i] for i in keep]
        rows = [case.rows_for(0)[i] for i in keep]
        batch = M.DeviceBatch.from_texts(texts)
        for tpl in _templates(case.g):
            _assert_result(rx.expand(tpl, batch), E.from_rows(tpl, rows, texts), (case.pat, tpl))
        pieces = [p for ps in X.lists(X.pack([[r[0] for r in rs] for rs in rows], texts)) for p in ps]
        assert rx.value_counts(texts, group=1) == list(collections.Counter(pieces).items()), case.pat
        pn, gn, _, _ = _run(rx, batch, 0, G.KERNEL[case.route], case.pat)
        tpl = _templates(case.g)[0]
        got = rx.sub(tpl, texts)
        for i, t in enumerate(texts):
            assert got[i] == CA.sub_from_rows(tpl, t, _rows_of(pn, gn, i)), (case.pat, tpl, t)
        by_route[case.route] += 1
    print("expand / value_counts / sub on generated %s patterns, by captures_all route: %s" % (family, dict(by_route)))
    # (a quarter of the census floor of the family's own route)
    assert by_route["chain" if family == "chain" else "fixed"] >= G.FLOORS[family] // 4, by_route
