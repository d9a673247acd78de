"""The generators of tests/capall_gen.py without a GPU: the census that keeps tests/test_gpu_capall_routes.py from
running empty, the route line of describe() on the hand patterns whose kernels the GPU suite pins, and the generators'
own shape."""
import re

import numpy as np

import capall_gen as G
import mojo_regex_amd as M


def test_census_of_the_generated_patterns():
    """From the seeds in capall_gen: at least 50 chain-route patterns with 10 oracle rows or more (15 each of 1, 2 and 3
    groups, 20 nested), 60 fixed-route and 20 general-route patterns of the fixed-width form, and the oracle declines at
    most 5 % of the (pattern, text) pairs of either family."""
    with G.c_backtracker():
        chain, fixed = G.cases("chain"), G.cases("fixed")
        cen = dict(G.chain_census(chain), **G.fixed_census(fixed))
    print("census", cen)
    G.check_chain_census(cen)
    G.check_fixed_census(cen)
    assert [c.pat for c in chain] == G.chain_patterns() and [c.pat for c in fixed] == G.fixed_patterns()
    assert len(chain) > 350 and len(fixed) > 200
    for c in chain + fixed:
        assert c.declined < len(c.texts), c.pat   # (every pattern meets the oracle on some text)
        assert max(len(t) for t in c.texts) <= 4096 and len(c.texts) == 60, c.pat


def test_route_line_of_describe():
    """`device.capall=`: the kernel captures_all takes on a CSR batch without a text beyond 4096 bytes."""
    want = {b"(\\d{3})(\\d{3})(\\d{4})": "fixed", b"(\\d{4})-(\\d{2})-(\\d{2})": "fixed", b"(\\w+) (\\w+)": "chain",
            b"([a-z]+)-(\\d{2,4})": "chain", b"((\\w+)-(\\d+))": "chain", b"(?:([a-z])(\\d+)) ": "chain",
            b"(a|ab)(c|bcd)(d*)": "general", b"(\\w+)|(\\d+)": "general",
            b"(\\d{2})(\\d{3})": "fixed",    # nothing but groups: the whole-text shortcut is the match
            b"(\\d{2})-(\\d{3})": "fixed"}
    for pat, route in want.items():
        d = M.compile_regex(pat).describe()
        assert G.route_of(d) == route, (pat, d)
        assert d.count("device.capall=") == 1
    # a pattern whose groups captures_all refuses has no route
    assert G.route_of(M.compile_regex(b"(" * 17 + b"a" + b")" * 17 + b"(b)").describe()) is None


def test_generators_are_seeded_and_in_form():
    assert G.chain_patterns() == G.chain_patterns() and G.fixed_patterns() == G.fixed_patterns()
    assert G.chain_patterns(1, 20) != G.chain_patterns(2, 20)
    piece = r"(?:\((?:\\d|\\d\{[123458]\})\)(?:[?+*]|\{2\})?|(?:[ax\- :./]|\\[.swd])(?:[?*+]|\{2\}|\{1,2\})?)"
    form = re.compile(r"\^?" + piece + r"{1,5}\$?")
    pats = G.fixed_patterns()
    assert len(pats) > 200
    for p in pats:
        assert form.fullmatch(p.decode()) and b"(" in p, p
    quantified = sum(bool(re.search(rb"\)(?:[?+*]|\{2\})", p)) for p in pats)
    anchored = sum(p.startswith(b"^") or p.endswith(b"$") for p in pats)
    assert quantified >= 20 and anchored >= 20, (quantified, anchored)
    rng = np.random.default_rng(3)
    for _ in range(50):
        pat, repl = G.random_chain_with_groups(rng)
        assert pat.count(b"(") == pat.count(b")") >= 1 and b"\\" in repl
    assert G.nested(b"((\\w+)-(\\d+))") and not G.nested(b"(\\w+) (\\w+)")
