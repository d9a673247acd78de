"""Generated patterns with capture groups for captures_all's three routes, their texts and the oracle's rows.

Two families: chains of classes and literals with groups around runs of their elements (the chain route,
k_capall_chain, where build_plan proves the chain; the interpreter elsewhere), and patterns in the reference's
"fixed-width" form -- (\\d{N}) groups with anything between them, which its detector counts as one literal byte each, so
that the windows of a row need not lie where the match puts them (k_capall_fixed, or the interpreter where the plan's
search has no spans route).  The route of a pattern is read from describe() (`device.capall=`), which needs no GPU.

Host-only: imports the oracle, numpy and the product library's host half; no torch, no device.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import captures_all_expect as CA
import layouts as LY
import mojo_regex_amd as M
import mrx_ref.hybrid as H

CHAIN_SEED, CHAIN_N = 20261101, 400
FIXED_SEED, FIXED_N = 20261102, 300
MIN_ROWS = 10
COUNTS = (0, 1, 3)
KERNEL = {"chain": b"k_capall_chain", "fixed": b"k_capall_fixed", "general": b"k_capall_emit"}
# the floors of tests/test_capall_gen_host.py, asserted again by the GPU module on what ran
FLOORS = {"chain": 50, "chain_by_groups": 15, "chain_nested": 20, "fixed": 60, "fixed_general": 20}
MAX_DECLINED = 0.05

Pair = Tuple[int, int]
Rows = Optional[List[List[Pair]]]   # None: the oracle declined the (pattern, text) pair


@contextlib.contextmanager
def c_backtracker():
    """The oracle's backtracking matcher as its C twin (equal to the Python one on every reference vector and on
    generated patterns: tests/test_oracle_c.py), as tests/big_fuzz.py switches it on.  The oracle's compile cache is
    emptied on both sides, so that no matcher of the other kind is reused."""
    before = H.USE_C_BACKTRACK
    H.USE_C_BACKTRACK = True
    H.clear_regex_cache()
    try:
        yield
    finally:
        H.USE_C_BACKTRACK = before
        H.clear_regex_cache()


def random_chain_with_groups(rng):
    """A random chain of classes and literals with quantifiers, capture groups around runs of its elements (nested now
    and then), and a replacement template over the groups."""
    atoms = ["\\w", "\\d", "\\s", "[a-z]", "[a-c]", "[0-9a-f]", "[^ ]", " ", "-", "\\.", "@", "x", "a", ":"]
    quants = ["", "", "+", "+", "{2}", "{1,3}", "{2,}", "{3,5}"]
    n = int(rng.integers(1, 7))
    elems = [atoms[int(rng.integers(len(atoms)))] + quants[int(rng.integers(len(quants)))] for _ in range(n)]
    opens, closes = [0] * (n + 1), [0] * (n + 1)
    ngroups = int(rng.integers(1, 4))
    for _ in range(ngroups):
        a = int(rng.integers(0, n))
        b = int(rng.integers(a + 1, n + 1))
        opens[a] += 1
        closes[b] += 1
    # (groups opened at a and closed at b in any order nest or overlap: close the inner ones first by emitting every
    # close in front of the opens of the same position -- overlapping pairs are then simply another nesting)
    pat = ""
    depth = 0
    for i in range(n):
        c = min(closes[i], depth)
        pat += ")" * c
        depth -= c
        pat += "(" * opens[i]
        depth += opens[i]
        pat += elems[i]
    pat += ")" * depth
    refs = [b"\\1", b"\\2", b"\\3", b"\\4", b"<", b">", b"-", b"", b"::", b"x"]
    repl = b"".join(refs[int(rng.integers(len(refs)))] for _ in range(int(rng.integers(1, 6))))
    if b"\\" not in repl:
        repl += b"\\1"
    return pat.encode(), repl


FIXED_WIDTHS = (1, 2, 3, 4, 5, 8)
FIXED_GROUP_QUANTS = ("?", "+", "*", "{2}")
FIXED_LITERALS = ("a", "x", "-", " ", ":", "\\.", "\\s", "\\w", ".", "/", "\\d")
FIXED_LITERAL_QUANTS = ("?", "*", "+", "{2}", "{1,2}")


def random_fixed_form(rng) -> bytes:
    """1 to 5 pieces, each a (\\d) / (\\d{N}) group -- one in seven with a quantifier behind it -- or a "literal", which
    the reference's detector counts as one byte whatever it is; '^' in front and '$' behind one time in ten each."""
    n = int(rng.integers(1, 6))
    is_group = [bool(rng.integers(0, 2)) for _ in range(n)]
    if not any(is_group):
        is_group[int(rng.integers(0, n))] = True
    pat = "^" if rng.random() < 0.1 else ""
    for grp in is_group:
        if grp:
            w = FIXED_WIDTHS[int(rng.integers(len(FIXED_WIDTHS)))]
            pat += "(\\d)" if w == 1 and rng.random() < 0.5 else "(\\d{%d})" % w
            if rng.random() < 1 / 7:
                pat += FIXED_GROUP_QUANTS[int(rng.integers(len(FIXED_GROUP_QUANTS)))]
        else:
            pat += FIXED_LITERALS[int(rng.integers(len(FIXED_LITERALS)))]
            if rng.random() < 0.3:
                pat += FIXED_LITERAL_QUANTS[int(rng.integers(len(FIXED_LITERAL_QUANTS)))]
    if rng.random() < 0.1:
        pat += "$"
    return pat.encode()


def chain_patterns(seed: int = CHAIN_SEED, n: int = CHAIN_N) -> List[bytes]:
    rng = np.random.default_rng(seed)
    return list(dict.fromkeys(random_chain_with_groups(rng)[0] for _ in range(n)))


def fixed_patterns(seed: int = FIXED_SEED, n: int = FIXED_N) -> List[bytes]:
    rng = np.random.default_rng(seed)
    return list(dict.fromkeys(random_fixed_form(rng) for _ in range(n)))


def route_of(describe: str) -> Optional[str]:
    """'chain', 'fixed' or 'general': the kernel captures_all takes on a CSR batch with no text beyond 4096 bytes (KERNEL);
    None for a pattern whose groups captures_all does not read."""
    for line in describe.split("\n"):
        if line.startswith("device.capall="):
            return line[len("device.capall="):]
    return None


def nested(pat: bytes) -> bool:
    """A capturing group inside a capturing group (the generators write no escaped parenthesis and no class with one)."""
    depth = 0
    for c in pat.decode():
        if c == "(":
            depth += 1
            if depth > 1:
                return True
        elif c == ")":
            depth -= 1
    return False


@dataclass
class Case:
    pat: bytes
    route: str
    g: int
    nested: bool
    texts: List[bytes]
    rows: Dict[int, List[Rows]]   # count -> the oracle's rows per text; filled by rows_for()

    def rows_for(self, count: int) -> List[Rows]:
        if count not in self.rows:
            self.rows[count] = [_oracle_rows(self.pat, t, count, self.g) for t in self.texts]
        return self.rows[count]

    @property
    def nrows(self) -> int:
        return sum(len(r) for r in self.rows_for(0) if r is not None)

    @property
    def declined(self) -> int:
        return sum(r is None for r in self.rows_for(0))


def _oracle_rows(pat: bytes, text: bytes, count: int, g: int) -> Rows:
    try:
        return CA.expected_rows(pat, text, count, g)
    except (H.ReferenceDoesNotTerminate, H.UnsupportedByOracle):
        return None


# The reference's backtracker is cubic and worse where adjacent leaves share their bytes, and the interpreter restates it:
# on an MI355X one captures_all call on this pattern's 60 texts of up to 200 bytes took 7.3 s (the next slowest
# generated chain 0.4 s, all 387 others 9 s for four calls each).  Its texts are cut to this many bytes, on the host and
# on the GPU alike; it stays in every test.
CUT_TEXTS = {b"\\w+\\w+(\\d+[0-9a-f]+((-{3,5}))[a-c]{1,3})": 64}


def texts_for(pat: bytes) -> List[bytes]:
    """No text beyond the chain kernel's tile: the route is the plan's."""
    texts = LY.make_texts(pat, 60, n_long=0)
    return [t[:CUT_TEXTS[pat]] for t in texts] if pat in CUT_TEXTS else texts


_cases: Dict[str, List[Case]] = {}


def cases(family: str) -> List[Case]:
    """Every generated pattern of `family` ('chain' or 'fixed'), none left out, with its route, its texts and the
    oracle's rows for count = 0.  Computed once per process, under the oracle's C backtracker, and never changed; call
    it (and Case.rows_for) inside c_backtracker()."""
    if family not in _cases:
        out = []
        for pat in (chain_patterns() if family == "chain" else fixed_patterns()):
            route = route_of(M.compile_regex(pat).describe())
            assert route is not None, pat   # (the generators write nothing that captures_all refuses)
            case = Case(pat, route, CA.num_groups(pat), nested(pat), texts_for(pat), {})
            case.rows_for(0)
            out.append(case)
        _cases[family] = out
    return _cases[family]


def chain_census(cs: Sequence[Case]) -> Dict[str, object]:
    """What the floors of the chain family are about: its chain-route cases with at least MIN_ROWS oracle rows, by group
    count and nesting, and the share of its (pattern, text) pairs the oracle declined."""
    ch = [c for c in cs if c.route == "chain" and c.nrows >= MIN_ROWS]
    return {
        "chain": len(ch),
        "chain_by_groups": [sum(c.g == k for c in ch) for k in (1, 2, 3)],
        "chain_nested": sum(c.nested for c in ch),
        "chain_declined": _share(cs),
    }


def fixed_census(cs: Sequence[Case]) -> Dict[str, object]:
    """The same for the fixed-width forms: the cases with at least MIN_ROWS oracle rows on either of their routes."""
    fx = [c for c in cs if c.nrows >= MIN_ROWS]
    return {
        "fixed": sum(c.route == "fixed" for c in fx),
        "fixed_general": sum(c.route == "general" for c in fx),
        "fixed_declined": _share(cs),
    }


def _share(cs: Sequence[Case]) -> float:
    pairs = sum(len(c.texts) for c in cs)
    assert pairs > 0
    return sum(c.declined for c in cs) / pairs


def check_chain_census(cen: Dict[str, object]) -> None:
    assert cen["chain"] >= FLOORS["chain"], cen
    assert min(cen["chain_by_groups"]) >= FLOORS["chain_by_groups"], cen
    assert cen["chain_nested"] >= FLOORS["chain_nested"], cen
    assert cen["chain_declined"] <= MAX_DECLINED, cen


def check_fixed_census(cen: Dict[str, object]) -> None:
    assert cen["fixed"] >= FLOORS["fixed"], cen
    assert cen["fixed_general"] >= FLOORS["fixed_general"], cen
    assert cen["fixed_declined"] <= MAX_DECLINED, cen
