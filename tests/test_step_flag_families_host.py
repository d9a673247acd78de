"""The planner's flag families that the stepper's route decision (FindallJob::choose_route in csrc/mrx_kernels.hip, the
core that sub, captures_all and split reach through csrc/mrx_core.hpp) relies on,
checked without a GPU on the route cases' patterns, the parity corpus, the empty-match, bitset and '$' lists and the
reference's benchmark patterns: which flags never meet on one plan."""
import os

import pytest

import mojo_regex_amd as M
import step_route_cases as S
from bench_engine_cases import CASES as BENCH_CASES

HERE = os.path.dirname(os.path.abspath(__file__))


def _parity_lists():
    """Every bytes literal of test_gpu_parity.py's module-level lists and parametrize lists: PATTERNS and the stepper,
    empty-match, bitset and '$' tests' own patterns (read from the file's syntax tree: importing it needs torch)."""
    import ast
    tree = ast.parse(open(os.path.join(HERE, "test_gpu_parity.py")).read())
    pats = []
    for node in ast.walk(tree):
        lists = []
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.List) and node in tree.body:
            lists.append(node.value)
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "parametrize" and len(node.args) > 1:
            lists.append(node.args[1])
        for lst in lists:
            pats += [c.value for c in ast.walk(lst) if isinstance(c, ast.Constant) and isinstance(c.value, bytes) and len(c.value) < 300]
    return pats


def _plans():
    out = []
    for f in S.FAMILIES.values():
        out.append((f.pattern, f.lazy, f.bitset))
    for p in _parity_lists() + [c.pattern for c in BENCH_CASES]:
        out.append((p, False, False))
        out.append((p, True, True))     # the bitset walk, LazyDFA reading
        out.append((p, False, True))
    return sorted(set(out))


def _flags(plan):
    try:
        return S.plan_facts(M.CompiledRegex(*plan).describe())
    except (M.RegexSyntaxError, M.UnsupportedPattern):
        return None


PLANS = [(p, f) for p, f in ((p, _flags(p)) for p in _plans()) if f is not None]


def test_the_corpus_reaches_every_family():
    assert len(PLANS) > 300
    for name, fam in S.FAMILIES.items():
        assert any(fam.member(f) for _, f in PLANS), name


@pytest.mark.parametrize("name", sorted(S.FAMILIES))
def test_every_family_has_its_member(name):
    fam = S.FAMILIES[name]
    d = M.CompiledRegex(fam.pattern, fam.lazy, fam.bitset).describe()
    assert fam.member(S.plan_facts(d)), d


def test_flag_families_are_exclusive():
    has, PF = S._has, S.PF
    for plan, f in PLANS:
        fl = f["flags"]
        step = fl & (PF["STEPPABLE"] | PF["STEP_REQ"])
        # the empty-match family needs a start state that accepts; the table / required-byte family excludes it
        if has(f, "STEP_EMPTY"):
            assert has(f, "START_ACCEPTING") and not step and not has(f, "BSTEP"), plan
        if step:
            assert not has(f, "START_ACCEPTING"), plan
        assert not (has(f, "STEPPABLE") and has(f, "STEP_REQ")), plan
        # the bitset walk needs PF_BITSET, which the table plans and the empty-match plans exclude; it brings PF_STEPPABLE
        if has(f, "BSTEP"):
            assert has(f, "BITSET", "STEPPABLE") and not fl & (PF["STEP_REQ"] | PF["STEP_BIG"] | PF["LAZY_END"]), plan
        if has(f, "BITSET"):
            assert not fl & (PF["STEP_EMPTY"] | PF["STEP_REQ"] | PF["LAZY_END"] | PF["MWALK"] | PF["MWALK_REQ"] |
                             PF["BACKSET"] | PF["MW_TRIES"] | PF["MW_EMPTY"]), plan
        # one-pass forms: where they are set
        if has(f, "MW_EMPTY"):
            assert has(f, "STEP_EMPTY") and f["mw_k"] in (-1, -2), plan
        if has(f, "MW_TRIES"):
            assert f["mw_k"] == -3 and not fl & (PF["MWALK"] | PF["STEP_REQ"] | PF["START_ACCEPTING"]), plan
        if has(f, "MWALK_REQ"):
            assert not has(f, "START_ACCEPTING"), plan
        if has(f, "BACKSET"):
            assert not has(f, "START_ACCEPTING"), plan
        if has(f, "LAZY_END"):
            assert not fl & (PF["STEP_REQ"] | PF["STEP_BIG"] | PF["BACKSET"] | PF["MWALK"] | PF["MW_TRIES"]), plan
        # a plan that may take the stepper's kernels at all carries one of the three family flags
        if fl & (PF["MWALK"] | PF["MW_TRIES"] | PF["BACKSET"] | PF["MWALK_REQ"]) and not has(f, "STREAMABLE"):
            assert step, plan
