"""The stepper family's routes, pinned: every case of step_route_cases.py launches the kernels that
tests/golden/step_routes.json records (tools/record_step_routes.py, run before the route decision of findall and count
became one), and every result equals the oracle's.

From the fifth eligible call on a tuner's route is the clock's choice: those calls must take one of the two routes the
first four took, and answer the same."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mojo_regex_amd as M  # noqa: E402
import step_route_cases as S  # noqa: E402
from mrx_ref import hybrid as O  # noqa: E402  (oracle: checker only)
from mrx_ref.hybrid import CompiledRegex as OracleRegex  # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_routes.json")) as _f:
    GOLDEN = json.load(_f)["routes"]

_texts, _batches, _spans, _subs = {}, {}, {}, {}


def _reference(case):
    """Texts, device batch and the oracle's findall of a (family, shape): computed once, shared by the cases, never changed."""
    f = S.FAMILIES[case.family]
    tkey = (case.family, "csr320" if case.shape == "pitch320" else case.shape, case.alphabet)
    if tkey not in _texts:
        _texts[tkey] = S.texts_for(case.family, case.shape, case.alphabet)
        o = OracleRegex(f.pattern, force_nfa=f.lazy)
        _spans[tkey] = [o.match_all(t) for t in _texts[tkey]]
    bkey = (case.family, case.shape, case.alphabet)
    if bkey not in _batches:
        _batches[bkey] = S.make_batch(M, torch, case.shape, _texts[tkey])
    if case.op == "sub" and tkey not in _subs:
        _subs[tkey] = [O.sub(f.pattern, S.SUB_REPL, t) for t in _texts[tkey]]
    return _texts[tkey], _batches[bkey], _spans[tkey], _subs.get(tkey)


def test_the_case_list_is_the_recorded_one():
    assert sorted(GOLDEN) == sorted(c.id for c in S.CASES)


@pytest.mark.parametrize("family", sorted(S.FAMILIES))
def test_every_family_has_its_member(family):
    """A planner change must not silently empty a row of the table: the family's pattern still compiles to its plan."""
    f = S.FAMILIES[family]
    d = M.CompiledRegex(f.pattern, f.lazy, f.bitset).describe()
    assert f.member(S.plan_facts(d)), d


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.id)
def test_route_and_result(case):
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path has no fallback")
    texts, batch, spans, subs = _reference(case)
    names, results = S.run_case(M, torch, case, batch, sum(len(t) for t in texts))
    want_names = GOLDEN[case.id]
    ops = S.ops_of(case)
    seen = {}
    for k, (op, name, res) in enumerate(zip(ops, names, results)):
        print(case.id, k, op, name)
        nth = seen[op] = seen.get(op, 0) + 1
        if nth <= 4:   # by construction: a tuner's first four calls alternate
            assert name == want_names[k], (case.id, k, names, want_names)
        else:          # the clock's choice
            assert name in {want_names[j] for j in range(len(ops)) if ops[j] == op and j < k}, (case.id, k, names, want_names)
        if op == "findall":
            assert res == spans, (case.id, k, next(i for i in range(len(texts)) if res[i] != spans[i]))
        elif op == "sub":
            assert res == subs, (case.id, k, next(i for i in range(len(texts)) if res[i] != subs[i]))
        else:
            assert res == [len(s) for s in spans], (case.id, k)
