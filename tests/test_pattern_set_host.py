"""Pattern sets without a GPU: compile errors, set-size limits, routes against the members' own plans, and the packed
set tables (mrx_testing_set_run walks them on the CPU as k_set_scan does) against the oracle per member."""
import random

import pytest

import mojo_regex_amd as M
from mrx_ref import RegexSyntaxError as OracleSyntaxError
from mrx_ref import hybrid as O
from pattern_gen import patterns as gen_patterns

OP_COUNT, OP_SEARCH, OP_MATCHES = 0, 1, 2


def _member_lines(s):
    return [ln for ln in s.describe().splitlines() if ln.startswith("member ")]


def test_compile_error_carries_the_member_index():
    with pytest.raises(M.RegexSyntaxError) as ei:
        M.compile_set([b"abc", b"\\d+", b"(ab", b"x"])
    msg = str(ei.value)
    assert msg.startswith("member 2: "), msg
    with pytest.raises(OracleSyntaxError) as eo:
        O.search(b"(ab", b"")
    assert msg == "member 2: " + str(eo.value)


def test_set_size_limits():
    with pytest.raises(M.MrxError, match="set size"):
        M.compile_set([])
    with pytest.raises(M.MrxError, match="set size"):
        M.compile_set([b"a%d" % i for i in range(257)])
    s = M.compile_set([b"a%d" % i for i in range(256)])
    assert len(s) == 256
    assert len(M.PatternSet([b"x"])) == 1


def test_routes_agree_with_each_members_own_plan():
    pats = [b"[a-z]+\\d+", b"hello", b"^abc", b"abc$", b"\\d+", b"(x|y|foo|bar)+", b".*", b"a\\w*$",
            b"[a-z]+@[a-z]+\\.com", b"\\d{3}-\\d{4}"] + [p.encode() for p in gen_patterns(7, 60)
                                                         if _parses(p.encode())]
    s = M.compile_set(pats)
    lines = _member_lines(s)
    assert len(lines) == len(pats)
    for j, (p, ln) in enumerate(zip(pats, lines)):
        d = M.CompiledRegex(p).describe()
        streamable = "device.streamable=yes" in d
        findall_only = "findall_only=1" in d
        assert ln.startswith("member %d:" % j)
        count_shared = " count=shared" in ln
        search_shared = " search=shared" in ln
        assert (" matches=shared" in ln) == search_shared, ln
        # shared only where the member's own call streams; a streamable member is shared unless its tables are too big
        assert not count_shared or streamable, (p, ln, d)
        assert not search_shared or (streamable and not findall_only), (p, ln, d)
        if streamable and "too large" not in ln:
            assert count_shared, (p, ln)
            assert search_shared == (not findall_only), (p, ln)
    # '^abc' runs its anchored automaton, '.*' its shortcut, 'a\w*$' the backtracker: their own calls
    for j in (2, 6, 7):
        assert " count=own" in lines[j] and " search=own" in lines[j], lines[j]


def _parses(p):
    try:
        O.search(p, b"")
        return True
    except OracleSyntaxError:
        return False
    except Exception:
        return False


def _texts(seed, n):
    r = random.Random(seed)
    alpha = b"abcxyz019 -@.fobarhelo"
    out = [b"", b"a", b"\xff\x80\x00", b"0" * 300, b"a" * 257, b"hello world 123 foo@bar.com"]
    while len(out) < n:
        k = r.random()
        if k < 0.1:
            out.append(bytes(r.randrange(256) for _ in range(r.randrange(40))))
        elif k < 0.2:
            out.append(bytes([r.choice(alpha)]) * r.randrange(1, 200))
        else:
            out.append(bytes(r.choice(alpha) for _ in range(r.randrange(0, 90))))
    return out


def test_packed_set_tables_equal_the_oracle_per_member():
    pats = [p.encode() for p in gen_patterns(20261015, 420)]
    pats = [p for p in pats if _parses(p)][:320]
    assert len(pats) >= 300
    texts = _texts(99, 200)
    want_s, want_c = {}, {}
    for p in pats:
        want_s[p] = [O.search(p, t) for t in texts]
        want_c[p] = [len(O.findall(p, t)) for t in texts]
    checked = {OP_COUNT: 0, OP_SEARCH: 0}
    sizes = [1, 5, 32, 100]
    i = 0
    while i < len(pats):
        size = sizes[(i // 7) % len(sizes)]
        members = pats[i:i + size]
        i += size
        s = M.compile_set(members)
        k = len(members)
        for ti, t in enumerate(texts):
            c = s._host_run(OP_COUNT, t)
            se = s._host_run(OP_SEARCH, t)
            mt = s._host_run(OP_MATCHES, t)
            for j, p in enumerate(members):
                if c[j] != -2:
                    assert c[j] == want_c[p][ti], (p, t, c[j], want_c[p][ti])
                    checked[OP_COUNT] += 1
                if se[2 * j] != -2:
                    w = want_s[p][ti]
                    assert (se[2 * j], se[2 * j + 1]) == (w if w else (-1, -1)), (p, t, se[2 * j:2 * j + 2], w)
                    assert mt[j] == (1 if w else 0), (p, t)
                    checked[OP_SEARCH] += 1
                else:
                    assert mt[j] == -2
        assert k == len(s)
    # most generated patterns are streamable: the shared pass is what is being checked
    assert checked[OP_COUNT] >= 100 * len(texts), checked
    assert checked[OP_SEARCH] >= 80 * len(texts), checked


def test_member_refusal_is_reported_before_anything_is_enqueued():
    # member 1's search is refused (its '$' LazyDFA cache exceeds what is tracked); the set call fails on the
    # argument checks' heels, before it touches a device -- which is why this runs without one
    s = M.compile_set([b"[a-z]+\\d+", b"(a|b)*a(a|b){5}$"])
    lib = M.load_library()
    fake = 1 << 40   # never dereferenced
    for fn in (lib.mrx_set_search_dev,):
        rc = fn(s._h, fake, fake, 10, fake, fake, None)
        assert rc == 2 and lib.mrx_last_error().startswith(b"member 1: "), (rc, lib.mrx_last_error())
    rc = lib.mrx_set_count_strided_dev(s._h, fake, 64, None, 64, 10, fake, None)
    assert rc == 2 and lib.mrx_last_error().startswith(b"member 1: ")
    rc = lib.mrx_set_matches_strided_dev(s._h, fake, 64, None, 65, 10, fake, None)
    assert rc == 5   # len > stride: argument rules of the single-pattern calls
