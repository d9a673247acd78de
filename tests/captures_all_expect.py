"""captures_all's expected answers, restated from the oracle's primitives as the loop of sub() with a group template
(oracle/mrx_ref/hybrid.py::_sub_impl, matcher.mojo:1679-1854; the contract is in include/mrx.h).

Host-only: imports the oracle, neither torch nor the product library.  expected_rows() raises
O.ReferenceDoesNotTerminate where the reference's loop would not end (a match in front of pos); callers skip those texts.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

from mrx_ref import hybrid as O

# (copied from test_gpu_parity.py, whose import loads torch and the product library)
GROUP_PATTERNS = [
    (b"(\\w+) (\\w+)", b"\\2 \\1"), (b"(\\d+)", b"[\\1,\\1]"), (b"(?:hello) (\\w+)", b"\\1"), (b"(\\d+)", b"[\\1]"),
    (b"(\\w+)@(\\w+)\\.com", b"\\2 at \\1"), (b"([a-z]+)(\\d*)x", b"<\\1|\\2>"), (b"^(\\w+)\\s+(\\w+)$", b"\\2,\\1"),
    (b"(a*)(b+)c", b"\\2\\1"), (b"\\s*(\\d+)\\s*", b"(\\1)"), (b"([a-z0-9]+)-([^-]+)", b"\\2-\\1"),
    (b"(\\d{2,4})-(\\d+)", b"\\2/\\1"), (b"x(.*)y", b"[\\1]"), (b"([a-zA-Z0-9._%+-]+)@([a-zA-Z0-9.-]+)", b"\\1 AT \\2"),
    (b"(\\w+)\\s(\\s*)(\\w*)", b"\\3\\2\\1"), (b"((\\w+)-(\\d+))", b"\\3:\\2:\\1"), (b"(\\d+)\\.(\\d+)", b"\\2.\\1 \\9"),
    (b"(h.llo) (w.*d)", b"\\2 \\1"), (b"([A-Z][a-z]+) ([A-Z][a-z]+)", b"\\2, \\1"), (b"(\\s+)(\\S?)", b"_\\2"),
    # alternation (_match_or) and quantified groups (_match_group_with_quantifier / the zero-repetition rule for a
    # quantified group that is not the last child of its sequence)
    (b"(a|b)(c)", b"\\2\\1"), (b"(ab)+(c)", b"<\\1\\2>"), (b"(\\w+)|(\\d+)", b"[\\1|\\2]"), (b"((a)|b)x", b"\\2\\1"),
    (b"(cat|dog)s? (\\w+)", b"\\2 \\1"), (b"x(a|b)?bc", b"[\\1]"), (b"(\\d+)(ab)*", b"\\1"), (b"(ab|a)(bc|c)?", b"\\1-\\2"),
    (b"(a(b|c)d)+", b"\\2\\1"), (b"((\\w)(\\d))*", b"\\3\\2"), (b"(foo|bar|baz)=(\\d+|x)", b"\\2=\\1"), (b"(a|ab)(c|bcd)(d*)", b"\\3\\2\\1"),
    (b"([a-c]+|\\d)x(y|z)*", b"\\1\\2"), (b"(a+|b+)+", b"<\\1>"), (b"(?:(x)|(y)|(z))+", b"\\1\\2\\3"),
]
CHAIN_SUBS = [(b"(\\w+) (\\w+)", b"\\2 \\1"), (b"(\\w+) (\\w+)", b"<\\2|\\1|\\2>"), (b"(\\w+) (\\w+)", b"\\3x\\1"),
              (b"([a-z]+)(\\d+)", b"\\2\\1"), (b"([a-z]+)-(\\d{2,4})", b"[\\2:\\1]"), (b"(\\d+)\\.(\\d+)", b"\\2,\\1"),
              (b"([a-c]{2,3})(x+)(\\d)", b"\\3\\2\\1"), (b"((\\d+)-([a-z]+))", b"\\3=\\2 (\\1)"), (b"(?:([a-z])(\\d+)) ", b"\\1"),
              (b"(\\d+)", b"<\\1>"), (b"([a-z]+)@([a-z]+)\\.(com|org)", b"\\2")]
# fixed-width group form: phone and date shapes, a group that can reach behind its text, and a "concat" pattern (groups
# only: the whole-text shortcut on texts of exactly its width)
FIXED_PATTERNS = [b"(\\d{3})(\\d{3})(\\d{4})", b"(\\d{4})-(\\d{2})-(\\d{2})", b"x(\\d)?", b"(\\d{2})-(\\d{3})",
                  b"(\\d{2})(\\d{3})"]

Pair = Tuple[int, int]


def num_groups(pat: bytes) -> int:
    """mrx_num_groups: the fixed form's group count, else the highest capturing group id (at most 9)."""
    orx = O.compile_regex(pat)
    if orx.fixed_total_width >= 0:
        return orx.fixed_num_groups
    g, i, cls = 0, 0, False
    while i < len(pat):
        c = pat[i:i + 1]
        if c == b"\\":
            i += 2
            continue
        if cls:
            cls = c != b"]"
        elif c == b"[":
            cls = True
            if pat[i + 1:i + 2] == b"]":
                i += 1
        elif c == b"(" and pat[i + 1:i + 2] != b"?":
            g += 1
        i += 1
    return min(g, 9)


def expected_rows(pat: bytes, text: bytes, count: int = 0, g: int = None) -> List[List[Pair]]:
    """The matches of sub()'s loop on `text`, at most `count` (0 = all), each as g + 1 pairs: groups 1..g, then the
    whole match.  Spans are raw (a fixed-width group may reach behind the text); a group without an entry is (-1, -1)."""
    orx = O.compile_regex(pat)
    if g is None:
        g = num_groups(pat)
    orx._enter()
    orx._depth += 1   # (as CompiledRegex.sub: the match_next calls of one text share one LazyDFA cache)
    try:
        return _rows(orx, text, count, g)
    finally:
        orx._depth -= 1


def _rows(orx, text: bytes, count: int, g: int) -> List[List[Pair]]:
    tl = len(text)
    if tl == 0:
        return []
    rows = []
    if orx.fixed_total_width >= 0:
        offs, widths = orx.fixed_offsets, orx.fixed_widths

        def row(ms, me):
            return [(ms + offs[j], ms + offs[j] + widths[j]) if j <= orx.fixed_num_groups else (-1, -1)
                    for j in range(1, g + 1)] + [(ms, me)]

        if orx.fixed_concat and tl == orx.fixed_total_width:
            return [row(0, tl)] if all(0x30 <= b <= 0x39 for b in text) else []
        nxt = lambda pos: orx.match_next(text, pos)   # noqa: E731
    else:
        bt = orx.matcher.nfa_matcher.backtrack
        found = {}

        def nxt(pos):
            m, groups = bt.match_next_with_groups(text, pos)
            found.clear()
            for gid, gs, ge in groups:
                found[gid] = (gs, ge)   # a later entry of the same group wins
            return m

        def row(ms, me):
            return [found.get(j, (-1, -1)) for j in range(1, g + 1)] + [(ms, me)]
    pos = 0
    while pos <= tl:
        m = nxt(pos)
        if m is None:
            break
        ms, me = m
        if (me + 1 if me == ms else me) <= pos:
            raise O.ReferenceDoesNotTerminate(text)
        rows.append(row(ms, me))
        pos = me + 1 if me == ms else me
        if count > 0 and len(rows) >= count:
            break
    return rows


def sub_from_rows(repl: bytes, text: bytes, rows: Sequence[Sequence[Pair]]) -> bytes:
    """sub(pattern, repl, text, count) assembled from the rows of that call's matches: the gaps between them, and per
    match the template with each \\j read from the row's group j (cut at the end of the text, as the oracle does)."""
    if not text:
        return text
    g = len(rows[0]) - 1 if rows else 0
    tpl = O._parse_repl_template(repl)
    out, pos = b"", 0
    for r in rows:
        ms, me = r[-1]
        if ms > pos:
            out += text[pos:ms]
        for gref, s, ln in tpl:
            if gref > 0:
                if gref <= g and r[gref - 1][0] >= 0:
                    gs, ge = r[gref - 1]
                    out += text[gs:ge]
            else:
                out += repl[s:s + ln]
        if me == ms:
            if pos < len(text):
                out += text[pos:pos + 1]
            pos = me + 1
        else:
            pos = me
    if pos < len(text):
        out += text[pos:]
    return out
