"""captures_all's expectation helper (tests/captures_all_expect.py) against the oracle, without a GPU: the rows it gives
for sub()'s loop, put back together with the template, must be exactly what the oracle's sub returns."""
import zlib

import numpy as np
import pytest

from mrx_ref import hybrid as O
import captures_all_expect as E

FIXED_SUBS = [(b"(\\d{3})(\\d{3})(\\d{4})", b"(\\1) \\2-\\3"), (b"(\\d{4})-(\\d{2})-(\\d{2})", b"\\2/\\3/\\1"),
              (b"x(\\d)?", b"[\\1]"), (b"(\\d{2})-(\\d{3})", b"\\2\\1\\9"), (b"(\\d{2})(\\d{3})", b"\\2.\\1")]
CASES = list(E.GROUP_PATTERNS) + list(E.CHAIN_SUBS) + FIXED_SUBS


def _texts(pat: bytes, n: int = 120):
    rng = np.random.default_rng(zlib.crc32(pat) ^ 0xCA11)
    al = np.frombuffer(b"abcxyz0123456789 -.@helowrdHW_\t,+" + bytes(c for c in pat if chr(c).isalnum()) * 2, np.uint8)
    out = [bytes(rng.choice(al, size=int(rng.integers(0, 80))).tolist()) for _ in range(n)]
    out += [b"", b"6502530000", b"Call 6502530000 or 4155551234 today.", b"2026-04-12 and 2025-12-25", b"hello world foo",
            b"x", b"x1x", b"12345", b"12-345", b"abcd", b"acd", b"xaayxbby"]
    tw = O.compile_regex(pat).fixed_total_width
    if tw > 0:   # texts of exactly the fixed width: the whole-text shortcut of "concat" patterns
        digits = np.frombuffer(b"0123456789", np.uint8)
        out += [bytes(rng.choice(digits, size=tw).tolist()) for _ in range(6)] + [b"1" * (tw - 1) + b"a"]
    return out


def test_the_helper_does_not_load_the_product():
    import importlib
    src = importlib.util.find_spec("captures_all_expect").origin
    text = open(src).read()
    assert "import torch" not in text and "mojo_regex_amd" not in text


def test_pinned_rows():
    """'(a|ab)(c|bcd)(d*)': findall finds (0, 4) in "abcd", sub()'s loop nothing; on "acd" one match."""
    p = b"(a|ab)(c|bcd)(d*)"
    assert O.findall(p, b"abcd") == [(0, 4)]
    assert E.expected_rows(p, b"abcd") == []
    assert E.expected_rows(p, b"acd") == [[(0, 1), (1, 2), (2, 3), (0, 3)]]
    assert O.sub(p, b"<\\1>", b"abcd") == b"abcd"


@pytest.mark.parametrize("pat,repl", CASES)
@pytest.mark.parametrize("count", [0, 1, 3])
def test_rows_rebuild_the_oracles_sub(pat, repl, count):
    g = E.num_groups(pat)
    checked = 0
    for t in _texts(pat):
        try:
            want = O.sub(pat, repl, t, count)
            rows = E.expected_rows(pat, t, count, g)
        except O.ReferenceDoesNotTerminate:
            continue
        assert all(len(r) == g + 1 for r in rows)
        if count:
            assert len(rows) <= count
        assert E.sub_from_rows(repl, t, rows) == want, (pat, repl, count, t, rows)
        checked += 1
    assert checked >= 100
