"""The expected (status, value) of a piece under the number grammars of include/mrx.h ("numbers"), from Python alone: a
regex fullmatch decides the grammar, int(t) and int(t, 16) give the integers with the int64 range test, and the exact
float rule -- d, the integer that all mantissa digits write, and q, the exponent minus the number of fraction digits,
answered when d <= 2^53 and |q| <= 22 once d's factors of ten are moved into q -- is done in Python integers.

Every value is the row's 64 bits as a signed int64: the integer itself, or the bits of the double, so that the sign
of a zero is compared too.  Host-only: neither torch nor the product library.
"""
from __future__ import annotations

import re
import struct
from typing import List, Sequence, Tuple

import numpy as np

OK, EMPTY, MALFORMED, RANGE = 0, 1, 2, 3
KINDS = ("int", "hex", "float")

GRAMMAR = {
    "int": re.compile(rb"[+-]?[0-9]+"),
    "hex": re.compile(rb"[+-]?(0[xX])?[0-9a-fA-F]+"),
    "float": re.compile(rb"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?"),
}
# the float grammar once more, with its parts named (used only on pieces that GRAMMAR["float"] has accepted)
_FLOAT_PARTS = re.compile(rb"([+-]?)(?:([0-9]+)\.?([0-9]*)|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?")


def float_bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def fill_word(kind: str, fill) -> int:
    """What a row that is not a number holds: `fill` itself, for "float" the bits of float(fill)."""
    return float_bits(float(fill)) if kind == "float" else int(fill)


def exact_float(piece: bytes):
    """The float rule on a piece of the float grammar: the double, or None where the rule does not answer."""
    sign, ip, fp, only_fp, exp = _FLOAT_PARTS.fullmatch(piece).groups()
    digits = (ip or b"") + (fp or b"") + (only_fp or b"")
    nfrac = len(fp or b"") + len(only_fp or b"")
    d, q = int(digits), (int(exp) if exp else 0) - nfrac
    while d and d % 10 == 0:
        d, q = d // 10, q + 1
    if d == 0:
        v = 0.0
    elif d <= 2 ** 53 and -22 <= q <= 22:
        v = float(d) * float(10 ** q) if q >= 0 else float(d) / float(10 ** -q)   # one IEEE operation on exact operands
    else:
        return None
    return -v if sign == b"-" else v


def expect(piece: bytes, kind: str, fill=0) -> Tuple[int, int]:
    """(status, the row's 64 bits as an int64)."""
    word = fill_word(kind, fill)
    if len(piece) == 0:
        return EMPTY, word
    if not GRAMMAR[kind].fullmatch(piece):
        return MALFORMED, word
    if kind == "float":
        v = exact_float(piece)
        return (RANGE, word) if v is None else (OK, float_bits(v))
    v = int(piece.decode("ascii"), 16 if kind == "hex" else 10)
    return (OK, v) if -(1 << 63) <= v < (1 << 63) else (RANGE, word)


def expect_many(pieces: Sequence[bytes], kind: str, fill=0) -> Tuple[np.ndarray, np.ndarray]:
    """(status uint8[m], values int64[m]) of the pieces."""
    got = [expect(p, kind, fill) for p in pieces]
    return np.array([s for s, _ in got], dtype=np.uint8), np.array([v for _, v in got], dtype=np.int64)


def python_value(piece: bytes, kind: str):
    """What the list forms return for a piece: int, float or None."""
    st, v = expect(piece, kind)
    if st != OK:
        return None
    return struct.unpack("<d", struct.pack("<q", v))[0] if kind == "float" else v


def clamp_piece(text: bytes, s: int, e: int) -> bytes:
    """The piece of `text` under the pair (s, e), clamped as mrx_gather_spans_dev clamps it."""
    s2 = min(max(int(s), 0), len(text))
    return text[s2:min(max(int(e), s2), len(text))]


# The listed edges: piece -> the status under "int", "hex" and "float", worked out by hand from the grammar and the rules.
LISTED = {
    b"": (EMPTY, EMPTY, EMPTY),
    b"+": (MALFORMED, MALFORMED, MALFORMED),
    b"-": (MALFORMED, MALFORMED, MALFORMED),
    b"-0": (OK, OK, OK),
    b"9223372036854775807": (OK, RANGE, RANGE),              # 2^63 - 1; as hex 19 digits; as a float d > 2^53
    b"9223372036854775808": (RANGE, RANGE, RANGE),
    b"-9223372036854775808": (OK, RANGE, RANGE),
    b"-9223372036854775809": (RANGE, RANGE, RANGE),
    b"0" * 100 + b"1": (OK, OK, OK),
    b"0x": (MALFORMED, MALFORMED, MALFORMED),
    b"0X1f": (MALFORMED, OK, MALFORMED),
    b"-0xff": (MALFORMED, OK, MALFORMED),
    b"7fffffffffffffff": (MALFORMED, OK, MALFORMED),         # 16 hex digits
    b"ffffffffffffffff": (MALFORMED, RANGE, MALFORMED),      # ... out of range, not -1
    b"8000000000000000": (OK, RANGE, OK),                    # decimal 8e15; hex 2^63
    b"-8000000000000000": (OK, OK, OK),                      # hex -2^63
    b"10000000000000000": (OK, RANGE, OK),                   # 17 hex digits
    b".": (MALFORMED, MALFORMED, MALFORMED),
    b"1.": (MALFORMED, MALFORMED, OK),
    b".5": (MALFORMED, MALFORMED, OK),
    b"1e22": (MALFORMED, OK, OK),                            # (hex digits all four)
    b"1e23": (MALFORMED, OK, RANGE),
    b"1e-22": (MALFORMED, MALFORMED, OK),
    b"123e-25": (MALFORMED, MALFORMED, RANGE),
    b"9007199254740992": (OK, RANGE, OK),                    # 2^53
    b"9007199254740993": (OK, RANGE, RANGE),
    b"1.5" + b"0" * 22: (MALFORMED, MALFORMED, OK),
    b"-0.0e999": (MALFORMED, MALFORMED, OK),
    b"1e" + b"9" * 20: (MALFORMED, RANGE, RANGE),
    b"1_0": (MALFORMED, MALFORMED, MALFORMED),
    b"inf": (MALFORMED, MALFORMED, MALFORMED),
    b"nan": (MALFORMED, MALFORMED, MALFORMED),
    b" 1": (MALFORMED, MALFORMED, MALFORMED),
    b"1\x002": (MALFORMED, MALFORMED, MALFORMED),
}


def edge_pieces() -> List[bytes]:
    """About 300 pieces: the listed edges; for every length 0..40 a decimal, a signed decimal, a hex and a float piece
    (so pieces end at byte 15, 16, 17, 31, 32 and 33 of their windows, and integers pass 2^63 and floats 2^53 on the
    way); near misses of each grammar; short random pieces over the grammars' alphabet."""
    rng = np.random.default_rng(20261019)

    def run(alphabet: bytes, k: int) -> bytes:
        a = np.frombuffer(alphabet, dtype=np.uint8)
        return a[rng.integers(0, len(a), size=k)].tobytes()

    out = list(LISTED)
    for k in range(41):
        out.append(run(b"0123456789", k))
        out.append((b"-" if k % 2 else b"+") + run(b"0123456789", k - 1) if k else b"")
        out.append((b"0x" if k > 2 and k % 3 == 0 else b"") + run(b"0123456789abcdefABCDEF", k - 2 if k > 2 and k % 3 == 0 else k))
        if k >= 2:
            at = int(rng.integers(0, k))
            body = run(b"0123456789", k - 1)
            out.append(body[:at] + b"." + body[at:])
        else:
            out.append(run(b"0123456789.", k))
    out += [b"+0", b"00", b"0x0", b"+0x10", b"0xx1", b"00x1", b"x1", b"0xg", b"1f", b"-ff", b"1.e5", b".e5", b"1e", b"1e+",
            b"1e+5", b"1E-5", b"1.5.2", b"1e5e5", b"--1", b"+-1", b"1-", b"e5", b"1.5e", b"15e-1", b"0.1", b"0.000001",
            b"123.456", b"-.5", b"+.5e-3", b"0e99999999999999999999", b"1e-99999999999999999999", b"-inf", b"1 ", b"1\n",
            b"\x00", b"12\x00", b"9007199254740992e22", b"9007199254740992e23", b"15" + b"0" * 22, b"15" + b"0" * 23,
            b"0." + b"0" * 30 + b"1", b"0." + b"0" * 21 + b"1", b"0" * 50 + b"." + b"0" * 50, b"-" + b"0" * 40,
            b"7" * 100, b"7" * 100 + b"x", b"-" + b"7" * 64 + b"_" + b"7" * 40, b"1." + b"3" * 70, b"3" * 70 + b"e5",
            b"3" * 70 + b".5e", b"f" * 20 + b"1" * 50, b"f" * 20 + b"1" * 50 + b"g",
            b"18446744073709551615", b"18446744073709551616", b"-8000000000000001", b"0xffffffffffffffff", b"123456789e-9"]
    while len(out) < 300:
        out.append(run(b"0123456789abcdefxX+-_ .eE", int(rng.integers(1, 12))))
    return out
