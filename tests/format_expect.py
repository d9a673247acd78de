"""What format (include/mrx.h, "format") has to give, in plain Python: a number cell is b"%<spec>" % value, a FIXED cell
only where the exact rule answers -- restated here in Python integers -- a record is the template with every \\1..\\9
replaced by the row's cell, and the row status is that of the lowest-numbered referenced column whose cell was not
written.  Host-only; shared by the host tests and the GPU tests."""
import struct

import numpy as np

OK, EMPTY, MALFORMED, RANGE = 0, 1, 2, 3
TEXT, INT10, INT16, FIXED = 0, 1, 2, 3
LIMIT = 10 ** 19
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def spec_kind(spec):
    """(kind, arg) of "d", ".Kd", "x", ".Kx", ".Pf"."""
    kind = {"d": INT10, "x": INT16, "f": FIXED}[spec[-1]]
    return kind, (int(spec[1:-1]) if len(spec) > 1 else 0)


def float_bits(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]


def bits_float(w):
    return struct.unpack("<d", struct.pack("<q", w))[0]


def fixed_scaled(bits, P):
    """N = round_half_even(|v| * 10^P) from a double's bits by the rule of include/mrx.h, or None when it is not below
    10^19 (NaN and the infinities among them).  Integers only."""
    bits &= (1 << 64) - 1
    E, frac = (bits >> 52) & 0x7FF, bits & ((1 << 52) - 1)
    if E == 0x7FF:
        return None
    m, e = (frac | (1 << 52), E - 1075) if E else (frac, -1074)
    prod = m * 10 ** P
    if e >= 0:
        q = prod << e
    else:
        q, rem, half = prod >> -e, prod & ((1 << -e) - 1), 1 << (-e - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
    return q if q < LIMIT else None


def cell(spec, value):
    """The cell of one value: bytes, or None where format prints nothing (a FIXED value the rule does not answer).  value
    is an int for "d" / "x" and a float for ".Pf"."""
    kind, arg = spec_kind(spec)
    if kind != FIXED:
        return (b"%" + spec.encode()) % int(value)
    bits = float_bits(float(value))
    N = fixed_scaled(bits, arg)
    if N is None:
        return None
    digits = b"%0*d" % (arg + 1, N)
    body = digits[:len(digits) - arg] + (b"." + digits[len(digits) - arg:] if arg else b"")
    return (b"-" if bits < 0 else b"") + body


def cell_of_word(kind, arg, word):
    """cell() from what the C side takes: a kind, its arg and the value's 64-bit word (an int64, a double's bits)."""
    if kind == FIXED:
        return cell(".%df" % arg, bits_float(word))
    return cell(".%d%s" % (arg, "d" if kind == INT10 else "x"), word)


def parse_template(template):
    """[(literal bytes | column number)] by sub's grammar: only \\1..\\9 are references."""
    out, lit, i = [], b"", 0
    while i < len(template):
        if template[i] == 0x5C and i + 1 < len(template) and 0x31 <= template[i + 1] <= 0x39:
            if lit:
                out.append(lit)
            out.append(template[i + 1] - 0x30)
            lit, i = b"", i + 2
        else:
            lit += template[i:i + 1]
            i += 1
    if lit:
        out.append(lit)
    return out


def records(template, columns):
    """(records, row status) of a call.  A column is a list of bytes (a text column) or (values, spec) or (values, spec,
    status): values are ints, or floats for ".Pf"; a status byte that is not OK prints nothing."""
    segs = parse_template(template)
    cols = []
    for c in columns:
        if isinstance(c, tuple):
            values, spec = c[0], c[1]
            status = c[2] if len(c) > 2 and c[2] is not None else [OK] * len(values)
            col = []
            for v, s in zip(values, status):
                b = cell(spec, v) if s == OK else None
                col.append((b, OK) if b is not None else (None, RANGE if s == OK else int(s)))
            cols.append(col)
        else:
            cols.append([(bytes(t), OK) for t in c])
    n = len(cols[0])
    assert all(len(c) == n for c in cols)
    used = sorted({s for s in segs if isinstance(s, int) and s <= len(cols)})
    recs, status = [], np.zeros(n, np.uint8)
    for r in range(n):
        recs.append(b"".join(s if isinstance(s, bytes) else (cols[s - 1][r][0] or b"") if s <= len(cols) else b"" for s in segs))
        status[r] = next((cols[j - 1][r][1] for j in used if cols[j - 1][r][0] is None), OK)
    return recs, status


def packed(recs):
    """(data bytes, offsets int64[n + 1]) of records back to back."""
    off = np.zeros(len(recs) + 1, np.int64)
    if recs:
        np.cumsum([len(r) for r in recs], out=off[1:])
    return b"".join(recs), off


# ---- the edge values ---------------------------------------------------------------------------------------------------

INT_SPECS = ("d", ".0d", ".1d", ".19d", ".20d", "x", ".0x", ".1x", ".19x", ".20x", ".7d", ".3x")
FIXED_PRECISIONS = tuple(range(10))


def int_edges():
    """Every power of ten +- 1 up to 10^18, the ends of int64, the hex edges."""
    vals = {0, 1, -1, 9, 10, -9, -10, 15, 16, 17, 255, 256, -255, -256, INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1}
    for k in range(19):
        for d in (-1, 0, 1):
            vals |= {10 ** k + d, -(10 ** k + d)}
    for k in range(0, 63, 4):
        for d in (-1, 0, 1):
            vals |= {(1 << k) + d, -((1 << k) + d)}
    vals |= {0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x100000000, 0x123456789ABCDEF, -0xFEDCBA987654321, 99999999, 100000000,
             9999999999999999, 10000000000000000}
    return sorted(v for v in vals if INT64_MIN <= v <= INT64_MAX)


def _neighbours(v):
    b = float_bits(v)
    return [bits_float(b - 1), v, bits_float(b + 1)]


def fixed_edges():
    """Doubles for every P: dyadic ties, signed zeros, denormals, 2^53, the doubles around 10^19 / 10^P, NaN, the
    infinities."""
    vals = [0.0, -0.0, 0.5, -0.5, 1.5, 2.5, -2.5, 0.125, 0.375, -0.04, 0.05, 0.25, 0.75, 1.0, -1.0, 9.5, 99.5, 999.5, 0.1, 0.2,
            0.3, 1e-9, 5e-10, 4.999e-10, 5e-324, -5e-324, 2.2250738585072014e-308, 2.0 ** 53, 2.0 ** 53 + 2, -(2.0 ** 53),
            2.0 ** 63, 2.0 ** 64, 1e18, 1e19, 1e22, 1e300, 1.7976931348623157e308, float("nan"), float("inf"), float("-inf"),
            123456.789, -987654.321, 3.141592653589793, 0.999999999, 0.9999999995, 9.9999999995, 1234567890.1234567]
    for k in range(1, 12):
        vals += [(2 * j + 1) / 2.0 ** k for j in range(0, 6)]        # ties of P < k, exact at P >= k
        vals += [-(2 * j + 1) / 2.0 ** k for j in range(0, 3)]
    for P in FIXED_PRECISIONS:
        for v in (10.0 ** (19 - P), float(10 ** 19 - 1) / 10 ** P, float(10 ** (19 - P)) - 0.5 / 10 ** P):
            vals += _neighbours(v) + _neighbours(-v)
    return vals


def fixed_random(n, seed):
    """n doubles: random bit patterns, scaled decimals from 10^-12 to 10^19 and dyadic ties."""
    rng = np.random.default_rng(seed)
    third = n // 3
    raw = rng.integers(0, 1 << 63, size=third, dtype=np.int64) * rng.choice(np.array([1, -1], np.int64), size=third)
    out = raw.view(np.float64).tolist()
    mant = rng.integers(0, 10 ** 7, size=third).astype(np.float64)
    out += (mant * 10.0 ** rng.integers(-12, 13, size=third) * rng.choice([1.0, -1.0], size=third)).tolist()
    rest = n - 2 * third
    out += ((2 * rng.integers(0, 1 << 20, size=rest) + 1) / 2.0 ** rng.integers(1, 30, size=rest)).tolist()
    return out
