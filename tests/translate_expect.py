"""What translate and strip must give (include/mrx.h, "translate", "strip"), in plain Python: bytes.translate, the
squeeze rule of the contract, and bytes.strip / lstrip / rstrip."""
import numpy as np

IDENTITY = bytes(range(256))
LOWER = IDENTITY.lower()
UPPER = IDENTITY.upper()
PERMUTATION = bytes(np.random.default_rng(256).permutation(256).astype(np.uint8).tolist())   # the general table
TAB_TO_SPACE = IDENTITY.replace(b"\t", b" ")                                                 # a one-byte replacement
DELETE40 = bytes(range(ord("a"), ord("z") + 1)) + b"0123456789 \r\t_"
assert len(DELETE40) == 40 and sorted(PERMUTATION) == list(range(256))

# (table, delete, squeeze): the parameter sets of the tests
MAPS = (dict(), dict(table=LOWER), dict(table=UPPER), dict(table=PERMUTATION), dict(table=TAB_TO_SPACE))
PACKED = (dict(delete=b"\r"), dict(delete=b"\r\" e"), dict(delete=DELETE40), dict(squeeze=b" "), dict(squeeze=b" \t-ab"),
          dict(table=LOWER, delete=b"aeiou\r"), dict(table=TAB_TO_SPACE, squeeze=b" "), dict(table=PERMUTATION, delete=b"b \n"),
          dict(table=PERMUTATION, squeeze=PERMUTATION[32:33] + PERMUTATION[97:99]))
PARAMETER_SETS = MAPS + PACKED
STRIPS = (dict(), dict(left=False), dict(right=False), dict(chars=b"x"), dict(chars=b" \t\"'"), dict(chars=b"ab", right=False),
          dict(chars=bytes(range(48, 58)) + b"-+.", left=False), dict(chars=b""))


def translate(t: bytes, table=None, delete=b"", squeeze=b"") -> bytes:
    assert not (delete and squeeze)
    u = t.translate(table, delete)
    if not squeeze or not u:
        return u
    a = np.frombuffer(u, np.uint8)   # (the rule of the contract, byte k > 0 against byte k - 1, on the whole text at once)
    keep = np.ones(len(a), bool)
    keep[1:] = ~(np.isin(a[1:], np.frombuffer(squeeze, np.uint8)) & (a[1:] == a[:-1]))
    return a[keep].tobytes()


def strip(t: bytes, chars=None, left=True, right=True):
    """(start, end) of the stripped text inside t"""
    start = len(t) - len(t.lstrip(chars)) if left else 0
    end = start + len(t[start:].rstrip(chars)) if right else len(t)
    return start, end


def expected(texts, table=None, delete=b"", squeeze=b""):
    """(out_offsets int64[n + 1], data uint8[bytes], [bytes, longest]) of a batch"""
    outs = [translate(t, table, delete, squeeze) for t in texts]
    off = np.zeros(len(outs) + 1, np.int64)
    if outs:
        np.cumsum([len(u) for u in outs], out=off[1:])
    data = np.frombuffer(b"".join(outs), np.uint8)
    return off, data, [int(off[-1]), max((len(u) for u in outs), default=0)]


def strip_rows(texts, chars=None, left=True, right=True):
    """rows int32[n, 1, 2]"""
    return np.array([strip(t, chars, left, right) for t in texts], np.int32).reshape(len(texts), 1, 2)
