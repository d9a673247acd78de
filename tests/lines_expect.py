"""What lines computes (include/mrx.h, "lines"), in plain Python: the expectation of the host and the GPU tests."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

OPTION_SETS = (
    dict(),
    dict(keepends=True),
    dict(crlf=True),
    dict(partial=False),
)


def lines(t: bytes, sep: bytes = b"\n", keepends: bool = False, crlf: bool = False, partial: bool = True) -> Tuple[List[bytes], int]:
    """(the lines of one text, the byte count of its unterminated tail)."""
    pieces = t.split(sep)
    tail = pieces.pop()   # what follows the last separator: nothing, or the unterminated tail
    out = []
    for p in pieces:
        if crlf and p.endswith(b"\r"):
            p = p[:-1]
        out.append(p + sep if keepends else p)
    if partial and tail:
        out.append(tail)
    return out, len(tail)


def expected(texts: Sequence[bytes], **opts):
    """(line_prefix int64[n + 1], owner int64[lines], out_offsets int64[lines + 1], out_data uint8[bytes], totals
    [lines, bytes, longest line, tail of the last text]) for a batch."""
    prefix, owner, off, data, tail = [0], [], [0], [], 0
    for i, t in enumerate(texts):
        ls, tail = lines(t, **opts)
        for l in ls:
            owner.append(i)
            data.append(l)
            off.append(off[-1] + len(l))
        prefix.append(len(owner))
    raw = b"".join(data)
    longest = max((len(l) for l in data), default=0)
    return (np.array(prefix, np.int64), np.array(owner, np.int64), np.array(off, np.int64),
            np.frombuffer(raw, np.uint8).copy(), [len(owner), len(raw), longest, tail if len(texts) else 0])
