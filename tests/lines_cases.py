"""The batches that the lines tests run, built from the piece length P of the testing hook (never a literal): the CPU
walk (tests/test_lines_host.py) and the kernels (tests/test_gpu_lines.py) take the same list."""
from __future__ import annotations

from typing import Dict, List

import numpy as np


def piece_length() -> int:
    import mojo_regex_amd as M
    return int(M.load_library().mrx_debug_lines_piece(-1))


def _filled(size: int, marks: Dict[int, bytes]) -> bytes:
    """`size` bytes without a separator, with the given bytes at the given positions."""
    t = bytearray((b"abcdefghij" * (size // 10 + 1))[:size])
    for at, what in marks.items():
        t[at:at + len(what)] = what
    assert len(t) == size
    return bytes(t)


def piece_edges(P: int) -> Dict[str, List[bytes]]:
    """One text of 3P + 5 bytes each: separators and carriage returns around the first piece edge."""
    size = 3 * P + 5
    return {
        "sep_at_P-1": [_filled(size, {P - 1: b"\n"})],
        "sep_at_P": [_filled(size, {P: b"\n"})],
        "sep_at_P+1": [_filled(size, {P + 1: b"\n"})],
        "sep_at_all_three": [_filled(size, {P - 1: b"\n\n\n"})],
        "cr_at_P-1_lf_at_P": [_filled(size, {P - 1: b"\r\n"})],
        "cr_at_2P-1_lf_at_2P_and_the_end": [_filled(size, {2 * P - 1: b"\r\n", size - 2: b"\r\n"})],
        "one_line_over_four_pieces": [_filled(size, {})],
        "all_separators": [b"\n" * size],
        "all_carriage_returns": [b"\r" * size],
        "cr_cr_lf_over_the_edge": [_filled(size, {P - 2: b"\r\r\n"}), _filled(size, {P - 1: b"\r\r\n"}), _filled(size, {P: b"\r\r\n"})],
        "cr_as_the_last_byte": [_filled(size, {100: b"\n", size - 1: b"\r"}), _filled(P, {P - 1: b"\r"}), b"\n"],
        "lf_as_the_last_byte_of_a_piece_sized_text": [_filled(P, {P - 1: b"\n"}), _filled(2 * P, {P - 1: b"\r", 2 * P - 1: b"\n"})],
    }


def output_alignment(P: int) -> Dict[str, List[bytes]]:
    """k single-byte lines in front of a line that runs over the piece edge: the first kept byte of the second piece
    lands on every residue of 16 in the output."""
    return {"%d_short_lines_first" % k: [b"x\n" * k + _filled(2 * P + 40 - 2 * k, {P + 300: b"\n", 2 * P: b"\r\n"})]
            for k in range(16)}


def empty_texts(P: int) -> Dict[str, List[bytes]]:
    return {
        "no_text": [],
        "one_empty_text": [b""],
        "only_empty_texts": [b""] * 5,
        "runs_of_empty_texts": [b"", b"", b"", b"a\nb", b"", b"", b"c", b"d\n", b"", b"\n", b"", b""],
        "empty_texts_around_long_ones": [b"", _filled(P + 7, {5: b"\n"}), b"", b"", _filled(2 * P, {P: b"\n"}), b""],
    }


def many_short_texts(P: int) -> Dict[str, List[bytes]]:
    rng = np.random.default_rng(20261020)
    al = np.frombuffer(b"\n\ra\nb", np.uint8)
    return {"300_texts_of_0_to_3_bytes": [al[rng.integers(0, len(al), size=int(rng.integers(0, 4)))].tobytes() for _ in range(300)]}


def log_texts(n: int, seed: int, longest: int = 200, n_long: int = 0, P: int = 0) -> List[bytes]:
    """Texts of several lines each over an alphabet with both line-end bytes, empty ones among them, and n_long of one to
    three pieces."""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(b"abcdefgh 0123456789\n\n\r\n", np.uint8)
    texts = [al[rng.integers(0, len(al), size=int(rng.integers(0, longest + 1)))].tobytes() for _ in range(n - n_long)]
    texts += [al[rng.integers(0, len(al), size=int(rng.integers(P, 3 * P + 1)))].tobytes() for _ in range(n_long)]
    texts[::11] = [b""] * len(texts[::11])
    order = rng.permutation(len(texts))
    return [texts[int(k)] for k in order]


def all_cases(P: int) -> Dict[str, List[bytes]]:
    out: Dict[str, List[bytes]] = {}
    for group in (piece_edges, output_alignment, empty_texts, many_short_texts):
        out.update(group(P))
    out["log_texts"] = log_texts(70, 7, n_long=3, P=P)
    return out
