"""The batches that the translate and strip tests run, built from the piece length P of the testing hook (never a
literal): the CPU walk (tests/test_translate_host.py) and the kernels (tests/test_gpu_translate.py) take the same list.

Every parameter set of tests/translate_expect.py deletes or squeezes the space or the carriage return (most of them
both kinds), so every structural case exists once with each as its special byte `s`; 'X' and 'Q' are in no set, and the
case tables change 'X'."""
from __future__ import annotations

from typing import Dict, List

import numpy as np

SPECIALS = (b" ", b"\r")
ALPHABET = b"  \r\r\t\t-ab\"eXYzQ\n0aeiou  \r"


def piece_length() -> int:
    import mojo_regex_amd as M
    return int(M.load_library().mrx_debug_translate_piece(-1))


def _mixed(size: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    al = np.frombuffer(ALPHABET, np.uint8)
    # runs of one to four equal bytes: something to squeeze
    picks = al[rng.integers(0, len(al), size=size)]
    return np.repeat(picks, rng.integers(1, 5, size=size))[:size].tobytes()


def _at(size: int, marks: Dict[int, bytes], fill: bytes = b"X") -> bytes:
    """`size` bytes of `fill` with the given bytes at the given positions."""
    t = bytearray(fill * size)
    for at, what in marks.items():
        t[at:at + len(what)] = what
    assert len(t) == size
    return bytes(t)


def piece_edges(P: int) -> Dict[str, List[bytes]]:
    out: Dict[str, List[bytes]] = {
        "lengths_around_a_piece": [_mixed(P - 1, 1), _mixed(P, 2), _mixed(P + 1, 3), _mixed(2 * P + 3, 4)],
        "a_run_of_a_byte_in_no_set": [b"Q" * 40, _at(2 * P, {P - 3: b"QQQQQQ", 14: b"QQQQ", 1022: b"QQQQ"})],
        "a_run_only_behind_the_map": [b"\t \t \t\t  X\t", _at(P + 20, {P - 2: b"\t \t ", 15: b" \t"})],
    }
    for s in SPECIALS:
        tag = "space" if s == b" " else "cr"
        out.update({
            "kept_run_over_the_piece_edge_" + tag: [s * (P - 8) + b"X" * 16 + s * P, s * (P - 1) + b"XY" + s * 7],
            "a_piece_of_dropped_bytes_between_two_kept_" + tag: [b"X" * P + s * P + b"Y" * P, b"Q" + s * (2 * P - 1) + b"Q"],
            "a_text_of_dropped_bytes_" + tag: [s * (P + 17), b"X", s * 5, s, b"Y" * 17, s * 16, s * (2 * P)],
            "runs_over_block_round_and_piece_edges_" + tag: [
                _at(2 * P + 9, {14: s * 4, 1022: s * 4, P - 2: s * 4, 2 * P - 1: s * 2}),
                _at(P + 40, {15: s, 16: s, 31: s * 2, 1023: s, 1024: s, P - 1: s, P: s}),
                _at(P + 40, {16: s * 2, 14: s, 1024: s * 3, P: s * 16}),
                _at(3 * P, {0: s * (2 * P + 1)})],
            "a_text_begins_with_the_last_byte_of_the_text_in_front_" + tag: [b"X" + s * 3, s * 3 + b"X", s, s, s + b"X", s * 16, s * 17, s],
        })
    return out


def output_alignment(P: int) -> Dict[str, List[bytes]]:
    """k kept bytes in front of a long text: its first output byte, and those of its pieces, land on every residue of
    16."""
    return {"%d_kept_bytes_first" % k: [b"Y" * k, _mixed(2 * P + 40 - k, 40 + k)] for k in range(16)}


def empty_texts(P: int) -> Dict[str, List[bytes]]:
    return {
        "no_text": [],
        "one_empty_text": [b""],
        "only_empty_texts": [b""] * 5,
        "runs_of_empty_texts": [b"", b"", b"", b"a  b", b"", b"", b"\r", b" d ", b"", b" ", b"", b""],
        "empty_texts_around_long_ones": [b"", _mixed(P + 7, 5), b"", b"", _mixed(2 * P, 6), b""],
    }


def many_short_texts(P: int) -> Dict[str, List[bytes]]:
    rng = np.random.default_rng(20261020)
    return {"300_texts_of_0_to_20_bytes": [_mixed(int(rng.integers(0, 21)), 100 + k) for k in range(300)]}


def mixed_texts(n: int, seed: int, longest: int = 200, n_long: int = 0, P: int = 0) -> List[bytes]:
    """Texts over the alphabet of the sets, empty ones among them, and n_long of one to three pieces."""
    rng = np.random.default_rng(seed)
    texts = [_mixed(int(rng.integers(0, longest + 1)), seed * 1000 + k) for k in range(n - n_long)]
    texts += [_mixed(int(rng.integers(P, 3 * P + 1)), seed * 1000 + n + k) for k in range(n_long)]
    texts[::11] = [b""] * len(texts[::11])
    order = rng.permutation(len(texts))
    return [texts[int(k)] for k in order]


def all_cases(P: int) -> Dict[str, List[bytes]]:
    out: Dict[str, List[bytes]] = {}
    for group in (piece_edges, output_alignment, empty_texts, many_short_texts):
        out.update(group(P))
    out["mixed_texts"] = mixed_texts(70, 7, n_long=3, P=P)
    return out


def strip_texts(s: bytes, other: bytes = b"Z") -> List[bytes]:
    """Texts for a strip whose set holds the byte `s` and not `other`: set bytes alone at the lengths around a 16-byte
    word, at one end only, at none, and the one other byte at every position of a word whatever the text's alignment."""
    texts = [s * k for k in (0, 1, 15, 16, 17, 40)]
    texts += [s * 3 + other * 5, other * 5 + s * 3, other * 7, other, s * 20 + other, other + s * 20, s + other + s]
    texts += [s * k + other + s * (33 - k) for k in range(34)]
    texts += [s * k + other * 2 + s * 3 + other + s * (18 - k) for k in range(19)]
    texts += [b"", s * 2 + other * 40 + s * 2, other * 16, s * 16 + other * 16 + s * 16]
    return texts
