"""The expansion of one two-word event record into spans (csrc/mrx_decode_bits.hpp, k_decode's lean pass) on the host,
through mrx_testing_decode_expand, against a reference that walks the 32 bytes of the pair one by one.

An event word covers 16 bytes: bit 2k = NEWSTART at byte k, bit 2k + 1 = EMIT at byte k (a match ends in front of it).
A legal record is one the scan can write: every NEWSTART of the record lies at or behind `start`, the start of the walk
alive at the pair's first byte (start <= pb wherever the record has a NEWSTART; the end-of-text record, whose start may
lie inside its pair, has none)."""
import itertools

import numpy as np

import mojo_regex_amd as M


def _reference(fe, fo, start, pb, fixed_len):
    """Vectorised over records: byte by byte, an EMIT closes the walk that is alive, then a NEWSTART opens one."""
    n = len(fe)
    cur = start.astype(np.int64).copy()
    counts = np.zeros(n, np.int32)
    spans = np.full((n, 32, 2), -99, np.int32)
    rows = np.arange(n)
    for k in range(32):
        word = (fe if k < 16 else fo).astype(np.int64) >> (2 * (k & 15))
        hit = (word & 2) != 0
        spans[rows[hit], counts[hit], 0] = (pb[hit] + k - fixed_len) if fixed_len else cur[hit]
        spans[rows[hit], counts[hit], 1] = pb[hit] + k
        counts += hit
        cur = np.where((word & 1) != 0, pb + k, cur)
    return counts, spans


def _expand(fe, fo, start, pb, fixed_len=0):
    n = len(fe)
    fe, fo = np.ascontiguousarray(fe, np.uint32), np.ascontiguousarray(fo, np.uint32)
    start, pb = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(pb, np.int32)
    counts = np.full(n, -1, np.int32)
    spans = np.full((n, 32, 2), -99, np.int32)
    rc = M.load_library().mrx_testing_decode_expand(n, fe.ctypes.data, fo.ctypes.data, start.ctypes.data, pb.ctypes.data,
                                                    fixed_len, counts.ctypes.data, spans.ctypes.data)
    assert rc == 0
    return counts, spans


def _check(fe, fo, start, pb, fixed_len=0):
    fe, fo = np.asarray(fe, np.uint32), np.asarray(fo, np.uint32)
    start = np.broadcast_to(np.asarray(start, np.int32), fe.shape).copy()
    pb = np.broadcast_to(np.asarray(pb, np.int32), fe.shape).copy()
    counts, spans = _expand(fe, fo, start, pb, fixed_len)
    want_counts, want_spans = _reference(fe, fo, start, pb, fixed_len)
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(spans, want_spans)       # (slots behind a record's count stay untouched: -99 on both sides)
    return counts, spans


def _masks(max_bits, odd):
    """Every word with at most max_bits bits set, each at bit 2k + odd of a byte k of the group."""
    out = [0]
    for r in range(1, max_bits + 1):
        for ks in itertools.combinations(range(16), r):
            out.append(sum(1 << (2 * k + odd) for k in ks))
    return np.array(out, np.uint32)


def test_every_word_with_at_most_three_emits_and_three_newstarts_in_either_group():
    """697 EMIT masks x 697 NEWSTART masks = 485 809 words, each as the even group in front of a probe word (EMIT at bytes
    0, 7 and 15, NEWSTART at byte 7: its starts come from the word under test) and as the odd group behind three probes
    (nothing; NEWSTART at byte 15; NEWSTART at bytes 0 and 9 with EMIT at 9)."""
    em, ns = _masks(3, 1), _masks(3, 0)
    assert len(em) == len(ns) == 697
    words = (em[:, None] | ns[None, :]).reshape(-1)
    probe_behind = np.uint32((2 << 0) | (2 << 14) | (1 << 14) | (2 << 30))
    for pb, start in ((0, 0), (32, 31), (992, 5)):
        _check(words, np.full_like(words, probe_behind), start, pb)
    for probe in (0, 1 << 30, (1 << 0) | (1 << 18) | (2 << 18)):
        _check(np.full_like(words, probe), words, 17, 64)


def test_random_legal_records():
    rng = np.random.default_rng(20260420)
    n = 6000
    fe = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    fo = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    thin = rng.integers(0, 1 << 32, (2, n), dtype=np.uint64).astype(np.uint32)
    fe[: n // 2] &= thin[0, : n // 2]                # half of them with a quarter of the bits
    fo[: n // 2] &= thin[1, : n // 2]
    pb = 32 * rng.integers(0, 32, n)
    start = (rng.integers(0, 1 << 30, n) % (pb + 1)).astype(np.int32)      # 0 .. pb
    counts, _ = _check(fe, fo, start, pb)
    assert counts.max() > 16 and counts.min() < 4
    # 16-byte records: pairs at any position, also in front of the text's first byte (no event before position 0)
    pb = rng.integers(-143, 65000, n)
    pb[: n // 3] = rng.integers(-143, 1, n // 3)          # (ragged batches: the even group up to 143 bytes in front)
    lo = np.clip(-pb, 0, 32)
    keep_e = ~((np.uint64(1) << (2 * np.minimum(lo, 16)).astype(np.uint64)) - np.uint64(1))
    keep_o = ~((np.uint64(1) << (2 * np.maximum(lo - 16, 0)).astype(np.uint64)) - np.uint64(1))
    start = (rng.integers(0, 1 << 30, n) % (np.maximum(pb, 0) + 1)).astype(np.int32)
    _check(fe & keep_e.astype(np.uint32), fo & keep_o.astype(np.uint32), start, pb)


def test_all_emit_word():
    """32 spans in one record: with a NEWSTART at every byte (the pattern [a-z]) and with none at all."""
    counts, spans = _check([0xFFFFFFFF, 0xAAAAAAAA], [0xFFFFFFFF, 0xAAAAAAAA], [95, 40], 96)
    assert counts.tolist() == [32, 32]
    assert spans[0, 0].tolist() == [95, 96] and spans[0, 31].tolist() == [126, 127]
    assert (spans[1, :, 0] == 40).all() and spans[1, :, 1].tolist() == list(range(96, 128))


def test_emit_at_byte_zero_takes_the_start_from_the_record():
    counts, spans = _check([2, 2 | 1, 2], [0, 0, 0], [3, 60, 0], [64, 64, 0])
    assert counts.tolist() == [1, 1, 1]
    assert spans[:, 0].tolist() == [[3, 64], [60, 64], [0, 0]]     # (a NEWSTART at the EMIT's own byte is not before it)


def test_end_of_text_record_whose_start_lies_inside_the_pair():
    """The scan's last record of a text: one EMIT bit, no NEWSTART, start anywhere up to the byte in front of it."""
    fe, fo, start, pb = [], [], [], []
    for k in range(32):
        for st in range(0, 32 + k):
            bit = 2 << (2 * (k & 15))
            fe.append(bit if k < 16 else 0)
            fo.append(bit if k >= 16 else 0)
            start.append(st)
            pb.append(32)
    counts, spans = _check(fe, fo, start, pb)
    assert (counts == 1).all() and np.array_equal(spans[:, 0, 0], np.array(start))


def test_emit_in_the_odd_group_with_the_last_newstart_in_the_even_group():
    fe = [1 << (2 * j) for j in range(16)] + [(1 << 4) | (1 << 20), 0]
    fo = [2 << (2 * k) for k in range(16)] + [2 << 6, 2 << 6]
    counts, spans = _check(fe, fo, 7, 128)
    assert counts.tolist() == [1] * 18
    assert spans[:16, 0, 0].tolist() == [128 + j for j in range(16)]
    assert spans[16, 0].tolist() == [128 + 10, 128 + 19] and spans[17, 0].tolist() == [7, 128 + 19]


def test_fixed_length_form():
    rng = np.random.default_rng(7)
    fe = rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32)
    fo = rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32)
    pb = 32 * rng.integers(1, 32, 2000)
    for fixed_len in (1, 5, 16):
        counts, spans = _check(fe, fo, 0, pb, fixed_len)
        k = int(np.argmax(counts))
        c = counts[k]
        assert c > 0 and np.array_equal(spans[k, :c, 1] - spans[k, :c, 0], np.full(c, fixed_len))


def test_arguments_and_listing():
    lib = M.load_library()
    assert lib.mrx_testing_decode_expand(1, None, None, None, None, 0, None, None) == -1
    assert lib.mrx_testing_decode_expand(0, None, None, None, None, 0, None, None) == 0
    one = np.zeros(64, np.int32)
    assert lib.mrx_testing_decode_expand(-1, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, 0,
                                         one.ctypes.data, one.ctypes.data) == -1
    assert lib.mrx_testing_decode_expand(1, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, -2,
                                         one.ctypes.data, one.ctypes.data) == -1
    for name in ("mrx_debug_decode_lean", "mrx_testing_decode_expand"):
        assert name in M.api.TESTING_SYMBOLS and hasattr(lib, name), name
