"""The _known_dev contract of include/mrx.h: "upper bounds are fine, neither may be too small".

Every mrx_*_known_dev entry point is reached through its public Python method on DeviceBatch.csr_known batches -- the
corpus as CSR at shifts 0, 1, 7 and 15, the shifted ones inside a larger buffer whose other bytes are the corpus's own --
with every pair of an end_offset and a max_len from the lists below: exact, barely loose, loose by a few KiB, several times
too large, and just above every limit with which the entry point's host code compares the longest or the mean text.
Every run must take the _known_dev entry (a spy on DeviceBatch._entry_points), equal the host expectation, and equal bit
for bit the run on the same texts without bounds; the bounds that a result carries on must be true.  No bound below the
real value is ever passed: that is outside the contract.

Two corpora: chain_cases.BASE, whose longest text (20000 bytes) lies above every limit but two, and chain_cases.SHORT,
the same texts without the four long ones (longest: 215 bytes), for which every limit is a legal upper bound."""
import os
import re
from contextlib import contextmanager

import numpy as np
import pytest

import chain_cases as CC
import layouts as LY
import mojo_regex_amd as M
from test_gpu_chains import expect_equal, expect_same_bits, expectation, handles, restrict, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = (0,) + LY.CSR_SHIFTS
CORPORA = {"base": CC.BASE, "short": CC.SHORT}
CONSUMER = {c.name: c for c in CC.CONSUMERS}

# The limits with which the host code compares max_text_len (the value just above each is passed where it is a legal
# bound).  The core's limits are named by function and constant (mrx_kernels.hip, mrx_sub.hip, mrx_capall.hip); line
# numbers elsewhere are those of mojo_regex_amd/csrc at the time of writing.
FINDALL_MAX = (
    1024,     # mrx_stream_bits.hip:425   stream_bits_eligible: max_len > 1024 (fixed pitch only; a CSR batch must not care)
    2048,     # pieces_prepare            the piece size C is at least 2048, C >= max_len cuts nothing
    4095,     # pieces_prepare            max_len < 4096, nothing long enough to cut
    65300,    # kRec32MaxLen              FindallJob's rec32 = max_text <= kRec32MaxLen: 16-bit positions in the event records
)             # (FindallJob's dyn: 1 << kDynShift and kStreamMaxText = 1 << 26 lie above 65537 and size scratch)
SUB_MAX = FINDALL_MAX + (
    2048,     # sub_chain_from_spans' and capall_from_spans' tile: the group-template forms take 2048 or 4096 positions
    4096,     # sub_chain_from_spans, capall_from_spans: max_len > 4096 is beyond the tile, the generic form
)
SET_SUB_MAX = FINDALL_MAX + (
    1472,     # mrx_set.hip:1093          the window W = min(kSetSubMaxW = 1536, longest + 1 rounded up to 64)
)
FILTER_MAX = (
    4096,     # mrx_filter.hip:55/161     kFilterTextMax: the text form of the byte mover up to here, the block form above
    4095,     # pieces_prepare            the search in front of it, as findall
)
MOVER_MAX = (4096,)   # mrx_filter.hip:161 alone: dict filter (mrx_lookup.hip:276), take (mrx_sort.hip:384), distinct (mrx_distinct.hip:331)
SORT_MAX = (
    216, 224,  # mrx_sort.hip:314/327     a radix pass and the last word of a round: d + 8 >= known_max, multiples of 8
)
NO_MAX = ()   # kw_*: mrx_keywords.hip:245 reads known_max and uses the byte count alone (kw_piece_rule); lines, translate
#               and strip: "max_text_len is not used" (include/mrx.h); fields routes by end_offset / n, below
# The limits on end_offset / n: mrx_fields_bits.hpp:85-87, the lanes that share a text by the mean length
FIELDS_MEAN = (96, 768, 16384)


class Row:
    def __init__(self, stem, consumers, max_limits, mean_limits=()):
        self.stem, self.consumers, self.max_limits, self.mean_limits = stem, consumers, max_limits, mean_limits


ROWS = {
    "mrx_findall_known_dev": Row("mrx_findall", ("findall_stream", "findall_step", "findall_groups"), FINDALL_MAX),
    "mrx_sub_known_dev": Row("mrx_sub", ("sub_dev_stream", "sub_dev_groups"), SUB_MAX),
    "mrx_set_findall_known_dev": Row("mrx_set_findall", ("set_findall",), FINDALL_MAX),
    "mrx_set_sub_known_dev": Row("mrx_set_sub", ("set_sub",), SET_SUB_MAX),
    "mrx_filter_known_dev": Row("mrx_filter", ("filter",), FILTER_MAX),
    "mrx_set_filter_known_dev": Row("mrx_set_filter", ("set_filter",), FILTER_MAX),
    "mrx_extract_known_dev": Row("mrx_extract", ("extract",), FINDALL_MAX),
    "mrx_distinct_known_dev": Row("mrx_distinct", ("distinct",), MOVER_MAX),
    "mrx_dict_filter_known_dev": Row("mrx_dict_filter", ("dict_filter",), MOVER_MAX),
    "mrx_sort_known_dev": Row("mrx_sort", ("argsort",), SORT_MAX),
    "mrx_take_known_dev": Row("mrx_take", ("take",), MOVER_MAX),
    "mrx_kw_findall_known_dev": Row("mrx_kw_findall", ("kw_findall",), NO_MAX),
    "mrx_kw_filter_known_dev": Row("mrx_kw_filter", ("kw_filter",), MOVER_MAX),
    "mrx_kw_leftmost_known_dev": Row("mrx_kw_leftmost", ("kw_leftmost",), NO_MAX),
    "mrx_kw_sub_known_dev": Row("mrx_kw_sub", ("kw_sub",), NO_MAX),
    "mrx_lines_known_dev": Row("mrx_lines", ("lines",), NO_MAX),
    "mrx_fields_known_dev": Row("mrx_fields", ("fields_ws", "fields_delim"), NO_MAX, FIELDS_MEAN),
    "mrx_translate_known_dev": Row("mrx_translate", ("upper", "translate_delete"), NO_MAX),
    "mrx_strip_known_dev": Row("mrx_strip", ("strip",), NO_MAX),
}
# the entry points whose bounds choose the kernel: a loose bound must reach another one than the exact bound did
MUST_DIFFER = ("mrx_filter_known_dev", "mrx_dict_filter_known_dev", "mrx_kw_filter_known_dev", "mrx_take_known_dev",
               "mrx_fields_known_dev")
REACHED = {}    # (entry, "exact" | "loose") -> the kernels (and lanes per text) that the short corpus at shift 0 reached
DONE = set()
_CASES = {}


def test_the_table_covers_the_header():
    hdr = open(os.path.join(ROOT, "include", "mrx.h")).read()
    declared = set(re.findall(r"\b(mrx_\w+_known_dev)\b", hdr))
    assert len(declared) >= 19
    assert declared == set(ROWS), (sorted(declared - set(ROWS)), sorted(set(ROWS) - declared))
    lib = M.load_library()
    for entry, row in ROWS.items():
        assert entry == row.stem + "_known_dev" and hasattr(lib, entry) and hasattr(lib, row.stem + "_dev")
        assert all(name in CONSUMER for name in row.consumers)


def case(corpus, shift):
    """(texts, data and offsets on the device, exact end_offset, exact max_len)."""
    key = (corpus, shift)
    if key not in _CASES:
        H = handles()
        texts = CORPORA[corpus]
        own = b"".join(texts)
        if shift == 0:
            lay = LY.csr_packed(texts)
        else:   # the poison: the corpus's own bytes, so that a kernel that reads past a text finds more of the same
            lay = LY.csr_shifted(texts, shift, lambda i, t, k: (own[max(i, 0) * 37 % len(own):] + own)[:k])
        lay.check()
        _CASES[key] = (texts, H.dev(lay.buf), H.dev(lay.offsets), int(lay.offsets[-1]), max(len(t) for t in texts))
    return _CASES[key]


def bound_pairs(row, n, end, longest):
    ends = [end, end + 1, end + 12345, 4 * end + 4096 * n]
    ends += [n * m + n for m in row.mean_limits if n * m + n > end]
    maxs = [longest, longest + 1] + [m + 1 for m in row.max_limits if m + 1 > longest] + [65537]
    assert min(ends) >= end and min(maxs) >= longest      # never below the real value
    assert max(maxs) <= 65537
    return [(e, m) for e in dict.fromkeys(ends) for m in dict.fromkeys(maxs)]


@contextmanager
def only(stem, which):
    """The stem's calls must take the entry `which` ("known" or "dev"); yields the list of the calls that did."""
    lib = M.load_library()
    fns = (getattr(lib, stem + "_dev"), getattr(lib, stem + "_known_dev"), getattr(lib, stem + "_strided_dev"))
    calls = []

    def spy(fn):
        def call(*args):
            calls.append(stem)
            return fn(*args)
        return call

    def never(*args):
        raise AssertionError("%s took the %s entry point" % (stem, "one that reads the bounds back" if which == "known" else "_known_dev"))

    had = M.DeviceBatch._entry_points.get(stem)
    M.DeviceBatch._entry_points[stem] = (never, spy(fns[1]), fns[2]) if which == "known" else (spy(fns[0]), never, fns[2])
    try:
        yield calls
    finally:
        if had is None:
            del M.DeviceBatch._entry_points[stem]
        else:
            M.DeviceBatch._entry_points[stem] = had


def carried_bounds_are_true(raw, what):
    for o in raw if isinstance(raw, (tuple, list)) else (raw,):
        if isinstance(o, M.DeviceBatch) and o.offsets is not None and o._max_len is not None:
            off = o.offsets.cpu().numpy()
            assert o._end_offset >= int(off[-1]) and o._max_len >= int(np.diff(off).max(initial=0)), (
                what, o._end_offset, int(off[-1]), o._max_len, int(np.diff(off).max(initial=0)))


def reached(entry):
    lib = M.load_library()
    name = lib.mrx_last_kernel_name().decode()
    if entry == "mrx_fields_known_dev":
        name += "/%d lanes per text" % lib.mrx_debug_fields_last_group()
    if entry == "mrx_sort_known_dev":
        name += "/%d rounds" % lib.mrx_debug_sort_rounds()
    return name


@pytest.mark.parametrize("entry,name", [(e, c) for e, row in ROWS.items() for c in row.consumers])
def test_loose_bounds_change_no_result(entry, name):
    H = handles()
    row, c = ROWS[entry], CONSUMER[name]
    for corpus in CORPORA:
        for shift in SHIFTS:
            texts, data, offsets, end, longest = case(corpus, shift)
            what = "%s via %s, %s corpus, shift %d" % (entry, name, corpus, shift)
            with only(row.stem, "dev") as calls:
                ref = to_np(c.device(H, M.DeviceBatch(data, offsets)))
            assert calls, what
            if c.limit:
                keep = [i for i, t in enumerate(texts) if len(t) <= c.limit]
                expect_equal(restrict(ref, keep), expectation(c, [texts[i] for i in keep]), what, [texts[i] for i in keep])
            else:
                expect_equal(ref, expectation(c, texts), what, texts)
            for e, m in bound_pairs(row, len(texts), end, longest):
                where = "%s, end_offset %d (exact %d), max_len %d (exact %d)" % (what, e, end, m, longest)
                with only(row.stem, "known") as calls:
                    raw = c.device(H, M.DeviceBatch.csr_known(data, offsets, e, m))
                assert calls, where
                if corpus == "short" and shift == 0:
                    kind = "exact" if (e, m) == (end, longest) else "loose"
                    REACHED.setdefault((entry, kind), set()).add(reached(entry))
                carried_bounds_are_true(raw, where)
                expect_same_bits(to_np(raw), ref, where, texts)
    DONE.add((entry, name))


def test_loose_bounds_reached_other_kernels():
    """Runs last: where the bounds choose the kernel, or the lanes that share a text, a loose pair chose another one than
    the exact pair did.  A loose bound that changes nothing tests nothing."""
    handles()
    for entry in MUST_DIFFER:          # (when run on its own: the runs that record the kernels)
        for name in ROWS[entry].consumers:
            if (entry, name) not in DONE:
                test_loose_bounds_change_no_result(entry, name)
    same = [e for e in MUST_DIFFER if not REACHED[(e, "loose")] - REACHED[(e, "exact")]]
    assert not same, (same, {k: sorted(v) for k, v in REACHED.items() if k[0] in same})
    assert REACHED[("mrx_filter_known_dev", "exact")] == {"k_filter_gather_text"}
    assert "k_filter_gather" in REACHED[("mrx_filter_known_dev", "loose")]
