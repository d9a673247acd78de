"""The 12-byte event record's third word (csrc/mrx_rec12.hpp) on the host: start (10 bits), matches before (10),
pair (6, 0..32) and lane (6) packed into one dword and taken apart again, through mrx_testing_rec12_roundtrip --
every corner of the four fields, and -1 for each field one past its range.  No GPU."""
import ctypes as C
import itertools

import mojo_regex_amd as M

MAXES = {"start": 1023, "pair": 32, "lane": 63, "before": 1023}


def _roundtrip(start, pair, lane, before):
    out = (C.c_int32 * 4)(-7, -7, -7, -7)
    rc = M.load_library().mrx_testing_rec12_roundtrip(start, pair, lane, before, out)
    return rc, list(out)


def test_every_corner_of_the_four_fields_round_trips():
    for start, pair, lane, before in itertools.product((0, MAXES["start"]), (0, MAXES["pair"]), (0, MAXES["lane"]),
                                                       (0, MAXES["before"])):
        rc, out = _roundtrip(start, pair, lane, before)
        assert rc == 0 and out == [start, pair, lane, before], (start, pair, lane, before, rc, out)


def test_fields_do_not_leak_into_each_other():
    """One field at its maximum (or an inner value with mixed bits), the others at a different pattern: a shifted or
    overlapping field would show in a neighbour."""
    for start, pair, lane, before in ((1023, 0, 0, 0), (0, 32, 0, 0), (0, 0, 63, 0), (0, 0, 0, 1023),
                                      (0x2AA, 21, 42, 0x155), (0x155, 10, 21, 0x2AA), (1, 31, 1, 1), (512, 16, 32, 512)):
        rc, out = _roundtrip(start, pair, lane, before)
        assert rc == 0 and out == [start, pair, lane, before], (start, pair, lane, before, rc, out)


def test_one_past_each_range_is_refused():
    ok = {"start": 5, "pair": 3, "lane": 7, "before": 9}
    for name, top in MAXES.items():
        for bad in (top + 1, -1):
            args = dict(ok)
            args[name] = bad
            rc, out = _roundtrip(args["start"], args["pair"], args["lane"], args["before"])
            assert rc == -1 and out == [-7, -7, -7, -7], (name, bad, rc, out)
    assert M.load_library().mrx_testing_rec12_roundtrip(0, 0, 0, 0, None) == -1


def test_hooks_are_declared():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mrx_testing.h")).read()
    lib = M.load_library()
    for name in ("mrx_debug_rec12", "mrx_testing_rec12_roundtrip"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in M.api.TESTING_SYMBOLS_NUMBERED and hasattr(lib, name), name
