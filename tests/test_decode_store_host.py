"""The index arithmetic of k_decode's 16-byte span stores (decode_store_plan, csrc/mrx_decode_bits.hpp) on the host,
through mrx_testing_decode_store_plan: every plan replayed into a sentinel-filled array.

The model: memory is a row of 8-byte cells; the span buffer begins at cell `a` (the parity of its address / 8), so span
index i is cell a + i, and a 16-byte store is legal on an even cell only.  The tile holds span k of the wavefront at
slot k + odd.  Every combination of the parity of pre0, the parity of the address, nspan in 0..9 and TILE - 1, TILE
(both tile sizes) and span_cap from pre0 - 1 to pre0 + nspan + 1; tools/decode_store_check.cpp enumerates the same
cases in C++ under the sanitizers."""
import ctypes as C

import numpy as np
import pytest

import mojo_regex_amd as M

SENTINEL = -77


def _plan(pre0, a, nspan, cap):
    out = (C.c_int32 * 5)(*([-1] * 5))
    assert M.load_library().mrx_testing_decode_store_plan(pre0, a, nspan, cap, out) == 0
    return tuple(out)   # odd, head, npairs, tail, nclip


def _replay(pre0, a, nspan, cap, tile_slots):
    odd, head, npairs, tail, nclip = _plan(pre0, a, nspan, cap)
    ctx = (pre0, a, nspan, cap)
    assert odd == (pre0 + a) & 1, ctx
    assert head in (0, 1) and tail in (0, 1) and npairs >= 0, ctx          # the head and the tail are single spans
    assert head + 2 * npairs + tail == nclip, ctx
    assert nspan + odd <= tile_slots, ctx
    tile = np.full(tile_slots, SENTINEL, np.int64)
    tile[odd:odd + nspan] = np.arange(nspan)
    size = max(cap, pre0 + nspan) + 4                                        # (room behind span_cap, to see a write there)
    mem = np.full(size, SENTINEL, np.int64)
    hits = np.zeros(size, np.int64)
    if head:
        mem[pre0] = tile[odd]
        hits[pre0] += 1
    if npairs:
        k0 = head                                                            # first span of the first pair
        assert (a + pre0 + k0) % 2 == 0, ctx                                 # pairs on even cells (k advances by 2) ...
        assert (k0 + odd) % 2 == 0, ctx                                      # ... and on even tile slots
        assert k0 + odd + 2 * npairs <= tile_slots, ctx
        mem[pre0 + k0:pre0 + k0 + 2 * npairs] = tile[k0 + odd:k0 + odd + 2 * npairs]
        hits[pre0 + k0:pre0 + k0 + 2 * npairs] += 1
    if tail:
        k = head + 2 * npairs
        mem[pre0 + k] = tile[k + odd]
        hits[pre0 + k] += 1
    end = max(pre0, min(pre0 + nspan, cap))
    want_hits = np.zeros(size, np.int64)
    want_hits[pre0:end] = 1
    assert np.array_equal(hits, want_hits), ctx                              # each span in range once, nothing outside
    want = np.full(size, SENTINEL, np.int64)
    want[pre0:end] = np.arange(end - pre0)
    assert np.array_equal(mem, want), ctx
    assert nclip == end - pre0, ctx


@pytest.mark.parametrize("tile", [2048, 3072])
def test_every_plan_writes_its_range_once_and_nothing_else(tile):
    cases = 0
    for pre0 in (6, 7):
        for a in (0, 1):
            for nspan in list(range(10)) + [tile - 1, tile]:
                for cap in range(pre0 - 1, pre0 + nspan + 2):
                    _replay(pre0, a, nspan, cap, tile + 2)
                    cases += 1
    assert cases == 4 * (sum(n + 3 for n in range(10)) + 2 * tile + 5)


def test_the_plan_depends_on_the_parity_of_pre0_only():
    """Span indices beyond 2^31: the same plan as at a small base of the same parity."""
    for pre0 in ((1 << 31) + 2, (1 << 31) + 3, (1 << 40) + 1):
        small = 6 + (pre0 & 1)
        for a in (0, 1):
            for nspan in range(10):
                for d in range(-1, nspan + 2):
                    assert _plan(pre0, a, nspan, pre0 + d) == _plan(small, a, nspan, small + d), (pre0, a, nspan, d)


def test_a_capacity_far_below_or_far_above():
    assert _plan(100, 0, 9, 0) == (0, 0, 0, 0, 0)
    assert _plan(101, 0, 9, -5) == (1, 0, 0, 0, 0)
    assert _plan(101, 0, 9, 1 << 62) == (1, 1, 4, 0, 9)
    assert _plan(100, 0, 9, 1 << 62) == (0, 0, 4, 1, 9)


def test_bad_arguments_are_refused():
    lib = M.load_library()
    out = (C.c_int32 * 5)()
    assert lib.mrx_testing_decode_store_plan(0, 0, -1, 10, out) == -1
    assert lib.mrx_testing_decode_store_plan(0, 2, 1, 10, out) == -1
    assert lib.mrx_testing_decode_store_plan(0, 0, 1, 10, None) == -1
