"""k_decode's tile store loops with two spans per lane and trip (k_decode<..., STORE16 = true>, decode_store_plan in
csrc/mrx_decode_bits.hpp).

Every case runs the call four times -- the span buffer 16-byte aligned and 8 bytes off it (`buf[1:]` of a sentinel-filled
buffer), each with 16-byte stores and under mrx_debug_decode_store16(0) -- and compares counts_prefix, the total and every
span with the oracle's C port (CDfa.findall_batch), the two store forms bit for bit, and every row of the buffer the call
must not write (the one in front of the spans, those behind min(total, span_cap)) with the sentinel.

Most batches hold spaces and digits under `\\d`, so that a text with k digits has exactly k spans and a wavefront's
count, and with it the parity of the next wavefront's first span, is chosen by the test."""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mojo_regex_amd as M  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch, to_ragged  # noqa: E402
from mrx_ref.cfast import CDfa  # noqa: E402  (oracle: checker only)

PAT = b"[a-z]+\\d+"
SENTINEL = -5
KERNELS = (b"k_stream_findall", b"k_stream_findall_pieces", b"k_stream_findall_dyn")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path has no fallback")


@contextlib.contextmanager
def _switch(name, value, back):
    lib = M.load_library()
    getattr(lib, name)(value)
    try:
        yield
    finally:
        getattr(lib, name)(back)


def _digit_rows(counts, L):
    """Row i: spaces and counts[i] digits at its end (the last one ends with the text): counts[i] spans under \\d."""
    rows = np.full((len(counts), L), ord(" "), dtype=np.uint8)
    digits = np.frombuffer(b"0123456789", dtype=np.uint8)
    for i, c in enumerate(counts):
        assert 0 <= c <= L
        if c:
            rows[i, L - c:] = digits[np.arange(c) % 10]
    return rows


def _spread(total, texts=64):
    """`total` spans over the texts of a wavefront, as evenly as they go."""
    return [total // texts + (1 if t < total % texts else 0) for t in range(texts)]


def _oracle_rows(pat, rows, lens=None):
    n, L = rows.shape
    lens = np.full(n, L, np.int64) if lens is None else np.asarray(lens, np.int64)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    packed = np.concatenate([rows[i, :lens[i]] for i in range(n)] + [np.zeros(0, np.uint8)])
    return CDfa(pat).findall_batch(np.ascontiguousarray(packed), offsets)


def _call(rx, batch, cap, room, off, st16, kernels=KERNELS):
    """One mrx_findall with `cap` as the capacity into rows [off, off + room) of a sentinel-filled buffer."""
    lib = M.load_library()
    assert room >= cap
    pre = torch.empty(batch.n + 1, dtype=torch.int64, device="cuda")
    buf = torch.full((room + 1 + off, 2), SENTINEL, dtype=torch.int32, device="cuda")
    sp = buf[off:]
    assert sp.data_ptr() % 16 == 8 * off
    total = C.c_int64(0)
    was = lib.mrx_debug_last_decode_store16()
    with _switch("mrx_debug_decode_store16", st16, 1):
        rc = batch.call(lib, "mrx_findall", (rx._h,), (M.api._ptr(pre), M.api._ptr(sp), cap, C.byref(total), rx._stream_ptr()))
        torch.cuda.synchronize()
        assert lib.mrx_last_kernel_name() in kernels, lib.mrx_last_kernel_name()
        assert lib.mrx_debug_last_decode_store16() == st16, (was, st16)
    return rc, int(total.value), pre, buf


def _check(pat, batch, want, cap=None, kernels=KERNELS):
    """want = (counts, spans, total) of the oracle.  Both address parities, both store forms."""
    _need_gpu()
    counts, osp, ototal = want
    osp = np.asarray(osp, np.int32).reshape(-1, 2)
    cap = ototal if cap is None else cap
    room = max(cap, ototal) + 3
    kept = min(cap, ototal)
    rx = M.compile_regex(pat)
    n = batch.n
    for off in (0, 1):
        bufs = []
        for st16 in (1, 0):      # (one after the other: a launch that left the hook alone would fail one of the two)
            rc, total, pre, buf = _call(rx, batch, cap, room, off, st16, kernels)
            assert rc == (M.api.MRX_OK if cap >= ototal else M.api.MRX_E_CAPACITY), (rc, off, st16)
            assert total == ototal == int(pre[n].item()) and int(pre[0].item()) == 0
            assert np.array_equal((pre[1:] - pre[:-1]).cpu().numpy(), counts)
            got = buf.cpu().numpy()
            assert np.array_equal(got[off:off + kept], osp[:kept]), (off, st16)
            assert (got[:off] == SENTINEL).all(), "the row in front of the spans was written (%d, %d)" % (off, st16)
            assert (got[off + kept:] == SENTINEL).all(), "a row at or behind the capacity was written (%d, %d)" % (off, st16)
            bufs.append((pre, buf))
        assert torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][1], bufs[1][1])
    return ototal


def _strided(rows, lens=None):
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    n, L = rows.shape
    dl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    return M.DeviceBatch.strided(d.reshape(-1), L, length=None if lens is not None else L, lens=dl)


# ---- both parities of a wavefront's first span -----------------------------------------------------------------------

@pytest.mark.parametrize("n", [65, 129])
@pytest.mark.parametrize("first", [37, 38], ids=["odd_first_wavefront", "even_first_wavefront"])
def test_texts_of_64_to_256_bytes_behind_an_odd_and_an_even_wavefront(n, first):
    rng = np.random.default_rng(1000 + n + first)
    lens = rng.integers(64, 257, size=n)
    counts = rng.integers(0, 6, size=n)
    counts[:64] = _spread(first)
    rows = np.full((n, 256), ord(" "), dtype=np.uint8)
    for i in range(n):   # digits at the end of the text, not of the row
        rows[i, lens[i] - counts[i]:lens[i]] = ord("0") + (np.arange(counts[i]) % 10)
    want = _oracle_rows(b"\\d", rows, lens)
    assert int(np.sum(want[0][:64])) == first and want[2] == int(counts.sum())
    _check(b"\\d", _strided(rows, lens.tolist()), want)


def test_wavefronts_of_zero_to_three_spans_at_either_parity():
    """Wavefront totals 0 1 0 1 2 3 2 3 1: every count of 0..3 behind an even and behind an odd number of spans."""
    totals = [0, 1, 0, 1, 2, 3, 2, 3, 1]
    pre = np.concatenate([[0], np.cumsum(totals)[:-1]])
    assert {(c, int(p) & 1) for c, p in zip(totals, pre)} >= {(c, q) for c in range(4) for q in (0, 1)}
    counts = []
    for t in totals:
        w = [0] * 64
        for k in range(t):
            w[(17 * k + 5) % 64] += 1
        counts += w
    rows = _digit_rows(counts, 64)
    want = _oracle_rows(b"\\d", rows)
    assert want[2] == sum(totals)
    _check(b"\\d", _strided(rows), want)


# ---- capacity ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("below", [0, 1, 2, "first_pair_aligned", "first_pair_shifted"])
def test_capacity_clips_per_span(below):
    """span_cap at the total, one and two below it, and inside the first wavefront's first pair: spans 0 and 1 where the
    buffer is aligned, spans 1 and 2 where it is 8 bytes off (span 0 is then the head)."""
    rows = _digit_rows(_spread(37) + _spread(90) + [2], 128)
    want = _oracle_rows(b"\\d", rows)
    assert want[2] == 129
    cap = {"first_pair_aligned": 1, "first_pair_shifted": 2}.get(below, want[2] - (below if isinstance(below, int) else 0))
    _check(b"\\d", _strided(rows), want, cap=cap)


# ---- every path in one launch --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,tile", [(1024, 3072), (256, 2048)])
@pytest.mark.parametrize("lead", [3, 4], ids=["odd_lead", "even_lead"])
def test_lean_multi_pass_and_dense_wavefronts_in_one_launch(L, tile, lead):
    """A sparse wavefront of `lead` spans, then wavefronts of exactly TILE, TILE - 1 and TILE + 1 spans (the last takes
    two passes of the tile loop), one above 3 x TILE (the dense row windows), and a last one of a single text."""
    dense = 3 * tile + 64
    counts = _spread(lead) + _spread(tile) + _spread(tile - 1) + _spread(tile + 1) + _spread(dense) + [2]
    rows = _digit_rows(counts, L)
    want = _oracle_rows(b"\\d", rows)
    assert want[2] == lead + 3 * tile + dense + 2
    _check(b"\\d", _strided(rows), want, kernels=(b"k_stream_findall",))
    _check(b"\\d", _strided(rows), want, cap=lead + 2 * tile + 5, kernels=(b"k_stream_findall",))   # (inside a second pass)


# ---- record forms, slot forms, batch layouts -------------------------------------------------------------------------------

def test_sixteen_byte_records_of_1040_byte_texts():
    rows = make_c2_batch(130, 1040, seed=20261021, device="cuda").cpu().numpy()
    assert _check(PAT, _strided(rows), _oracle_rows(PAT, rows), kernels=(b"k_stream_findall",)) > 130


@pytest.mark.parametrize("long_mode", [0, 2], ids=["long_text_rule", "no_long_text_kernels"])
def test_eight_byte_tile_slots_for_a_text_above_65300_bytes(long_mode):
    """Positions that need 32 bits: int2 tile slots, pairs read with one 16-byte LDS read.  Three texts of 70 000 bytes
    with a digit every 47 bytes and two short ones: about 4 500 spans in a wavefront, three passes of the tile loop."""
    texts = []
    for k in range(3):
        t = np.full(70000 + k, ord(" "), dtype=np.uint8)
        t[k::47] = ord("0") + k
        texts.append(t.tobytes())
    texts += [b"7", b"a1 b22 c333"]
    batch = M.DeviceBatch.from_texts(texts)
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    want = CDfa(b"\\d").findall_batch(np.ascontiguousarray(data), offsets)
    assert want[2] > 2 * 2048
    with _switch("mrx_debug_long_text_kernels", long_mode, 0):
        _check(b"\\d", batch, want, kernels=(b"k_stream_findall", b"k_stream_findall_pieces"))
        _check(b"\\d", batch, want, cap=want[2] - 1, kernels=(b"k_stream_findall", b"k_stream_findall_pieces"))


def test_ragged_csr_batch_on_dynamic_tasks():
    data, offsets = to_ragged(make_c2_batch(300, 1024, seed=20261022, device="cuda"), 0)
    want = CDfa(PAT).findall_batch(data.cpu().numpy(), offsets.cpu().numpy())
    with _switch("mrx_debug_long_text_kernels", 2, 0), _switch("mrx_debug_dynamic_texts", 1, 0):
        _check(PAT, M.DeviceBatch(data, offsets), want, kernels=(b"k_stream_findall_dyn",))
        _check(PAT, M.DeviceBatch(data, offsets), want, cap=want[2] - 2, kernels=(b"k_stream_findall_dyn",))


def test_ragged_csr_batch_on_static_tasks():
    data, offsets = to_ragged(make_c2_batch(300, 1024, seed=20261023, device="cuda"), 0)
    want = CDfa(PAT).findall_batch(data.cpu().numpy(), offsets.cpu().numpy())
    with _switch("mrx_debug_long_text_kernels", 2, 0), _switch("mrx_debug_dynamic_texts", 2, 0):
        _check(PAT, M.DeviceBatch(data, offsets), want, kernels=(b"k_stream_findall",))


def test_split_findall_adds_the_first_half_through_base():
    """mrx_debug_split_findall(1) at the split's minimum size, the first half with an odd total."""
    n = (1 << 18) + 65
    period = np.frombuffer(b"abcxyz0189 -", dtype=np.uint8)[np.random.default_rng(20261021).integers(0, 12, size=(389, 16))]
    rows = np.tile(period, ((n + 388) // 389, 1))[:n].copy()
    rows[0] = np.frombuffer(b"a1 b2 c3 d4 e5  ", dtype=np.uint8)
    want = _oracle_rows(PAT, rows)
    half = ((n // 2) // 64) * 64
    if int(np.sum(want[0][:half])) % 2 == 0:   # (one span less in the first half)
        rows[0, 1] = ord(" ")
        want = _oracle_rows(PAT, rows)
    assert int(np.sum(want[0][:half])) % 2 == 1
    with _switch("mrx_debug_split_findall", 1, 0):
        _check(PAT, _strided(rows), want, kernels=(b"k_stream_findall",))


# ---- two streams ---------------------------------------------------------------------------------------------------------

def test_two_calls_in_flight_on_two_streams():
    _need_gpu()
    lib = M.load_library()
    rx = M.compile_regex(b"\\d")
    ra = _digit_rows(_spread(37) + _spread(3071) + [1], 1024)
    rb = _digit_rows(_spread(3073) + _spread(38) + [3], 1024)
    want = [_oracle_rows(b"\\d", r) for r in (ra, rb)]
    batches = [_strided(r) for r in (ra, rb)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [[torch.full((w[2] + 2, 2), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)] for w in want]
    pres = [[torch.empty(b.n + 1, dtype=torch.int64, device="cuda") for _ in range(3)] for b in batches]
    torch.cuda.synchronize()
    with _switch("mrx_debug_decode_store16", 1, 1):
        for r in range(3):
            for k in (0, 1):
                with torch.cuda.stream(streams[k]):
                    rx.findall_async(batches[k], (pres[k][r], bufs[k][r][k:k + want[k][2]]))   # (stream 1: 8 bytes off)
                assert lib.mrx_debug_last_decode_store16() == 1
        torch.cuda.synchronize()
    for k in (0, 1):
        counts, osp, ototal = want[k]
        for pre, buf in zip(pres[k], bufs[k]):
            got = buf.cpu().numpy()
            assert int(pre[-1].item()) == ototal
            assert np.array_equal((pre[1:] - pre[:-1]).cpu().numpy(), counts)
            assert np.array_equal(got[k:k + ototal], np.asarray(osp, np.int32).reshape(-1, 2))
            assert (got[:k] == SENTINEL).all() and (got[k + ototal:] == SENTINEL).all()
