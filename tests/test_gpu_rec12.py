"""Findall with 12-byte event records (csrc/mrx_rec12.hpp): texts of at most 1 KiB at a 16-byte aligned fixed pitch.

Every case compares counts, offsets and spans with the oracle's C port (CDfa.findall_batch) AND, bit for bit, with the
same call under mrx_debug_rec12(0) -- the 16-byte records -- and asserts that the call went through k_stream_findall.
Shapes are the smallest that reach each path of the scan's record writes and of k_decode's unpacking: partial
wavefronts, the end-of-text record at every byte of a pair (pair 32 included), several tile passes, the dense row
windows with every field at its maximum, the class-table and fixed-length forms, and the rule's boundary."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mojo_regex_amd as M  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch, make_digits_batch, make_phone_batch  # noqa: E402
from mrx_ref.cfast import CDfa  # noqa: E402  (oracle: checker only)

PAT = b"[a-z]+\\d+"
TAIL = b" zz99"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path has no fallback")


def _oracle(pat, rows, lens):
    """rows: uint8[n, pitch] on the host; text i = rows[i, :lens[i]].  -> (counts, spans, total) of the oracle."""
    n = rows.shape[0]
    lens = np.asarray(lens, dtype=np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    packed = np.concatenate([rows[i, :lens[i]] for i in range(n)] + [np.zeros(0, np.uint8)])
    return CDfa(pat).findall_batch(np.ascontiguousarray(packed), offsets)


def _check(pat, d, length=None, lens=None, span_cap=None, kernel=b"k_stream_findall"):
    """d: uint8[n, pitch] on the device.  The default route against the oracle and against the 16-byte records."""
    n, pitch = d.shape
    lib = M.load_library()
    rx = M.compile_regex(pat)
    dl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    batch = M.DeviceBatch.strided(d.reshape(-1), pitch, length=length, lens=dl)
    if span_cap is None:
        span_cap = n * pitch + n
    pre, sp, tot = rx._dev_findall(batch, span_cap=span_cap)
    assert lib.mrx_last_kernel_name() == kernel
    try:
        lib.mrx_debug_rec12(0)
        pre0, sp0, tot0 = rx._dev_findall(batch, span_cap=span_cap)
        assert lib.mrx_last_kernel_name() == kernel
    finally:
        lib.mrx_debug_rec12(1)
    assert tot == tot0 and torch.equal(pre, pre0) and torch.equal(sp[:tot], sp0[:tot0])
    counts, osp, ototal = _oracle(pat, d.cpu().numpy(), [length] * n if lens is None else lens)
    assert tot == ototal == int(pre[n].item()) and int(pre[0].item()) == 0
    assert np.array_equal((pre[1:] - pre[:-1]).cpu().numpy(), counts)
    assert np.array_equal(sp[:tot].cpu().numpy(), osp)
    return pre, sp, tot


def _c2_with_tails(n, L, cut=None):
    """make_c2_batch's mix, cut to its first `cut` columns where given (so that short texts are cut from real ones)."""
    d = make_c2_batch(n, L, seed=20260318, device="cuda")
    if cut is not None:
        d = d[:, :cut].contiguous()
    return d


def _set_tail(d, rows, end):
    """Bytes [end - 5, end) of the given rows := " zz99" (as much of it as fits): a match that ends exactly at `end`."""
    k = min(len(TAIL), end)
    if k > 0:
        d[rows, end - k:end] = torch.tensor(list(TAIL[len(TAIL) - k:]), dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_wavefront_edges_and_the_match_that_ends_at_byte_1024(n):
    """Partial wavefronts; every third text's match ends with the text: the end-of-text record at pair 32."""
    _need_gpu()
    d = _c2_with_tails(n, 1024)
    _set_tail(d, torch.arange(0, n, 3, device="cuda"), 1024)
    pre, sp, tot = _check(PAT, d, length=1024)
    assert int(sp[:tot, 1].max().item()) == 1024


@pytest.mark.parametrize("length", [1, 15, 16, 17, 31, 32, 33, 1000, 1023, 1024])
def test_common_lengths_around_the_pair_boundaries(length):
    """Pairs whose odd group lies outside the text; the tail bit in F_even (length & 31 < 16) and in F_odd."""
    _need_gpu()
    pitch = (length + 15) // 16 * 16
    d = _c2_with_tails(130, 1024, cut=pitch)
    _set_tail(d, torch.arange(0, 130, 3, device="cuda"), length)
    _check(PAT, d, length=length)


def test_per_text_lengths_with_a_tail_at_every_byte_of_a_pair():
    """lens in [0, 1024] at pitch 1024, with 0, 1, 1023 and 1024 forced in; every text of 5 bytes and more ends with a
    match, so the end-of-text event falls on every value of len & 31 (and, for 1024, on pair 32)."""
    _need_gpu()
    n = 200
    rng = np.random.default_rng(20260319)
    lens = rng.integers(0, 1025, size=n)
    lens[:4] = (0, 1, 1023, 1024)
    lens[4:36] = 512 + np.arange(32)          # every residue mod 32, whatever the draw gave
    d = _c2_with_tails(n, 1024)
    for i in range(n):
        _set_tail(d, i, int(lens[i]))
    assert len(set(int(x) & 31 for x in lens)) == 32
    _check(PAT, d, lens=[int(x) for x in lens])


def test_several_tile_passes():
    """113 matches per text, 7232 per wavefront: three passes of the 3072-span tile (`tb` offsets with the new `within`)."""
    _need_gpu()
    row = (b"abcdefg1 " * 114)[:1024]
    d = torch.tensor(list(row), dtype=torch.uint8, device="cuda").repeat(130, 1)
    pre, sp, tot = _check(PAT, d, length=1024)
    assert tot == 130 * 113


def test_dense_row_windows():
    """512 matches per text, 32768 per wavefront -- above three tiles, so k_decode takes the row windows."""
    _need_gpu()
    d = torch.tensor(list(b"a1" * 512), dtype=torch.uint8, device="cuda").repeat(130, 1)
    pre, sp, tot = _check(PAT, d, length=1024)
    assert tot == 130 * 512


def test_dense_row_windows_with_every_field_at_its_maximum():
    """The one-byte-match pattern [a-z] on texts of 1024 letters takes this route too (asserted in _check): 1024 matches
    per text, so `before` and `start` reach 1023 in the record of the last pair.  A second batch mixes such texts with
    sparse ones, so that one row of a window runs far ahead of the others."""
    _need_gpu()
    d = torch.full((130, 1024), ord("q"), dtype=torch.uint8, device="cuda")
    pre, sp, tot = _check(b"[a-z]", d, length=1024)
    assert tot == 130 * 1024 and sp[tot - 1].tolist() == [1023, 1024]
    d[1::2] = make_c2_batch(65, 1024, seed=5, device="cuda")
    _check(b"[a-z]", d, length=1024)


def test_other_automaton_forms():
    """The class-table form (phone numbers, 1 KiB), short texts (digit runs, 256 B: the 2048-span tile) and the exact
    literal `ab` (fixed_len: st = pb + kk - fixed_len, with a match that ends with the text)."""
    _need_gpu()
    _check(b"(\\d{3})(\\d{3})(\\d{4})", make_phone_batch(200, device="cuda"), length=1024)
    _check(b"\\d+", make_digits_batch(200, 256, device="cuda"), length=256)
    d = _c2_with_tails(200, 1024)
    ab = torch.tensor(list(b"ab"), dtype=torch.uint8, device="cuda")
    d[::3, 1022:] = ab
    d[1::3, 15:17] = ab       # straddles the two groups of pair 0
    d[2::3, 31:33] = ab       # straddles pairs 0 and 1
    pre, sp, tot = _check(b"ab", d, length=1024)
    assert tot >= 200


def test_rule_boundary_keeps_the_16_byte_records():
    """Length and pitch 1040: above kRec12MaxLen, so the 16-byte form is still chosen -- and still exact."""
    _need_gpu()
    d = _c2_with_tails(130, 1040)
    _set_tail(d, torch.arange(0, 130, 3, device="cuda"), 1040)
    pre, sp, tot = _check(PAT, d, length=1040)
    assert int(sp[:tot, 1].max().item()) == 1040


def test_capacity_below_the_total():
    """span_cap below the total: the same return code, the same total and the same spans up to the cap as the 16-byte
    records give; the offsets are complete either way."""
    _need_gpu()
    n = 200
    d = _c2_with_tails(n, 1024)
    _set_tail(d, torch.arange(0, n, 3, device="cuda"), 1024)
    lib = M.load_library()
    rx = M.compile_regex(PAT)
    batch = M.DeviceBatch.strided(d.reshape(-1), 1024, length=1024)
    counts, osp, ototal = _oracle(PAT, d.cpu().numpy(), [1024] * n)
    cap = ototal // 2 + 1
    assert 0 < cap < ototal

    def run():
        pre = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        sp = torch.full((cap + 64, 2), -5, dtype=torch.int32, device="cuda")
        total = C.c_int64(0)
        rc = batch.call(lib, "mrx_findall", (rx._h,), (M.api._ptr(pre), M.api._ptr(sp), cap, C.byref(total), rx._stream_ptr()))
        torch.cuda.synchronize()
        assert lib.mrx_last_kernel_name() == b"k_stream_findall"
        return rc, int(total.value), pre, sp

    rc, total, pre, sp = run()
    try:
        lib.mrx_debug_rec12(0)
        rc0, total0, pre0, sp0 = run()
    finally:
        lib.mrx_debug_rec12(1)
    assert rc == rc0 == M.api.MRX_E_CAPACITY and total == total0 == ototal
    assert torch.equal(pre, pre0) and torch.equal(sp, sp0)
    assert np.array_equal(sp[:cap].cpu().numpy(), osp[:cap])
    assert bool((sp[cap:] == -5).all())          # nothing behind the capacity is written


def test_two_calls_in_flight_on_two_streams():
    """Two batches, two torch streams, separate outputs, calls enqueued alternately without a read-back in between:
    each stream's record regions are its own."""
    _need_gpu()
    rx = M.compile_regex(PAT)
    da = _c2_with_tails(200, 1024)
    _set_tail(da, torch.arange(0, 200, 3, device="cuda"), 1024)
    db = torch.tensor(list((b"abcdefg1 " * 114)[:1024]), dtype=torch.uint8, device="cuda").repeat(130, 1)
    want = [_oracle(PAT, x.cpu().numpy(), [1024] * x.shape[0]) for x in (da, db)]
    batches = [M.DeviceBatch.strided(x.reshape(-1), 1024, length=1024) for x in (da, db)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[(torch.empty(b.n + 1, dtype=torch.int64, device="cuda"),
              torch.empty((w[2] + 8, 2), dtype=torch.int32, device="cuda")) for _ in range(3)]
            for b, w in zip(batches, want)]
    torch.cuda.synchronize()
    for r in range(3):
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                rx.findall_async(batches[k], outs[k][r])
            assert M.load_library().mrx_last_kernel_name() == b"k_stream_findall"
    torch.cuda.synchronize()
    for k in (0, 1):
        counts, osp, ototal = want[k]
        for pre, sp in outs[k]:
            assert int(pre[-1].item()) == ototal
            assert np.array_equal((pre[1:] - pre[:-1]).cpu().numpy(), counts)
            assert np.array_equal(sp[:ototal].cpu().numpy(), osp)
