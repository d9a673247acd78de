"""k_decode's lean pass (csrc/mrx_decode_bits.hpp): wavefronts of the streaming findall whose spans fit one LDS tile.

Every case compares counts, offsets and spans with the oracle's C port (CDfa.findall_batch) AND, bit for bit, with the
same call under mrx_debug_decode_lean(0) -- the general tile loop -- and asserts that the call went through
k_stream_findall and that the decode launch was the lean instantiation on one side of the switch and the general one
on the other (mrx_debug_last_decode_lean).  Shapes are the smallest that reach each edge: partial wavefronts and a
partial last batch of records, the end-of-text record at every byte of a pair, a start carried over many pairs, records with 32 spans, the multi-pass
and dense paths next to it (unchanged, and equal), the fixed-length form, both tiles and both record widths."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mojo_regex_amd as M  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch, make_digits_batch, to_ragged  # noqa: E402
from mrx_ref.cfast import CDfa  # noqa: E402  (oracle: checker only)

PAT = b"[a-z]+\\d+"
TAIL = b" zz99"
# what the switch is put back to: the library's default, which MRX_DECODE_LEAN=0 overrides
_LEAN_DEFAULT = 0 if os.environ.get("MRX_DECODE_LEAN", "").strip() == "0" else 1


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


def _check(pat, d, length=None, lens=None, kernel=b"k_stream_findall"):
    """d: uint8[n, pitch] on the device.  The default route against the oracle and against the general tile loop."""
    n, pitch = d.shape
    lib = M.load_library()
    rx = M.compile_regex(pat)
    dl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    batch = M.DeviceBatch.strided(d.reshape(-1), pitch, length=length, lens=dl)
    span_cap = n * pitch + n
    default = _LEAN_DEFAULT
    try:
        lib.mrx_debug_decode_lean(1)
        pre, sp, tot = rx._dev_findall(batch, span_cap=span_cap)
        assert lib.mrx_last_kernel_name() == kernel and lib.mrx_debug_last_decode_lean() == 1
        lib.mrx_debug_decode_lean(0)
        pre0, sp0, tot0 = rx._dev_findall(batch, span_cap=span_cap)
        assert lib.mrx_last_kernel_name() == kernel and lib.mrx_debug_last_decode_lean() == 0
    finally:
        lib.mrx_debug_decode_lean(default)
    assert tot == tot0 and torch.equal(pre, pre0) and torch.equal(sp[:tot], sp0[:tot0])
    counts, osp, ototal = _oracle(pat, d.cpu().numpy(), [length] * n if lens is None else lens)
    assert tot == ototal == int(pre[n].item()) and int(pre[0].item()) == 0
    assert np.array_equal((pre[1:] - pre[:-1]).cpu().numpy(), counts)
    assert np.array_equal(sp[:tot].cpu().numpy(), osp)
    return pre, sp, tot


def _c2(n, L=1024, cut=None):
    d = make_c2_batch(n, L, seed=20260421, device="cuda")
    if cut is not None:
        d = d[:, :cut].contiguous()
    return d


def _set_tail(d, rows, end):
    """Bytes [end - 5, end) of the given rows := " zz99" (as much of it as fits): a match that ends exactly at `end`."""
    k = min(len(TAIL), end)
    if k > 0:
        d[rows, end - k:end] = torch.tensor(list(TAIL[len(TAIL) - k:]), dtype=torch.uint8, device="cuda")


def _rows(row, n):
    return torch.tensor(list(row), dtype=torch.uint8, device="cuda").repeat(n, 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_partial_wavefronts_and_a_partial_last_batch_of_records(n):
    _need_gpu()
    d = _c2(n)
    _set_tail(d, torch.arange(0, n, 3, device="cuda"), 1024)
    pre, sp, tot = _check(PAT, d, length=1024)
    assert int(sp[:tot, 1].max().item()) == 1024


@pytest.mark.parametrize("length", [1, 15, 16, 17, 31, 32, 33, 1023, 1024])
def test_common_lengths_around_the_pair_boundaries(length):
    _need_gpu()
    pitch = (length + 15) // 16 * 16
    d = _c2(130, cut=pitch)
    _set_tail(d, torch.arange(0, 130, 3, device="cuda"), length)
    _check(PAT, d, length=length)


def test_per_text_lengths_with_the_end_of_text_record_at_every_byte_of_a_pair():
    _need_gpu()
    n = 1100
    lens = [i % 1025 for i in range(n)]
    d = _c2(n)
    col = torch.arange(1024, device="cuda")[None, :]
    ends = torch.tensor(lens, device="cuda")[:, None]
    tail = torch.tensor(list(TAIL), dtype=torch.uint8, device="cuda")
    k = col - (ends - 5)                                  # bytes [len - 5, len) := " zz99", as much of it as fits
    inside = (k >= 0) & (k < 5)
    d[inside] = tail[k[inside]]
    _check(PAT, d, lens=lens)


def test_a_start_carried_over_ten_pairs_and_three_chunks():
    """One token of 300 letters and two digits per text, at a different offset in each: its start is carried by the
    records' start field over ten pairs (and three 128-byte chunks of the scan) to the record that holds its end."""
    _need_gpu()
    n = 70
    d = torch.full((n, 1024), ord(" "), dtype=torch.uint8, device="cuda")
    tok = torch.tensor(list(b"q" * 300 + b"42"), dtype=torch.uint8, device="cuda")
    for i in range(n):
        d[i, 3 * i:3 * i + 302] = tok
    pre, sp, tot = _check(PAT, d, length=1024)
    assert tot == n and sp[:tot].tolist() == [[3 * i, 3 * i + 302] for i in range(n)]


def test_dense_path_next_to_it_is_unchanged():
    """[a-z] on 64 texts of 1024 letters: 32 spans per record, 65 536 per wavefront -- the dense row windows."""
    _need_gpu()
    d = torch.full((64, 1024), ord("q"), dtype=torch.uint8, device="cuda")
    pre, sp, tot = _check(b"[a-z]", d, length=1024)
    assert tot == 64 * 1024


@pytest.mark.parametrize("letters,length", [(40, 1024), (60, 1024), (30, 48), (40, 48), (60, 64)])
def test_full_records_on_either_side_of_the_tile(letters, length):
    """[a-z] on 64 texts that begin with `letters` letters: records with 32 spans.  In 1 KiB texts (3072-span tile) 40
    letters are 2 560 spans, the lean pass, and 60 are 3 840, two passes of the general loop; in short texts (2048-span
    tile) 30 letters are 1 920 spans, lean, 40 are two passes and 60 letters of 64 bytes two as well."""
    _need_gpu()
    d = torch.full((64, length), ord(" "), dtype=torch.uint8, device="cuda")
    d[:, :letters] = ord("k")
    pre, sp, tot = _check(b"[a-z]", d, length=length)
    assert tot == 64 * letters


def test_fixed_length_form():
    """`hello` at offsets 0, 11, 27 and len - 5: start = end - 5 whatever the records' start field says."""
    _need_gpu()
    d = _c2(130)
    hello = torch.tensor(list(b"hello"), dtype=torch.uint8, device="cuda")
    for at in (0, 11, 27, 1024 - 5):
        d[:, at:at + 5] = hello
    pre, sp, tot = _check(b"hello", d, length=1024)
    assert tot >= 4 * 130 and sp[0].tolist() == [0, 5] and sp[tot - 1].tolist() == [1019, 1024]


def test_short_texts_take_the_2048_span_tile():
    _need_gpu()
    _check(b"\\d+", make_digits_batch(200, 256, device="cuda"), length=256)


def test_sixteen_byte_records_with_the_lean_pass():
    _need_gpu()
    lib = M.load_library()
    try:
        lib.mrx_debug_rec12(0)
        d = _c2(130)
        _set_tail(d, torch.arange(0, 130, 3, device="cuda"), 1024)
        _check(PAT, d, length=1024)
        _check(PAT, _c2(130, 1040), length=1040)           # (a pitch the 12-byte records do not take either way)
        _check(b"\\d+", make_digits_batch(200, 256, device="cuda"), length=256)
    finally:
        lib.mrx_debug_rec12(1)


@pytest.mark.parametrize("pat", [PAT, b"\\d+", b"ab"])
def test_ragged_batches_whose_first_pair_lies_in_front_of_the_text(pat):
    """Texts packed back to back (offsets): a text's first pair begins up to 143 bytes in front of it, so the records'
    pair position is negative -- the empty-mask value of the start arithmetic must not wrap there."""
    _need_gpu()
    lib = M.load_library()
    data, offsets = to_ragged(_c2(300), 0)
    batch = M.DeviceBatch(data, offsets)
    rx = M.compile_regex(pat)
    try:
        lib.mrx_debug_decode_lean(1)
        pre, sp, tot = rx._dev_findall(batch, span_cap=int(data.numel()) + 300)
        ran_lean = lib.mrx_debug_last_decode_lean()
        lib.mrx_debug_decode_lean(0)
        pre0, sp0, tot0 = rx._dev_findall(batch, span_cap=int(data.numel()) + 300)
        assert lib.mrx_debug_last_decode_lean() == 0
    finally:
        lib.mrx_debug_decode_lean(_LEAN_DEFAULT)
    assert ran_lean == 1        # (a static task with two-word records: the form the lean pass covers)
    assert tot == tot0 and torch.equal(pre, pre0) and torch.equal(sp[:tot], sp0[:tot0])
    counts, osp, ototal = CDfa(pat).findall_batch(data.cpu().numpy(), offsets.cpu().numpy())
    assert tot == ototal
    assert np.array_equal((pre[1:] - pre[:-1]).cpu().numpy(), counts)
    assert np.array_equal(sp[:tot].cpu().numpy(), osp)


def test_capacity_seven_below_the_total():
    """Spans up to the capacity are written, the seven slots behind it keep their canary, the call reports the
    capacity error -- with the lean pass and without."""
    _need_gpu()
    n = 130
    d = _c2(n)
    _set_tail(d, torch.arange(0, n, 3, device="cuda"), 1024)
    lib = M.load_library()
    rx = M.compile_regex(PAT)
    batch = M.DeviceBatch.strided(d.reshape(-1), 1024, length=1024)
    counts, osp, ototal = _oracle(PAT, d.cpu().numpy(), [1024] * n)
    cap = ototal - 7
    assert cap > 0

    def run():
        pre = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        sp = torch.full((ototal, 2), -5, dtype=torch.int32, device="cuda")
        total = C.c_int64(0)
        rc = batch.call(lib, "mrx_findall", (rx._h,), (M.api._ptr(pre), M.api._ptr(sp), cap, C.byref(total), rx._stream_ptr()))
        torch.cuda.synchronize()
        assert lib.mrx_last_kernel_name() == b"k_stream_findall"
        return rc, int(total.value), pre, sp

    try:
        lib.mrx_debug_decode_lean(1)
        rc, total, pre, sp = run()
        assert lib.mrx_debug_last_decode_lean() == 1
        lib.mrx_debug_decode_lean(0)
        rc0, total0, pre0, sp0 = run()
        assert lib.mrx_debug_last_decode_lean() == 0
    finally:
        lib.mrx_debug_decode_lean(_LEAN_DEFAULT)
    assert rc == rc0 == M.api.MRX_E_CAPACITY and total == total0 == ototal
    assert torch.equal(pre, pre0) and torch.equal(sp, sp0)
    assert np.array_equal(sp[:cap].cpu().numpy(), osp[:cap])
    assert sp.shape[0] - cap == 7 and bool((sp[cap:] == -5).all())


def test_two_calls_in_flight_on_two_streams():
    _need_gpu()
    lib = M.load_library()
    lib.mrx_debug_decode_lean(1)
    try:
        _two_streams()
        assert lib.mrx_debug_last_decode_lean() == 1
    finally:
        lib.mrx_debug_decode_lean(_LEAN_DEFAULT)


def _two_streams():
    rx = M.compile_regex(PAT)
    da = _c2(130)
    _set_tail(da, torch.arange(0, 130, 3, device="cuda"), 1024)
    db = _rows((b"abcdefg1 " * 114)[:1024], 70)            # 113 matches a text: three passes of the general loop
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
