"""k_decode's per-wavefront header: the task index and the wavefront's base, record count and `base` as
scalars, the sums of the scan tiles in front and the counts' exclusive scan on the DPP path, and the lean pass's first
batch of records requested at the top of the task.

Every case compares `counts_prefix`, the total and every span with the oracle's C port (CDfa.findall_batch).  The
shapes are the smallest at which the header can go wrong: wavefronts of 1, 63, 64 and 65 texts, a last wavefront
without a record, a batch without a match, wavefronts on either side of a scan tile (2048 wavefronts), more scan tiles
in front than a wavefront has lanes (65), every instantiation that shares the header, the three expansion paths whose
choice is now a scalar branch, the second half of a split call (`base`), and a capacity below the total.  The large
batches repeat a short period of distinct texts; their expected CSR is built from the oracle's answer for one period."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mojo_regex_amd as M  # noqa: E402
from mojo_regex_amd.workloads import make_c2_batch, make_digits_batch  # noqa: E402
from mrx_ref.cfast import CDfa  # noqa: E402  (oracle: checker only)

PAT = b"[a-z]+\\d+"
ALPHABET = b"abcxyz0189 -"
# what the switch is put back to: the library's default, which MRX_DECODE_LEAN=0 overrides
_LEAN_DEFAULT = 0 if os.environ.get("MRX_DECODE_LEAN", "").strip() == "0" else 1
_SCAN_TILE = 2048          # wavefronts per k_scan_local tile (kScanTile)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path has no fallback")


def _random_rows(n, L, seed, alphabet=ALPHABET):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=(n, L))]


def _oracle(pat, rows, lens):
    """rows: uint8[n, pitch] on the host; text i = rows[i, :lens[i]].  -> (counts, spans, total) of the oracle."""
    n = rows.shape[0]
    lens = np.asarray(lens, dtype=np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    packed = np.concatenate([rows[i, :lens[i]] for i in range(n)] + [np.zeros(0, np.uint8)])
    return CDfa(pat).findall_batch(np.ascontiguousarray(packed), offsets)


def _findall(pat, d, length, lens, lean, span_cap):
    """One call with the lean switch at `lean`; asserts the route and the instantiation through the last-call hooks."""
    lib = M.load_library()
    n, pitch = d.shape
    dl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    batch = M.DeviceBatch.strided(d.reshape(-1), pitch, length=length, lens=dl)
    try:
        lib.mrx_debug_decode_lean(lean)
        pre, sp, tot = M.compile_regex(pat)._dev_findall(batch, span_cap=span_cap)
        assert lib.mrx_last_kernel_name() == b"k_stream_findall"
        assert lib.mrx_debug_last_decode_lean() == lean
    finally:
        lib.mrx_debug_decode_lean(_LEAN_DEFAULT)
    return pre, sp, tot


def _check(pat, rows, length=None, lens=None, both=False):
    """rows: uint8[n, pitch] on the host.  The lean instantiation against the oracle; with `both`, the general tile loop
    behind the same header too, bit-equal."""
    n, pitch = rows.shape
    counts, osp, ototal = _oracle(pat, rows, [length] * n if lens is None else lens)
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    span_cap = ototal + 3
    outs = [_findall(pat, d, length, lens, lean, span_cap) for lean in ((1, 0) if both else (1,))]
    for pre, sp, tot in outs:
        assert tot == ototal == int(pre[n].item()) and int(pre[0].item()) == 0
        assert np.array_equal((pre[1:] - pre[:-1]).cpu().numpy(), counts)
        assert np.array_equal(sp[:tot].cpu().numpy(), osp)
    if both:
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1][:ototal], outs[1][1][:ototal])
    return ototal


# ---- partial and exact wavefronts ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129])
def test_partial_and_exact_wavefronts(n):
    """32-byte texts at pitch 32: the exclusive scan, the stores of prefix[n] and the total by the lane of text n - 1,
    and the clamped record loads of a wavefront with fewer than 64 texts."""
    _need_gpu()
    rows = _random_rows(n, 32, 100 + n)
    rows[::3, 27:] = np.frombuffer(b" zz99", dtype=np.uint8)   # (a match that ends with the text, in text 0 too)
    assert _check(PAT, rows, length=32, both=True) >= (n + 2) // 3


@pytest.mark.parametrize("n", [65, 129])
def test_last_wavefront_without_a_record(n):
    """The texts of the last wavefront hold no match: it has zero records, and its early loads read the first slot of
    its own region."""
    _need_gpu()
    rows = _random_rows(n, 32, 200 + n)
    rows[n - (n % 64):] = ord(" ")
    assert _check(PAT, rows, length=32, both=True) > 0


def test_batch_without_a_match():
    _need_gpu()
    assert _check(PAT, np.full((129, 32), ord("-"), dtype=np.uint8), length=32, both=True) == 0


# ---- across scan tiles -----------------------------------------------------------------------------------------

_PERIOD = 389   # texts in a period: a prime, so that no two wavefronts of a scan tile hold the same texts


def _periodic(n):
    """n texts of 16 bytes that repeat a period of distinct texts, on the device, and their CSR from the oracle's answer
    for one period: (rows on the device, prefix int64[n + 1], spans int32[total, 2])."""
    period = _random_rows(_PERIOD, 16, 20261019)
    counts_p, spans_p, total_p = _oracle(PAT, period, [16] * _PERIOD)
    assert total_p > _PERIOD // 4 and len(set(period.tobytes()[i * 16:i * 16 + 16] for i in range(_PERIOD))) == _PERIOD
    k, r = divmod(n, _PERIOD)
    dp = torch.from_numpy(period).cuda()
    d = torch.cat([dp.repeat(k, 1), dp[:r]])
    cp = torch.from_numpy(np.asarray(counts_p, dtype=np.int64)).cuda()
    prefix = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(torch.cat([cp.repeat(k), cp[:r]]), 0, out=prefix[1:])
    sp = torch.from_numpy(np.asarray(spans_p, dtype=np.int32).reshape(-1, 2)).cuda()
    spans = torch.cat([sp.repeat(k, 1), sp[:int(counts_p[:r].sum())]])
    return d, prefix, spans


@pytest.mark.parametrize("n", [64 * _SCAN_TILE + 65, 64 * _SCAN_TILE * 65 + 1],
                         ids=["one_tile_in_front", "sixty_five_tiles_in_front"])
def test_across_scan_tiles(n):
    """One scan tile and a partial wavefront behind it; and 65 tiles in front of the last wavefront, one more than a
    wavefront has lanes (the smallest batch that leaves the one-load-per-lane form of the tile sums)."""
    _need_gpu()
    d, prefix, spans = _periodic(n)
    total = int(prefix[n].item())
    assert (n + 63) // 64 - 1 == (n - 1) // 64 and ((n - 1) // 64) // _SCAN_TILE == (1 if n < (1 << 20) else 65)
    pre, sp, tot = _findall(PAT, d, 16, None, 1, total + 3)
    assert tot == total
    assert torch.equal(pre, prefix)
    assert torch.equal(sp[:tot], spans)


# ---- the other instantiations that share the header --------------------------------------------------------------

def test_256_byte_texts_take_the_2048_span_tile():
    _need_gpu()
    _check(b"\\d+", make_digits_batch(200, 256, device="cuda").cpu().numpy(), length=256, both=True)


def test_1040_byte_texts_take_sixteen_byte_records():
    _need_gpu()
    _check(PAT, make_c2_batch(130, 1040, seed=20261019, device="cuda").cpu().numpy(), length=1040, both=True)


def test_ragged_fixed_pitch_batch_with_lens():
    _need_gpu()
    n = 300
    rows = make_c2_batch(n, 1024, seed=20261020, device="cuda").cpu().numpy()
    lens = [(37 * i) % 1025 for i in range(n)]
    lens[n - 1] = 0
    _check(PAT, rows, lens=lens, both=True)


def test_literal_takes_the_fixed_length_form():
    _need_gpu()
    rows = _random_rows(130, 1024, 77, alphabet=b"helo wrd")
    rows[:, 1019:] = np.frombuffer(b"hello", dtype=np.uint8)
    assert _check(b"hello", rows, length=1024, both=True) >= 130


def test_multi_pass_and_dense_wavefronts_behind_a_scalar_branch():
    """Digits-only runs under \\d in 1 KiB texts (3072-span tile): wavefront 0 is sparse (lean pass), wavefront 1 holds
    64 x 50 = 3200 spans (two passes of the tile loop), wavefront 2 holds 64 x 150 = 9600 (above 3 tiles: the dense
    path), wavefront 3 is one sparse text."""
    _need_gpu()
    rows = np.full((193, 1024), ord(" "), dtype=np.uint8)
    digits = np.frombuffer(b"0123456789" * 15, dtype=np.uint8)
    rows[0:64:5, 7:10] = digits[:3]
    rows[64:128, 3:53] = digits[:50]
    rows[128:192, 500:650] = digits
    rows[192, 1020:1024] = digits[:4]
    assert _check(b"\\d", rows, length=1024, both=True) == 13 * 3 + 3200 + 9600 + 4


# ---- base --------------------------------------------------------------------------------------------------------

def test_split_findall_adds_the_first_half_through_base():
    """mrx_debug_split_findall(1) at the split's minimum size: the second half's decode takes the spans in front of it
    from `base`.  Bit-equal to the unsplit call."""
    _need_gpu()
    lib = M.load_library()
    n = (1 << 18) + 65
    d, prefix, spans = _periodic(n)
    total = int(prefix[n].item())
    batch = M.DeviceBatch.strided(d.reshape(-1), 16, length=16)
    rx = M.compile_regex(PAT)
    pre0, sp0, tot0 = rx._dev_findall(batch, span_cap=total + 3)
    lib.mrx_debug_split_findall(1)
    try:
        pre1, sp1, tot1 = rx._dev_findall(batch, span_cap=total + 3)
    finally:
        lib.mrx_debug_split_findall(0)
    assert tot0 == tot1 == total
    assert torch.equal(pre0, prefix) and torch.equal(sp0[:total], spans)
    assert torch.equal(pre1, pre0) and torch.equal(sp1[:total], sp0[:total])


# ---- capacity ----------------------------------------------------------------------------------------------------

def test_capacity_seven_below_the_total():
    """prefix and the total are complete, the spans up to the capacity exact, the words behind the buffer untouched."""
    _need_gpu()
    n = 129
    rows = _random_rows(n, 32, 4242)
    counts, osp, ototal = _oracle(PAT, rows, [32] * n)
    cap = ototal - 7
    assert cap > 0
    lib = M.load_library()
    rx = M.compile_regex(PAT)
    d = torch.from_numpy(rows).cuda()
    batch = M.DeviceBatch.strided(d.reshape(-1), 32, length=32)
    for lean in (1, 0):
        pre = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        buf = torch.full((ototal, 2), -5, dtype=torch.int32, device="cuda")   # (the call is told of `cap` rows only)
        total = C.c_int64(0)
        try:
            lib.mrx_debug_decode_lean(lean)
            rc = batch.call(lib, "mrx_findall", (rx._h,), (M.api._ptr(pre), M.api._ptr(buf), cap, C.byref(total), rx._stream_ptr()))
            torch.cuda.synchronize()
            assert lib.mrx_last_kernel_name() == b"k_stream_findall" and lib.mrx_debug_last_decode_lean() == lean
        finally:
            lib.mrx_debug_decode_lean(_LEAN_DEFAULT)
        assert rc == M.api.MRX_E_CAPACITY and int(total.value) == ototal == int(pre[n].item())
        assert np.array_equal((pre[1:] - pre[:-1]).cpu().numpy(), counts)
        assert np.array_equal(buf[:cap].cpu().numpy(), osp[:cap])
        assert bool((buf[cap:] == -5).all())
