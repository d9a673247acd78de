"""captures_all on the GPU (mrx_captures_all_*, CompiledRegex.captures_all) against the loop of sub() with a group
template restated from the oracle (tests/captures_all_expect.py), across its three routes and the batch layouts."""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mojo_regex_amd as M  # noqa: E402
from mojo_regex_amd.api import MRX_E_ARGUMENT, MRX_E_CAPACITY, _ptr  # noqa: E402
from mrx_ref import hybrid as O  # noqa: E402  (oracle: checker only)
import captures_all_expect as E  # noqa: E402
import layouts as LY  # noqa: E402
from bench_engine_cases import CASES as BENCH_CASES  # noqa: E402
from test_gpu_parity import generic_kernels  # noqa: E402
from capall_gen import KERNEL, route_of  # noqa: E402

FIXED = E.FIXED_PATTERNS
PATTERNS = [p for p, _ in E.GROUP_PATTERNS] + list(dict.fromkeys(p for p, _ in E.CHAIN_SUBS)) + FIXED


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _texts(pat: bytes, n: int = 160, seed: int = 0):
    rng = np.random.default_rng(zlib.crc32(pat) + seed)
    al = np.frombuffer(b"abcxyz0123456789 -.@helowrdHW_\t,+" + bytes(c for c in pat if chr(c).isalnum()) * 2, np.uint8)
    out = [bytes(rng.choice(al, size=int(rng.integers(0, 60))).tolist()) for _ in range(n)]
    out += [bytes(rng.choice(al, size=int(rng.integers(1, 4097))).tolist()) for _ in range(24)]
    out += [bytes(rng.choice(al, size=int(rng.integers(4097, 6000))).tolist()) for _ in range(3)]
    out += [b"", b"6502530000", b"Call 6502530000 or 4155551234 today.", b"2026-04-12 and 2025-12-25", b"hello world foo",
            b"x", b"x1x", b"abcd", b"acd", b"a"]
    tw = O.compile_regex(pat).fixed_total_width
    if tw > 0:
        digits = np.frombuffer(b"0123456789", np.uint8)
        out += [bytes(rng.choice(digits, size=tw).tolist()) for _ in range(6)] + [b"1" * (tw - 1) + b"a"]
    return out


def _rows_of(prefix, groups, i):
    return [[tuple(int(x) for x in pr) for pr in r] for r in groups[int(prefix[i]):int(prefix[i + 1])]]


def _check(pat, texts, count, prefix, groups, g, cache=None):
    """cache: (count, text) -> the oracle's rows (None where its loop does not end), for a second batch of the same texts"""
    prefix = np.asarray(prefix)
    groups = np.asarray(groups)
    assert prefix.shape == (len(texts) + 1,) and groups.shape == (int(prefix[-1]), g + 1, 2)
    checked = 0
    for i, t in enumerate(texts):
        if cache is not None and (count, t) in cache:
            want = cache[count, t]
        else:
            try:
                want = E.expected_rows(pat, t, count, g)
            except O.ReferenceDoesNotTerminate:
                want = None
            if cache is not None:
                cache[count, t] = want
        if want is None:
            continue
        assert _rows_of(prefix, groups, i) == want, (pat, count, i, t[:80])
        checked += 1
    assert checked > len(texts) // 2


@pytest.mark.parametrize("pat", PATTERNS)
def test_captures_all_matches_subs_loop(pat):
    _need_gpu()
    rx = M.compile_regex(pat)
    g = rx.num_groups
    texts = _texts(pat)
    short = [t for t in texts if len(t) <= 4096]   # (without a text beyond the chain kernel's tile: the plan's own route)
    assert len(short) == len(texts) - 3
    lib = M.load_library()
    cache = {}
    for count in (0, 1, 3):
        prefix, groups = rx.captures_all(texts, count)
        _check(pat, texts, count, prefix, groups, g, cache)
        p2, g2 = rx.captures_all(M.DeviceBatch.from_texts(short), count)
        assert lib.mrx_last_kernel_name() == KERNEL[route_of(rx.describe())], (pat, lib.mrx_last_kernel_name())
        _check(pat, short, count, p2.cpu().numpy(), g2.cpu().numpy(), g, cache)
        if count == 0:   # the first row of a text is its captures() row (outside the whole-text shortcut)
            caps = rx.captures(texts)
            orx = O.compile_regex(pat)
            for i, t in enumerate(texts):
                if orx.fixed_concat and len(t) == orx.fixed_total_width:
                    continue
                if prefix[i + 1] > prefix[i]:
                    assert (groups[prefix[i]] == caps[i]).all(), (pat, t)


@pytest.mark.parametrize("name", ["sub_group_phone_fmt", "sub_group_date_fmt", "sub_group_word_swap"])
def test_reference_benchmark_inputs(name):
    _need_gpu()
    case = next(c for c in BENCH_CASES if c.name == name)
    texts = [case.text, case.text[:1000], case.text[7:3000], b""]
    rx = M.compile_regex(case.pattern)
    for count in (0, 1, 3):
        prefix, groups = rx.captures_all(texts, count)
        _check(case.pattern, texts, count, prefix, groups, rx.num_groups)


def test_pinned_backtracker_case():
    """sub()'s loop, not findall: '(a|ab)(c|bcd)(d*)' finds nothing in "abcd" (findall: (0, 4))."""
    _need_gpu()
    prefix, groups = M.captures_all(b"(a|ab)(c|bcd)(d*)", [b"abcd", b"acd"])
    assert prefix.tolist() == [0, 0, 1]
    assert groups.tolist() == [[[0, 1], [1, 2], [2, 3], [0, 3]]]


ROUTES = [(b"(\\d{3})(\\d{3})(\\d{4})", b"k_capall_fixed"), (b"(\\d{4})-(\\d{2})-(\\d{2})", b"k_capall_fixed"),
          (b"(\\w+) (\\w+)", b"k_capall_chain"), (b"([a-z]+)-(\\d{2,4})", b"k_capall_chain"),
          (b"(a|ab)(c|bcd)(d*)", b"k_capall_emit"), (b"(\\w+)|(\\d+)", b"k_capall_emit")]


@pytest.mark.parametrize("pat,kernel", ROUTES)
def test_routes_agree_with_the_generic_kernels(pat, kernel):
    _need_gpu()
    lib = M.load_library()
    rx = M.compile_regex(pat)
    texts = [t for t in _texts(pat, seed=5) if len(t) <= 4096]
    for count in (0, 3):
        batch = M.DeviceBatch.from_texts(texts)
        p1, g1 = rx.captures_all(batch, count)
        assert lib.mrx_last_kernel_name() == kernel, (pat, lib.mrx_last_kernel_name())
        with generic_kernels():
            p2, g2 = rx.captures_all(batch, count)
            assert lib.mrx_last_kernel_name() == b"k_capall_emit"
        assert torch.equal(p1, p2) and torch.equal(g1, g2), pat
        _check(pat, texts, count, p1.cpu().numpy(), g1.cpu().numpy(), rx.num_groups)


LAYOUT_PATTERNS = [b"(\\d{3})(\\d{3})(\\d{4})", b"(\\w+) (\\w+)", b"(a|ab)(c|bcd)(d*)", b"x(\\d)?", b"(\\d+)\\.(\\d+)"]


@pytest.mark.parametrize("pat", LAYOUT_PATTERNS)
def test_layouts_and_poisoned_bytes(pat):
    _need_gpu()
    rx = M.compile_regex(pat)
    g = rx.num_groups
    texts = LY.make_texts(pat, 200, 4)
    lays = LY.layouts_for(texts, LY.pattern_poison(pat), texts[:120])
    by_texts = {}
    for lay in lays:
        prefix, groups = rx.captures_all(lay.device(), 0)
        prefix, groups = prefix.cpu().numpy(), groups.cpu().numpy()
        _check(pat, lay.texts, 0, prefix, groups, g)
        key = tuple(lay.texts)
        if key in by_texts:
            p0, g0 = by_texts[key]
            assert np.array_equal(p0, prefix) and np.array_equal(g0, groups), (pat, lay.name)
        else:
            by_texts[key] = (prefix, groups)


def _raw(rx, texts, count, cap, groups=None):
    lib = M.load_library()
    b = M.DeviceBatch.from_texts(texts)
    g = rx.num_groups
    prefix = torch.zeros(b.n + 1, dtype=torch.int64, device="cuda")
    if groups is None:
        groups = torch.full((max(cap, 1) + 4, g + 1, 2), -7, dtype=torch.int32, device="cuda")
    total = C.c_int64(-1)
    rc = lib.mrx_captures_all_dev(rx._h, _ptr(b.data), _ptr(b.offsets), b.n, count, _ptr(prefix), _ptr(groups), cap,
                                  C.byref(total), rx._stream_ptr())
    torch.cuda.synchronize()
    return rc, int(total.value), prefix, groups


@pytest.mark.parametrize("pat", [b"(\\d{3})(\\d{3})(\\d{4})", b"(\\w+) (\\w+)", b"(a|ab)(c|bcd)(d*)"])
def test_contract_edges(pat):
    _need_gpu()
    rx = M.compile_regex(pat)
    p0, g0 = rx.captures_all([], 0)
    assert p0.tolist() == [0] and g0.shape[0] == 0
    texts = _texts(pat, 60)
    prefix, groups = rx.captures_all(texts)
    need = int(prefix[-1])
    assert need > 2
    rc, total, _, buf = _raw(rx, texts, 0, need - 1)
    assert rc == MRX_E_CAPACITY and total == need
    assert (buf[need - 1:] == -7).all().item()   # nothing at or beyond the cap
    rc, total, p2, buf = _raw(rx, texts, 0, need)
    assert rc == 0 and total == need
    assert np.array_equal(p2.cpu().numpy(), prefix) and np.array_equal(buf[:need].cpu().numpy(), groups)
    assert (buf[need:] == -7).all().item()
    rc, _, _, _ = _raw(rx, texts, -1, need)
    assert rc == MRX_E_ARGUMENT


def test_refused_pattern():
    _need_gpu()
    rx = M.compile_regex(b"(" * 17 + b"a" + b")" * 17 + b"(b)")
    with pytest.raises(M.UnsupportedPattern):
        rx.captures_all([b"abc"])


def test_large_chain_batch_against_the_generic_route():
    """2^16 texts of 1 KiB on a chain pattern: bit-identical with the lane-per-text route."""
    _need_gpu()
    lib = M.load_library()
    n, L = 1 << 16, 1024
    rng = np.random.default_rng(7)
    al = np.frombuffer(b"abcdefgh xyz 0123 ", np.uint8)
    arr = torch.from_numpy(rng.choice(al, size=n * L).astype(np.uint8)).cuda()
    batch = M.DeviceBatch.strided(arr, L, length=L)
    rx = M.compile_regex(b"(\\w+) (\\w+)")
    p1, g1 = rx.captures_all(batch)
    assert lib.mrx_last_kernel_name() == b"k_capall_chain"
    with generic_kernels():
        p2, g2 = rx.captures_all(batch)
    assert torch.equal(p1, p2) and torch.equal(g1, g2)
    host = arr.cpu().numpy().reshape(n, L)
    p1 = p1.cpu().numpy()
    g1 = g1.cpu().numpy()
    for i in range(0, n, 4099):
        assert _rows_of(p1, g1, i) == E.expected_rows(b"(\\w+) (\\w+)", host[i].tobytes(), 0, 2)
