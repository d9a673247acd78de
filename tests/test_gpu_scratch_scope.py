"""Per-call device scratch belongs to the call's scope: whichever way an entry point returns, answered or refused, no
byte of the calling thread's arenas is still handed out behind it (mrx_debug_scratch_in_use() == 0).

The calls are those of tests/scratch_matrix.py: every entry point on a CSR batch of 130 texts, 128 x 64 and 64 x 2048
bytes at a fixed pitch, the routes forced with the testing switches, sub's two retries and the refused calls.  Each call's
result is compared with the oracle, so a call that leaves the arena clean by doing nothing does not pass."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mojo_regex_amd as M  # noqa: E402

import scratch_matrix as SM  # noqa: E402

CASES = SM.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_nothing_is_in_use_behind_the_call(case):
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path has no fallback")
    lib = M.load_library()
    assert lib.mrx_debug_scratch_in_use() == 0, "in use before the call"
    with SM.switched(case.switch):
        case.run(True)
    assert lib.mrx_debug_scratch_in_use() == 0, case.name


def test_released_arenas_hold_nothing():
    lib = M.load_library()
    torch.cuda.synchronize()
    lib.mrx_release_scratch()
    assert lib.mrx_debug_scratch_in_use() == 0 and lib.mrx_debug_scratch_bytes() == 0
