"""The stepper family's routes as data: which kernels a count / findall / sub call launches (mrx_last_kernel_name) for
one pattern of every flag family, on the smallest batch shapes that still reach every branch, under the debug knobs that
steer those branches.  Shared by tools/record_step_routes.py, which writes tests/golden/step_routes.json, and by
tests/test_gpu_step_routes.py, which holds the library to that file and every result to the oracle.

A case runs on a handle of its own (CompiledRegex, never compile_regex's cache): the route tuners keep their state in the
handle, and the first eligible calls of a fresh handle take their routes by construction."""
import ctypes as C
import contextlib
import re
import string
import zlib
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

# DevPlan::flags (csrc/mrx_plan.hpp) as mrx_describe prints them (`flags=0x...`)
PF = dict(START_ACCEPTING=1 << 5, PREFILTER=1 << 7, STREAMABLE=1 << 9, BITSET=1 << 10, STREAM_SEARCH=1 << 11,
          STEPPABLE=1 << 12, STEP_SEARCH=1 << 13, STEP_REQ=1 << 14, STEP_BIG=1 << 15, BSTEP=1 << 16, BT_FIRST=1 << 17,
          BT_SEARCH=1 << 18, STEP_EMPTY=1 << 19, MWALK=1 << 20, MWALK_REQ=1 << 21, BACKSET=1 << 22, LAZY_END=1 << 23,
          MW_EMPTY=1 << 24, MW_TRIES=1 << 25)


def plan_facts(describe: str) -> dict:
    """flags, mw_walks (DevPlan::mw_k) and the bitset program's fixed match length, from mrx_describe's text."""
    fx = re.search(r"fixed_len=(-?\d+)", describe)
    return dict(flags=int(re.search(r"flags=0x([0-9a-f]+)", describe).group(1), 16),
                mw_k=int(re.search(r"mw_walks=(-?\d+)", describe).group(1)),
                fixed_len=int(fx.group(1)) if fx else 0)


def _has(f, *names):
    return all(f["flags"] & PF[n] for n in names)


def _lacks(f, *names):
    return not any(f["flags"] & PF[n] for n in names)


# more byte classes than the backward table and the multi-walk builders take: a plain table plan and nothing else
_MANY = (string.ascii_lowercase + string.ascii_uppercase + "_!#%&<>=;,~").encode()
_PLAIN = b"[0-9]+@(?:" + b"|".join(bytes([c]) for c in _MANY) + b")"
_NANPA = (rb"(?:2(?:0[1-35-9]|1[02-9]|2[03-57-9]|3[1459]|4[08]|5[1-46]|6[0279]|7[0269]|8[13])|3(?:0[1-47-9]|1[02-9]|2[0135-79]|"
          rb"3[0-24679]|4[167]|5[0-2]|6[01349]|8[056])|4(?:0[124-9]|1[02-579]|2[3-5]|3[0245]|4[023578]|58|6[349]|7[0589]|8[04])|"
          rb"5(?:0[1-47-9]|1[0235-8]|20|3[0149]|4[01]|5[179]|6[1-47]|7[0-5]|8[0256])|6(?:0[1-35-9]|1[024-9]|2[03689]|3[016]|"
          rb"4[0156]|5[01679]|6[0-279]|78|8[0-29])|7(?:0[1-46-8]|1[2-9]|2[04-8]|3[0-247]|4[037]|5[47]|6[02359]|7[0-59]|8[156])|"
          rb"8(?:0[1-68]|1[02-8]|2[0168]|3[0-2589]|4[03578]|5[046-9]|6[02-5]|7[028])|9(?:0[1346-9]|1[02-9]|2[0589]|3[0146-8]|"
          rb"4[01357-9]|5[12469]|7[0-389]|8[04-69]))[2-9]\d{6}")


class Family(NamedTuple):
    pattern: bytes
    alphabet: bytes          # what the texts are drawn from
    member: object           # plan_facts -> bool: the plan belongs to the family
    lazy: bool = False       # compile options (lazydfa_semantics, bitset_nfa)
    bitset: bool = False
    long_shapes: bool = True  # the family has a long-text treatment (pieces, wavefront per text, split) to reach
    plant: bytes = b""       # a match the alphabet would hardly ever draw, written over some of the random bytes


# One pattern per family.  `member` is asserted through mrx_describe, so that a planner change cannot silently empty a row.
FAMILIES: Dict[str, Family] = {
    "plain": Family(_PLAIN, b"0123456789@abXY_! ",
                    lambda f: _has(f, "STEPPABLE") and _lacks(f, "STREAMABLE", "BACKSET", "MWALK", "MW_TRIES", "STEP_BIG", "BSTEP", "LAZY_END")),
    "plain_backset": Family(b"[a-c]{17}[d-f]", b"abcabcabcd ",
                            lambda f: _has(f, "STEPPABLE", "BACKSET") and _lacks(f, "STREAMABLE", "MWALK", "MW_TRIES", "STEP_BIG"),
                            plant=b"abcabcabcabcabcabcabcde"),
    "step_big": Family(_NANPA, b"0123456789 ", lambda f: _has(f, "STEPPABLE", "STEP_BIG")),
    "req_mwalk": Family(b"\\d{3}-\\d{4}", b"abcxyz0189 -555-1234", lambda f: _has(f, "STEP_REQ", "MWALK_REQ")),
    "req_plain": Family(b"\\d+-[0-9-]{8}x", b"0123456789--x ab", lambda f: _has(f, "STEP_REQ") and _lacks(f, "MWALK_REQ"),
                        plant=b"12-3456-789x"),
    "mwalk": Family(b"\\d+(\\.\\d+)?", b"0123456789.. abc", lambda f: _has(f, "STEPPABLE", "MWALK")),
    "tries": Family(b"foo|[a-z]{3}\\d|[ab]", b"abcfoxyz0123 -", lambda f: _has(f, "STEPPABLE", "MW_TRIES", "BACKSET")),
    "step_empty": Family(b"(ab){9}|x*", b"abx ab", lambda f: _has(f, "STEP_EMPTY") and _lacks(f, "MW_EMPTY"), long_shapes=False),
    "mw_empty_1": Family(b"a*", b"aab x", lambda f: _has(f, "MW_EMPTY") and f["mw_k"] == -1, long_shapes=False),
    "mw_empty_2": Family(b"ca*t", b"caat x", lambda f: _has(f, "MW_EMPTY") and f["mw_k"] == -2, long_shapes=False),
    "bstep_fixed10": Family(b"(\\d{3})(\\d{3})(\\d{4})", b"0123456789 -", lambda f: _has(f, "BSTEP") and f["fixed_len"] >= 4,
                            lazy=True, bitset=True, long_shapes=False),
    "bstep_fixed2": Family(b"(a|b)x", b"abx ", lambda f: _has(f, "BSTEP") and 0 < f["fixed_len"] < 4, bitset=True, long_shapes=False),
    "bstep_loop": Family(b"(ab)+c", b"abc ", lambda f: _has(f, "BSTEP") and f["fixed_len"] == 0, bitset=True, long_shapes=False),
    "lazy_end": Family(b"(foo|bar)$", b"fobar ", lambda f: _has(f, "STEPPABLE", "LAZY_END"), long_shapes=False, plant=b"foo"),
    "backtracker": Family(b"hello.*", b"helo wrd", lambda f: _has(f, "BT_SEARCH") and _lacks(f, "STREAMABLE"), long_shapes=False, plant=b"hello"),
    "streamable": Family(b"[a-z]+\\d+", b"abcxyz0189 -", lambda f: _has(f, "STREAMABLE", "STEPPABLE"), long_shapes=False),
    # sub's match_next sequence on a memchr-prefiltered plan
    "req_prefilter": Family(b"\\w+@\\w+\\.com", b"abc@.com xy1", lambda f: _has(f, "STEP_REQ", "PREFILTER"), long_shapes=False, plant=b"ab@xy.com"),
}

SHAPES = ("csr320", "pitch320", "long6", "ragged")
PITCH = 208


def texts_for(family: str, shape: str, alphabet: bytes = None) -> List[bytes]:
    """csr320 / pitch320: 320 texts of 0..200 bytes (at least 256, so the tuners are eligible; five wavefronts with a
    ragged tail).  long6: 6 texts of 40000 bytes (pieces, the wavefront kernel).  ragged: the 320 and 2 texts of 40000
    bytes (longest >= 32768 and >= 8 x the average: step_split = 16384)."""
    al = np.frombuffer(alphabet or FAMILIES[family].alphabet, dtype=np.uint8)
    rng = np.random.default_rng(zlib.crc32(family.encode()))

    plant = b"" if alphabet else FAMILIES[family].plant

    def draw(k):
        t = bytearray(rng.choice(al, size=int(k)).tolist())
        if plant and len(t) >= len(plant) and rng.integers(0, 3) == 0:   # one in three: at the end, or anywhere
            for at in ([len(t) - len(plant)] if rng.integers(0, 2) else rng.integers(0, len(t) - len(plant) + 1, size=1 + len(t) // 400)):
                t[at:at + len(plant)] = plant
        return bytes(t)
    lens = rng.integers(0, 201, size=320)
    lens[:3] = [0, 1, 200]
    short = [draw(k) for k in lens]
    if shape in ("csr320", "pitch320"):
        return short
    longs = [draw(40000) for _ in range(6)]
    return longs if shape == "long6" else short + longs[:2]


def make_batch(M, torch, shape: str, texts: List[bytes]):
    if shape != "pitch320":
        return M.DeviceBatch.from_texts(texts)
    arr = np.zeros((len(texts), PITCH), np.uint8)
    for i, t in enumerate(texts):
        arr[i, :len(t)] = np.frombuffer(t, np.uint8)
    lens = torch.tensor([len(t) for t in texts], dtype=torch.int32, device="cuda")
    return M.DeviceBatch.strided(torch.from_numpy(arr).cuda().reshape(-1), PITCH, length=PITCH, lens=lens)


class Case(NamedTuple):
    family: str
    shape: str
    op: str                  # count | findall | findall0 (span_cap == 0) | sub (mrx_sub_dev: match_next_sequence)
    long_text: int = 0       # mrx_debug_long_text_kernels
    multiwalk: int = 0       # mrx_debug_multiwalk
    generic: int = 0         # mrx_debug_force_generic
    tries_always: int = 0    # mrx_debug_tries_always
    calls: int = 1           # > 1: a tuner case -- the same call again on the same handle
    alphabet: bytes = None   # instead of the family's

    @property
    def id(self) -> str:
        s = "%s/%s/%s" % (self.family, self.shape, self.op)
        for k in ("long_text", "multiwalk", "generic", "tries_always"):
            if getattr(self, k):
                s += "/%s=%d" % (k, getattr(self, k))
        if self.calls > 1:
            s += "/x%d" % self.calls
        if self.alphabet:
            s += "/" + self.alphabet.decode()
        return s


def _cases() -> List[Case]:
    out: List[Case] = []
    steppers = ("plain", "plain_backset", "step_big", "req_mwalk", "req_plain", "mwalk", "tries")
    for fam, f in FAMILIES.items():
        if fam == "req_prefilter":
            continue
        ta = 1 if fam == "tries" else 0   # (without it the tuner's alternation decides: the tuner cases below)
        for shape in ("csr320", "pitch320"):
            for op in ("count", "findall"):
                out.append(Case(fam, shape, op, tries_always=ta))
        out.append(Case(fam, "csr320", "findall0", tries_always=ta))
        if f.long_shapes:
            for op in ("count", "findall"):
                for lt in (0, 1, 2, 3):
                    out.append(Case(fam, "long6", op, long_text=lt, tries_always=ta))
                out.append(Case(fam, "ragged", op, tries_always=ta))
            out.append(Case(fam, "long6", "findall0", tries_always=ta))
        else:
            for op in ("count", "findall"):   # families without a long-text treatment: that they have none
                out.append(Case(fam, "long6", op))
    # no multi-walk forms, no marks, no fixed-length union pass
    for fam in ("plain_backset", "step_big", "req_mwalk", "mwalk", "tries", "mw_empty_1", "mw_empty_2", "bstep_fixed10", "bstep_fixed2"):
        for op in ("count", "findall"):
            out.append(Case(fam, "csr320", op, multiwalk=2))
    for fam in ("req_mwalk", "mwalk", "plain_backset"):
        for op in ("count", "findall"):
            out.append(Case(fam, "long6", op, multiwalk=2))
            out.append(Case(fam, "ragged", op, multiwalk=2))
    # the stepper and nothing newer (1), the literal restatement (2)
    for fam in ("streamable", "plain_backset", "mwalk", "req_mwalk", "step_empty", "mw_empty_1", "bstep_fixed10", "backtracker", "step_big"):
        for g in (1, 2):
            for op in ("count", "findall"):
                out.append(Case(fam, "csr320", op, generic=g))
    for op in ("count", "findall"):
        out.append(Case("streamable", "long6", op, generic=1))
        out.append(Case("streamable", "long6", op, generic=1, long_text=1))
    # sub's match_next sequence: a plain plan and a prefiltered one
    for fam in ("mwalk", "req_prefilter", "req_mwalk", "step_empty"):
        out.append(Case(fam, "csr320", "sub"))
    out.append(Case("mwalk", "long6", "sub"))
    out.append(Case("req_prefilter", "csr320", "count"))
    out.append(Case("req_prefilter", "csr320", "findall"))
    # ---- tuners: calls 1-4 take routes 1, 2, 1, 2; from call 5 on the clock decides ----
    for shape in ("csr320", "pitch320"):
        out.append(Case("tries", shape, "findall", calls=6))
        out.append(Case("tries", shape, "count", calls=6))
    out.append(Case("tries", "csr320", "findall+count", calls=8))   # (their keys differ by bit 29: each starts at route 1)
    out.append(Case("req_mwalk", "long6", "findall", calls=6))                        # synchronising bytes everywhere
    out.append(Case("req_mwalk", "long6", "findall", calls=6, alphabet=b"0123456789-"))   # none: the wavefront kernel for good
    out.append(Case("req_mwalk", "long6", "count", calls=3))                          # (count is not tuned)
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return out


CASES: List[Case] = _cases()
SUB_REPL = b"<#>"


@contextlib.contextmanager
def knobs(lib, case: Case):
    lib.mrx_debug_long_text_kernels(case.long_text)
    lib.mrx_debug_multiwalk(case.multiwalk)
    lib.mrx_debug_force_generic(case.generic)
    lib.mrx_debug_tries_always(case.tries_always)
    try:
        yield
    finally:
        lib.mrx_debug_long_text_kernels(0)
        lib.mrx_debug_multiwalk(0)
        lib.mrx_debug_force_generic(0)
        lib.mrx_debug_tries_always(0)


def compile_case(M, case: Case):
    f = FAMILIES[case.family]
    return M.CompiledRegex(f.pattern, f.lazy, f.bitset)   # a handle of this case's own


def ops_of(case: Case) -> List[str]:
    """The operation of each of the case's calls."""
    if case.op == "findall+count":
        return ["findall", "findall", "count", "count", "count", "count", "findall", "findall"]
    return [case.op] * case.calls


def run_case(M, torch, case: Case, batch, nbytes: int) -> Tuple[List[str], list]:
    """The case's calls on a fresh handle: ([kernel name per call], [result per call]).  A result is a list of counts
    (count, findall0), a list of span lists (findall) or a list of texts (sub)."""
    lib = M.load_library()
    rx = compile_case(M, case)
    names, results = [], []
    n = batch.n
    with knobs(lib, case):
        for op in ops_of(case):
            if op == "count":
                res = rx.count(batch).cpu().tolist()
            elif op == "findall":
                pre, sp, tot = rx._dev_findall(batch, span_cap=nbytes + n + 64)   # room for every span: no retry
                pre, sp = pre.cpu().numpy(), sp[:tot].cpu().numpy()
                res = [[(int(a), int(b)) for a, b in sp[pre[i]:pre[i + 1]]] for i in range(n)]
            elif op == "findall0":
                prefix = torch.empty(n + 1, dtype=torch.int64, device="cuda")
                total = C.c_int64(-1)
                rc = batch.call(lib, "mrx_findall", (rx._h,), (C.c_void_p(prefix.data_ptr()), None, 0, C.byref(total), rx._stream_ptr()))
                assert rc in (M.api.MRX_OK, M.api.MRX_E_CAPACITY), rc
                assert (rc == M.api.MRX_OK) == (total.value == 0)
                prefix = prefix.cpu().numpy()
                assert prefix[0] == 0 and prefix[n] == total.value
                res = np.diff(prefix).tolist()
            else:
                off, out = rx.sub_dev(SUB_REPL, batch)
                off, out = off.cpu().numpy(), out.cpu().numpy().tobytes()
                res = [out[off[i]:off[i + 1]] for i in range(n)]
            names.append(lib.mrx_last_kernel_name().decode())
            torch.cuda.synchronize()
            results.append(res)
    return names, results
