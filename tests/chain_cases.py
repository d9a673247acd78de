"""The cases that tests/test_gpu_chains.py and tests/test_gpu_known_bounds.py share: two corpora, every operation that
MAKES a batch on the device (the producers) and every public operation that TAKES one (the consumers), each with its
host expectation.

Host-only: numpy, the oracle and the existing *_expect.py modules; nothing is computed here a second time.  A device call
is a function of (H, batch) -- or, for a producer, of (H, texts, batch) -- where H is a Handles object that the GPU
modules build once: it is the only place that imports torch and the product library, and only when it is constructed.
tests/test_chain_cases_host.py checks this module alone, through the expectations.
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Sequence, Tuple

import numpy as np

import captures_all_expect as CAX
import distinct_expect as DX
import expand_expect as EX
import extract_expect as XX
import fields_expect as FDX
import filter_expect as FX
import format_expect as FMX
import keywords_expect as KX
import kw_sub_expect as KSX
import layouts as LY
import lines_expect as LNX
import lookup_expect as LX
import parse_expect as PX
import set_findall_expect as SFX
import set_sub_expect as SSX
import sort_expect as SX
import translate_expect as TX
from mrx_ref import hybrid as O

# ---- the parameters of every call ------------------------------------------------------------------------------------
STREAM = b"[a-z]+\\d+"          # streamable: byte columns
STEP = b"\\w+\\d{2}"            # stepper, multi-walk
GROUPS = b"(\\w+) (\\w+)"       # general groups
NUM = b"\\d+"                   # streamable: numbers and split
OPT = b"x(\\d)?"                # fixed-width groups: group 1 is unset in "xy"
KEEP = b"hello"                 # a pure literal: filter's pattern
PATTERNS = (STREAM, STEP, GROUPS, NUM, OPT, KEEP)
assert all(p in LY.PATTERNS for p in PATTERNS)
CONSUMER_PATTERNS = (STREAM, STEP, GROUPS)
SET = [STREAM, NUM, KEEP]
SET_REPLS = [b"", b"#", b"<h>"]
SUB_REPL = {STREAM: b"", STEP: b"<#>", GROUPS: b"\\2 \\1"}
TEMPLATE = b"<\\2:\\1>"
KW = [b"error", b"timeout", b"GET", b"err", b"web1", b"Alice"]
KW_REPL = b"<K>"
FMT = b"[\\1|\\2]\n"
DELETE, SQUEEZE = b"aeiou\r", b" "
WS_COLUMNS, DELIM_COLUMNS, CUT_COLUMNS = [1, 3, -1], [2, -1], [1, 3]


# ---- the corpora -----------------------------------------------------------------------------------------------------
def _line(rng) -> bytes:
    method = [b"GET", b"POST", b"HEAD", b"get"][int(rng.integers(0, 4))]
    path = [b"a", b"bb", b"ccc", b"x7", b"xy"][int(rng.integers(0, 5))]
    user = [b"Alice", b"bob7", b"carol", b"Dave42"][int(rng.integers(0, 4))]
    msg = [b"ok", b"error timeout", b"hello world", b"Warn  disk", b"error", b""][int(rng.integers(0, 6))]
    return b"%s /item%d/%s %d host=web%d, user=%s  %s" % (method, int(rng.integers(0, 9)), path, int(rng.integers(200, 504)),
                                                         int(rng.integers(1, 30)), user, msg)


def _long(rng, size: int) -> bytes:
    parts, have = [], 0
    while have < size:
        parts.append(_line(rng) + (b"\r\n" if rng.random() < 0.2 else b"\n"))
        have += len(parts[-1])
    return b"".join(parts)[:size]


def _base() -> List[bytes]:
    rng = np.random.default_rng(20261021)
    fixed = [b"", b"", b"", b"   ", b" \t ", b"42", b"-17", b" 8 ", b"3.5", b"0x1f", b"bob7", b"abc123", b"  hello  ", b"hello",
             b"GET", b"\n\n", b"a,b,c", b",", b"one two", b"error", b"x7 xy x", b"Alice", b"1,,2\n", b"no newline at the end"]
    texts = list(fixed) + [b"42", b"hello", b"GET", b"bob7", b"error"]          # repeats: distinct, sort ties
    while len(texts) < 146:
        k = int(rng.integers(1, 5))
        t = b"\n".join(_line(rng) for _ in range(k)) + (b"\n" if rng.random() < 0.5 else b"")
        if rng.random() < 0.15:
            t = t.replace(b"\n", b"\n\n", 1)                                       # an empty line
        texts.append(t[:300])
    order = rng.permutation(len(texts))
    texts = [texts[int(k)] for k in order]
    for at, size in ((3, 5000), (40, 9000), (90, 17000), (140, 20000)):          # above 4096, and above 16 KiB
        texts.insert(at, _long(rng, size))
    return texts


BASE = _base()
SHORT = [t for t in BASE if len(t) <= 300]     # the same texts without the four long ones: every route limit is a legal bound
DEGENERATE = {
    "no_texts": [],
    "one_empty": [b""],
    "empties70": [b""] * 70,
    "nothing": [b"~~~", b"#", b"~#~#", b"##~"] * 8,     # no letter, digit, blank, comma or newline: nothing is kept or found
}
CORPORA = dict(DEGENERATE, base=BASE)
DICT = [b"", b"GET", b"hello", b"42", b"error", b"bob7", b"abc123", b"web12", b"Alice"] + BASE[10:40:3] + [b"GET"]


# ---- the oracle, once per (pattern, text) ---------------------------------------------------------------------------
_FINDALL, _TEST = {}, {}


def findall(pat: bytes, t: bytes) -> List[Tuple[int, int]]:
    return XX.findall_rows(pat, [t], _FINDALL)[0]


def _i32(rows, width) -> np.ndarray:
    return np.array(rows, dtype=np.int32).reshape((-1,) + width)


def _prefix(counts) -> np.ndarray:
    p = np.zeros(len(counts) + 1, dtype=np.int64)
    if len(counts):
        np.cumsum(counts, out=p[1:])
    return p


def findall_arrays(pat, T):
    rows = [findall(pat, t) for t in T]
    return _prefix([len(r) for r in rows]), _i32([s for r in rows for s in r], (2,))


def span_arrays(fn, pat, T):
    got = [fn(pat, t) or (-1, -1) for t in T]
    return np.array([g[0] for g in got], np.int32), np.array([g[1] for g in got], np.int32)


def split_arrays(pat, T):
    rows = [LY.split_ranges(findall(pat, t), len(t), 0) for t in T]
    return _prefix([len(r) for r in rows]), _i32([s for r in rows for s in r], (2,))


def captures_arrays(pat, T):
    g = CAX.num_groups(pat)
    rows = [CAX.expected_rows(pat, t, 0, g) for t in T]
    return _prefix([len(r) for r in rows]), _i32([m for r in rows for m in r], (g + 1, 2))


def packed(texts: Sequence[bytes]):
    return SX.packed(texts)


def flat(lists) -> List[bytes]:
    return [p for row in lists for p in row]


def take_index(n: int) -> np.ndarray:
    """Every second text, then a quarter of them again in reverse: repeats, and texts that are never taken."""
    even = np.arange(0, n, 2, dtype=np.int64)
    return np.concatenate([even, even[::-1][:n // 4]])


def ragged(T):
    """The texts at a fixed pitch with lens, every row's tail filled with the corpus's own bytes."""
    own = (b"".join(T) or b"~") * 2
    return LY.ragged_rows(T, True, lambda i, t, k: (own[i % len(own):] + own * (k // len(own) + 1))[:k])


# ---- the handles of the device calls: the only place that loads torch and the library -------------------------------
class Handles:
    def __init__(self):
        import torch
        import mojo_regex_amd as M
        self.torch, self.M = torch, M
        self.rx = {p: M.compile_regex(p) for p in PATTERNS}
        self.set = M.compile_set(SET)
        self.dict = M.Dictionary(DICT)
        self.kw = M.Keywords(KW)

    def dev(self, a):
        return self.torch.from_numpy(np.array(a)).cuda()

    def strided(self, T):
        return ragged(T).device()


class Producer(NamedTuple):
    name: str
    covers: Tuple[str, ...]                                # the public methods it runs
    device: Callable                                       # (H, texts, batch) -> DeviceBatch
    expect: Callable[[Sequence[bytes]], List[bytes]]       # texts -> the result's texts
    can_empty: bool                                        # can the operation yield an empty text?


def _kw_kept(T):
    idx, _, _ = KX.filtered(KX.findall(KW, T), T)
    return [T[int(i)] for i in idx]


def _dict_kept(T):
    return [bytes(T[int(i)]) for i in LX.filtered(DICT, T)[0]]


def _joined_lines(T, **opts):
    return LNX.lines(b"".join(T), **opts)[0]


def _from_lines(H, T, b, **opts):
    # the packed bytes of the batch as one buffer: a batch made by from_texts holds exactly that buffer as its data
    return H.M.DeviceBatch.from_lines(b.data, **opts)


PRODUCERS = [
    Producer("filter", ("CompiledRegex.filter",), lambda H, T, b: H.rx[KEEP].filter(b)[0],
             lambda T: FX.expected_lists([KEEP], T, cache=_TEST)[0], False),
    Producer("set_filter", ("PatternSet.filter",), lambda H, T, b: H.set.filter(b)[0],
             lambda T: FX.expected_lists(SET, T, cache=_TEST)[0], False),
    Producer("dict_filter", ("Dictionary.filter",), lambda H, T, b: H.dict.filter(b)[0], _dict_kept, True),
    Producer("kw_filter", ("Keywords.filter",), lambda H, T, b: H.kw.filter(b)[0], _kw_kept, False),
    Producer("extract", ("CompiledRegex.extract",), lambda H, T, b: H.rx[STREAM].extract(b)[0],
             lambda T: flat(XX.lists(XX.expected_findall(STREAM, T, _FINDALL))), False),
    Producer("extract_group", ("CompiledRegex.extract", "DeviceBatch.gather_spans"), lambda H, T, b: H.rx[OPT].extract(b, group=1)[0],
             lambda T: flat(XX.lists(XX.expected_group(OPT, T, 1))), True),
    Producer("split_batch", ("CompiledRegex.split_batch", "DeviceBatch.gather_spans"), lambda H, T, b: H.rx[NUM].split_batch(b)[0],
             lambda T: flat(XX.lists(XX.expected_split(NUM, T, 0, _FINDALL))), True),
    Producer("expand", ("CompiledRegex.expand",), lambda H, T, b: H.rx[GROUPS].expand(TEMPLATE, b)[0],
             lambda T: flat(EX.lists(EX.expected(GROUPS, TEMPLATE, T))), False),
    Producer("distinct", ("DeviceBatch.distinct",), lambda H, T, b: b.distinct()[0], lambda T: DX.values(DX.expected(T)), True),
    Producer("sort", ("DeviceBatch.sort", "DeviceBatch.argsort", "DeviceBatch.take"), lambda H, T, b: b.sort()[0],
             lambda T: sorted(T), True),
    Producer("take", ("DeviceBatch.take",), lambda H, T, b: b.take(H.dev(take_index(len(T)))),
             lambda T: SX.take(T, take_index(len(T))), True),
    Producer("lines", ("DeviceBatch.lines",), lambda H, T, b: b.lines()[0], lambda T: flat(LNX.lines(t)[0] for t in T), True),
    Producer("from_lines", ("DeviceBatch.from_lines",), lambda H, T, b: _from_lines(H, T, b), _joined_lines, True),
    Producer("from_lines_keepends", ("DeviceBatch.from_lines",), lambda H, T, b: _from_lines(H, T, b, keepends=True),
             lambda T: _joined_lines(T, keepends=True), False),
    Producer("lower", ("DeviceBatch.lower", "DeviceBatch.translate"), lambda H, T, b: b.lower(),
             lambda T: [TX.translate(t, TX.LOWER) for t in T], True),
    Producer("lower_strided", ("DeviceBatch.lower", "DeviceBatch.translate"), lambda H, T, b: H.strided(T).lower(),
             lambda T: [TX.translate(t, TX.LOWER) for t in T], True),
    Producer("translate_delete", ("DeviceBatch.translate",), lambda H, T, b: b.translate(delete=DELETE),
             lambda T: [TX.translate(t, None, DELETE) for t in T], True),
    Producer("translate_squeeze", ("DeviceBatch.translate",), lambda H, T, b: b.translate(TX.TAB_TO_SPACE, squeeze=SQUEEZE),
             lambda T: [TX.translate(t, TX.TAB_TO_SPACE, b"", SQUEEZE) for t in T], True),
    Producer("strip", ("DeviceBatch.strip", "DeviceBatch.gather_spans"), lambda H, T, b: b.strip(),
             lambda T: [t.strip() for t in T], True),
    Producer("kw_sub", ("Keywords.sub", "Keywords.subn"), lambda H, T, b: H.kw.sub(KW_REPL, b),
             lambda T: KSX.sub(KW, KW_REPL, T)[0], True),
    Producer("format_records", (), lambda H, T, b: H.M.format_records(FMT, [b, H.dev(np.arange(len(T), dtype=np.int64))]),
             lambda T: FMX.records(FMT, [T, (list(range(len(T))), "d")])[0], False),
    Producer("sub_dev", ("CompiledRegex.sub_dev",),
             lambda H, T, b: (lambda r: H.M.DeviceBatch(r[1], r[0]))(H.rx[STREAM].sub_dev(SUB_REPL[STREAM], b)),
             lambda T: [O.sub(STREAM, SUB_REPL[STREAM], t) for t in T], True),
    Producer("set_sub", ("PatternSet.sub",), lambda H, T, b: (lambda r: H.M.DeviceBatch(r[1], r[0]))(H.set.sub(SET_REPLS, b)),
             lambda T: SSX.expected_lists(SET, SET_REPLS, T, 0, _FINDALL)[0], True),
]


# ---- consumers -------------------------------------------------------------------------------------------------------
class Consumer(NamedTuple):
    name: str
    covers: Tuple[str, ...]
    device: Callable      # (H, batch) -> a tuple of tensors, DeviceBatches and ints: every defined output
    expect: Callable      # texts -> the same outputs as numpy arrays and ints (a DeviceBatch as offsets, data)
    hit: Callable         # (expectation, texts) -> one flag per text or row: the corpus must give some of each
    limit: int = 0        # > 0: the host expectation affords texts of at most this many bytes (the output is a CSR of rows
                          # over the texts: longer texts are held to the from_texts run alone)


def _some(prefix_at=0):
    return lambda e, T: np.diff(e[prefix_at]) > 0


CAPTURES_LIMIT = 1024


def _per_pattern(p) -> List[Consumer]:
    tag = {STREAM: "stream", STEP: "step", GROUPS: "groups"}[p]
    orx = O.compile_regex(p)
    return [
        Consumer("findall_" + tag, ("CompiledRegex.findall", "CompiledRegex.match_all"),
                 lambda H, b: (lambda r: (r[0], r[1][:r[2]], r[2]))(H.rx[p].findall(b)),
                 lambda T: (lambda e: e + (len(e[1]),))(findall_arrays(p, T)), _some()),
        Consumer("count_" + tag, ("CompiledRegex.count",), lambda H, b: (H.rx[p].count(b),),
                 lambda T: (np.array([len(findall(p, t)) for t in T], np.int32),), lambda e, T: e[0] > 0),
        Consumer("search_" + tag, ("CompiledRegex.search", "CompiledRegex.match_next", "CompiledRegex.test"),
                 lambda H, b: H.rx[p].search(b) + (H.rx[p].test(b),),
                 lambda T: (lambda e: e + (e[0] >= 0,))(span_arrays(O.search, p, T)), lambda e, T: e[0] >= 0),
        Consumer("match_first_" + tag, ("CompiledRegex.match_first",), lambda H, b: H.rx[p].match_first(b),
                 lambda T: span_arrays(O.match_first, p, T), lambda e, T: e[0] >= 0),
        Consumer("is_match_" + tag, ("CompiledRegex.is_match",), lambda H, b: (H.rx[p].is_match(b),),
                 lambda T: (np.array([bool(orx.is_match(t)) for t in T], np.uint8),), lambda e, T: e[0] > 0),
        Consumer("sub_dev_" + tag, ("CompiledRegex.sub_dev",), lambda H, b: H.rx[p].sub_dev(SUB_REPL[p], b),
                 lambda T: packed([O.sub(p, SUB_REPL[p], t) for t in T]),
                 lambda e, T: np.array([len(findall(p, t)) > 0 for t in T])),
        Consumer("split_dev_" + tag, ("CompiledRegex.split_dev",),
                 lambda H, b: (lambda r: (r[0], r[1][:r[2]], r[2]))(H.rx[p].split_dev(b)),
                 lambda T: (lambda e: e + (len(e[1]),))(split_arrays(p, T)), lambda e, T: np.diff(e[0]) > 1),
        Consumer("captures_all_" + tag, ("CompiledRegex.captures_all",), lambda H, b: H.rx[p].captures_all(b),
                 lambda T: captures_arrays(p, T), _some(),
                 # the reference's group loop is quadratic where its matches come from match_next: 20 KiB take 15 minutes
                 0 if p == GROUPS else CAPTURES_LIMIT),
    ]


def _set_search(T):
    s = np.full((len(T), len(SET)), -1, np.int32)
    e = s.copy()
    for i, t in enumerate(T):
        for j, p in enumerate(SET):
            w = O.search(p, t)
            if w:
                s[i, j], e[i, j] = w
    return s, e, s >= 0


def _set_extract(T):
    hits = SFX.expected_lists(SET, T, _FINDALL)
    prefix, owner, off, data = XX.pack([[(a, b) for _, a, b in row] for row in hits], T)
    return off, data, prefix, np.array([m for row in hits for m, _, _ in row], np.int32), owner


def _kept_flags(e, T):
    f = np.zeros(len(T), bool)
    f[e[2]] = True
    return f


def _numbers(T):
    rows = [findall(NUM, t) for t in T]
    pieces = [t[a:b] for t, r in zip(T, rows) for a, b in r]
    status, values = PX.expect_many(pieces, "int")
    prefix = _prefix([len(r) for r in rows])
    return values, status, prefix, np.repeat(np.arange(len(T), dtype=np.int64), np.diff(prefix))


def _parse(kind):
    def expect(T):
        status, values = PX.expect_many(T, kind)
        return values, status
    return expect


def _value_counts(T):
    rows = SX.value_counts(flat(XX.lists(XX.expected_findall(STREAM, T, _FINDALL))), "count", 10)
    return packed([v for v, _ in rows]) + (np.array([c for _, c in rows], np.int64),)


def _format(T):
    recs, status = FMX.records(FMT, [T, (list(range(len(T))), "d")])
    return packed(recs) + (status,)


def _lines(T):
    prefix, owner, off, data, totals = LNX.expected(T)
    return off, data, prefix, owner, totals[1], totals[2], totals[3]


def _fields(columns, delim):
    def expect(T):
        rows, nf, prefix = FDX.expected(T, columns, delim)
        return prefix, rows, nf
    return expect


def _cut(T):
    rows, _, _ = FDX.expected(T, CUT_COLUMNS + [1], None)
    template = b" ".join(b"\\%d" % (j + 1) for j in range(len(CUT_COLUMNS))) + b"\n"
    _, owner, off, data = EX.from_rows(template, [[[tuple(p) for p in rows[i]]] for i in range(len(T))], T)
    return off, data, owner


def _kw_sub(T):
    outs, ns = KSX.sub(KW, KW_REPL, T)
    return packed(outs) + (ns,)


def _translated(T, **args):
    off, data, totals = TX.expected(T, **args)
    return off, data, totals[0], totals[1]


def _same_length(H, res):
    """A same-length translate's result has its input's layout: its texts, read back and packed."""
    return H.M.DeviceBatch.from_texts(texts_of(res))


def texts_of(batch) -> List[bytes]:
    """The texts of a DeviceBatch, read back: CSR or fixed pitch."""
    raw = batch.data.cpu().numpy().tobytes()
    if batch.offsets is not None:
        off = batch.offsets.cpu().numpy()
        return [raw[off[i]:off[i + 1]] for i in range(batch.n)]
    lens = batch.lens.cpu().numpy() if batch.lens is not None else [batch.length] * batch.n
    return [raw[i * batch.stride:i * batch.stride + int(lens[i])] for i in range(batch.n)]


CONSUMERS = [c for p in CONSUMER_PATTERNS for c in _per_pattern(p)] + [
    Consumer("set_search", ("PatternSet.search", "PatternSet.matches"), lambda H, b: H.set.search(b) + (H.set.matches(b),),
             _set_search, lambda e, T: e[2].any(axis=1)),
    Consumer("set_count", ("PatternSet.count",), lambda H, b: (H.set.count(b),),
             lambda T: (np.array([[len(findall(p, t)) for p in SET] for t in T], np.int32).reshape(len(T), len(SET)),),
             lambda e, T: e[0].sum(axis=1) > 0),
    Consumer("set_findall", ("PatternSet.findall",), lambda H, b: H.set.findall(b), lambda T: SFX.expected_arrays(SET, T, _FINDALL), _some()),
    Consumer("set_sub", ("PatternSet.sub", "PatternSet.subn"), lambda H, b: H.set.subn(SET_REPLS, b),
             lambda T: SSX.expected_arrays(SET, SET_REPLS, T, 0, _FINDALL), lambda e, T: e[2] > 0),
    Consumer("set_extract", ("PatternSet.extract", "DeviceBatch.gather_spans"), lambda H, b: H.set.extract(b), _set_extract, _some(2)),
    Consumer("filter", ("CompiledRegex.filter",), lambda H, b: (lambda r: (r[0], r[1]))(H.rx[KEEP].filter(b)),
             lambda T: (lambda e: (e[1], e[2], e[0]))(FX.expected([KEEP], T, cache=_TEST)), _kept_flags),
    Consumer("set_filter", ("PatternSet.filter",), lambda H, b: H.set.filter(b, mode="all", invert=True),
             lambda T: (lambda e: (e[1], e[2], e[0]))(FX.expected(SET, T, "all", True, _TEST)), _kept_flags),
    Consumer("extract", ("CompiledRegex.extract",), lambda H, b: H.rx[STREAM].extract(b),
             lambda T: (lambda e: (e[2], e[3], e[0], e[1]))(XX.expected_findall(STREAM, T, _FINDALL)), _some(2)),
    Consumer("expand", ("CompiledRegex.expand",), lambda H, b: H.rx[GROUPS].expand(TEMPLATE, b),
             lambda T: (lambda e: (e[2], e[3], e[0], e[1]))(EX.expected(GROUPS, TEMPLATE, T)), _some(2)),
    Consumer("numbers", ("CompiledRegex.numbers", "DeviceBatch.parse_spans"), lambda H, b: H.rx[NUM].numbers(b, "int"), _numbers, _some(2)),
    Consumer("value_counts", ("CompiledRegex.value_counts", "DeviceBatch.distinct", "DeviceBatch.take"),
             lambda H, b: H.rx[STREAM].value_counts(b, sort="count", top=10), _value_counts,
             lambda e, T: np.array([len(findall(STREAM, t)) > 0 for t in T])),
    Consumer("distinct", ("DeviceBatch.distinct",), lambda H, b: b.distinct(),
             lambda T: (lambda e: (e[3], e[4], e[2], e[0], e[1]))(DX.expected(T)), lambda e, T: e[2][e[3]] > 1),
    Consumer("dict_lookup", ("Dictionary.lookup", "Dictionary.isin"), lambda H, b: (H.dict.lookup(b), H.dict.isin(b)),
             lambda T: (lambda e: (e, e >= 0))(LX.expected(DICT, T)), lambda e, T: e[1]),
    Consumer("dict_filter", ("Dictionary.filter",), lambda H, b: H.dict.filter(b, invert=True),
             lambda T: (lambda e: (e[1], e[2], e[0]))(LX.filtered(DICT, T, True)), _kept_flags),
    Consumer("argsort", ("DeviceBatch.argsort",), lambda H, b: b.argsort(rank=True), SX.expected,
             lambda e, T: np.bincount(e[1])[e[1]] > 1),   # (a text that occurs more than once: a tie of the sort)
    Consumer("take", ("DeviceBatch.take",), lambda H, b: (b.take(H.dev(take_index(b.n))),),
             lambda T: packed(SX.take(T, take_index(len(T)))), lambda e, T: np.bincount(take_index(len(T)), minlength=len(T)) > 0),
    Consumer("parse_int", ("DeviceBatch.parse",), lambda H, b: b.parse("int", fill=-1),
             lambda T: (lambda e: (e[1], e[0]))(PX.expect_many(T, "int", -1)), lambda e, T: e[1] == 0),
    Consumer("parse_float", ("DeviceBatch.parse",), lambda H, b: (lambda r: (r[0].view(H.torch.int64), r[1]))(b.parse("float")),
             _parse("float"), lambda e, T: e[1] == 0),
    Consumer("format_records", (), lambda H, b: H.M.format_records(FMT, [b, H.dev(np.arange(b.n, dtype=np.int64))], status=True),
             _format, lambda e, T: np.array([len(t) > 0 for t in T])),
    Consumer("kw_count", ("Keywords.count", "Keywords.contains"), lambda H, b: (H.kw.count(b), H.kw.contains(b)),
             lambda T: (lambda c: (c, c > 0))(KX.counts(KX.findall(KW, T))), lambda e, T: e[1]),
    Consumer("kw_findall", ("Keywords.findall",), lambda H, b: H.kw.findall(b), lambda T: KX.arrays(KX.findall(KW, T)), _some()),
    Consumer("kw_filter", ("Keywords.filter",), lambda H, b: H.kw.filter(b),
             lambda T: (lambda e: (e[1], np.frombuffer(e[2], np.uint8), e[0]))(KX.filtered(KX.findall(KW, T), T)), _kept_flags),
    Consumer("kw_leftmost", ("Keywords.leftmost",), lambda H, b: H.kw.leftmost(b), lambda T: KX.arrays(KSX.leftmost(KW, T)), _some()),
    Consumer("kw_sub", ("Keywords.sub", "Keywords.subn"), lambda H, b: H.kw.subn(KW_REPL, b), _kw_sub, lambda e, T: e[2] > 0),
    Consumer("lines", ("DeviceBatch.lines",),
             lambda H, b: (lambda r: (r[0], r[1], r[2], r[0]._end_offset, r[0]._max_len, r[0].tail))(b.lines()), _lines, _some(2)),
    Consumer("fields_ws", ("DeviceBatch.fields",), lambda H, b: b.fields(WS_COLUMNS), _fields(WS_COLUMNS, None),
             lambda e, T: e[1][:, 1, 0] >= 0),
    Consumer("fields_delim", ("DeviceBatch.fields",), lambda H, b: b.fields(DELIM_COLUMNS, delim=b","), _fields(DELIM_COLUMNS, b","),
             lambda e, T: e[1][:, 0, 0] >= 0),
    Consumer("cut", ("DeviceBatch.cut", "DeviceBatch.fields", "DeviceBatch.expand_spans"), lambda H, b: b.cut(CUT_COLUMNS), _cut,
             lambda e, T: np.diff(e[0]) > 2),
    Consumer("upper", ("DeviceBatch.upper", "DeviceBatch.translate"), lambda H, b: (_same_length(H, b.upper()),),
             lambda T: packed([TX.translate(t, TX.UPPER) for t in T]), lambda e, T: np.array([t != t.upper() for t in T])),
    Consumer("translate_delete", ("DeviceBatch.translate",),
             lambda H, b: (lambda r: (r, r._end_offset, r._max_len))(b.translate(delete=DELETE)),
             lambda T: _translated(T, delete=DELETE), lambda e, T: np.array([t != TX.translate(t, None, DELETE) for t in T])),
    Consumer("strip", ("DeviceBatch.strip",), lambda H, b: b.strip(spans=True),
             lambda T: (np.arange(len(T) + 1, dtype=np.int64), TX.strip_rows(T)), lambda e, T: np.array([t != t.strip() for t in T])),
]

# The batch-taking public methods that no producer and no consumer runs, each with its reason.
NOT_COVERED = {
    # constructors and accessors: they take no batch
    "DeviceBatch.csr_known": "constructor", "DeviceBatch.strided": "constructor", "DeviceBatch.from_texts": "constructor",
    "DeviceBatch.from_arrow": "constructor (needs pyarrow)", "DeviceBatch.call": "the dispatch under every operation",
    "DeviceBatch.csr_offsets": "accessor", "DeviceBatch.longest": "accessor",
    "CompiledRegex.get_engine_type": "no batch", "CompiledRegex.get_stats": "no batch", "CompiledRegex.describe": "no batch",
    "PatternSet.describe": "no batch", "Keywords.describe": "no batch",
    # the _async twins: the same C call on the caller's tensors
    "DeviceBatch.lines_async": "_async twin", "DeviceBatch.fields_async": "_async twin", "DeviceBatch.translate_async": "_async twin",
    "DeviceBatch.strip_async": "_async twin", "DeviceBatch.distinct_async": "_async twin", "DeviceBatch.take_async": "_async twin",
    "CompiledRegex.filter_async": "_async twin", "CompiledRegex.extract_async": "_async twin",
    "CompiledRegex.findall_async": "_async twin", "PatternSet.filter_async": "_async twin",
    "Dictionary.lookup_async": "_async twin", "Dictionary.filter_async": "_async twin", "Keywords.filter_async": "_async twin",
    # host-list wrappers: they upload a list and read the device form back
    "CompiledRegex.findall_lists": "host-list wrapper", "CompiledRegex.split": "host-list wrapper",
    "CompiledRegex.captures": "host-list wrapper", "CompiledRegex.sub": "host-list wrapper",
    "PatternSet.findall_lists": "list form of findall", "Keywords.findall_lists": "list form of findall",
    "Keywords.leftmost_lists": "list form of leftmost",
    # the Engine seam with a start argument and the one-match capture form: no *_expect module states them, and this
    # module writes no expectation of its own
    "CompiledRegex.match_first_at": "start seam: tests/test_gpu_parity.py", "CompiledRegex.match_next_at": "start seam",
    "CompiledRegex.is_match_at": "start seam", "CompiledRegex.captures_dev": "one-match captures: tests/test_gpu_parity.py",
}
