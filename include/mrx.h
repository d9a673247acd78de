/*
 * mrx.h -- C ABI of the MI355X batch regex matcher (libmrx_hip.so).
 *
 * Drop-in boundary for the byte-scanning hot path of msaelices/mojo-regex.
 * The reference has no FFI; the seams this ABI replaces are its two Mojo traits
 * and the module functions built on them (all paths relative to the reference):
 *
 *   Engine        src/regex/engine.mojo:4-37      match_first / match_all
 *   RegexMatcher  src/regex/matcher.mojo:181-209  match_first / match_all (+ match_next)
 *   module API    src/regex/matcher.mojo:1325-1415 (search, findall, split, match_first)
 *                 src/regex/matcher.mojo:1857-1917 (sub)
 *   CompiledRegex src/regex/matcher.mojo:929-1163  (compile once, match many)
 *
 * The reference matches ONE text per call on the CPU.  This library matches a
 * BATCH of texts per call on the GPU (one wavefront lane per text) and returns,
 * for every text, exactly what the reference call returns for it: byte offsets,
 * half-open [start, end), leftmost start / longest end, restart-per-position
 * search (src/regex/dfa.mojo:1875-2130).
 *
 * Conventions (mirroring SURVEY.md 8(b)):
 *   - Ownership: the caller owns every input and output buffer; the library owns
 *     the opaque compiled handle until mrx_free().  A handle is immutable after
 *     mrx_compile(), so concurrent batch calls on one handle are safe.
 *   - Errors: integer status; mrx_last_error() gives the message of the last
 *     failing call on this thread.  Pattern syntax errors carry the reference's
 *     own message text (src/regex/lexer.mojo:150-152, parser.mojo:224-237,340,399).
 *     Matching never fails on data: "no match" is start = end = -1 / count 0.
 *   - Text is raw bytes (no UTF-8 awareness), as in the reference (all tables
 *     are 256 wide, src/regex/dfa.mojo:215-254).
 *   - Span offsets are int32 and relative to the start of each text (texts up to
 *     2 GiB - 1); batch offsets are int64.
 *   - Batch layout: `data` holds the texts back to back, text i occupies
 *     data[offsets[i] .. offsets[i+1]).  The *_strided entry points take texts
 *     at a fixed pitch instead: text i starts at data + i*stride and has length
 *     lens[i] (or `len` for all i when lens == NULL).  Every layout runs on the
 *     streaming kernels when the plan allows it; stride % 16 == 0 with a 16-byte
 *     aligned `data` is the fastest form (no per-text alignment frame).
 *   - Pointers named d_* are DEVICE pointers (HBM); everything else is host
 *     memory.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     The *_dev entry points enqueue work and return without synchronising
 *     unless they have to report a total (documented per function).
 *   - No CPU fallback exists: without a usable HIP device every matching entry
 *     point fails with MRX_E_NO_DEVICE.
 */
#ifndef MRX_H
#define MRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mrx_handle mrx_handle;

enum {
  MRX_OK = 0,
  MRX_E_SYNTAX = 1,       /* the reference's parser raises on this pattern          */
  MRX_E_UNSUPPORTED = 2,  /* refused, never approximated: backtracker programs beyond */
                          /* the flat form's limits, tables beyond their budgets ... */
                          /* mrx_last_error() carries the reason                    */
  MRX_E_NO_DEVICE = 3,    /* no HIP device / HIP runtime error                      */
  MRX_E_CAPACITY = 4,     /* output buffer too small; *total holds the need         */
  MRX_E_ARGUMENT = 5
};

/* ---- compile (replaces CompiledRegex(pattern), matcher.mojo:964-978) ---------- */
/* A CONTRACT OF THIS LIBRARY'S OWN -- `$` on the LazyDFA search (search / findall / count / sub of a pattern with `$`
 * that the reference routes to NFAMatcher: matcher.mojo:401-431).  Upstream's LazyDFA decides whether `$` holds when a
 * (state, byte) transition is FIRST computed -- it holds iff that byte is the last of the text in hand -- and caches the
 * answer for every later use, in that call and in every later call on the same CompiledRegex (pikevm.mojo:869-942):
 * `^[a-z]+$` finds "abc" in a fresh process, nothing in "abcabc", and after that nothing in "abc" either.  A batch
 * has no call order, so every text of every call is answered AS A FRESHLY COMPILED PATTERN WOULD answer it: the
 * cache is empty when a text begins and is carried through that text's walks (findall, the match_next calls of one
 * sub) exactly as upstream carries it.  The oracle restates this (oracle/mrx_ref), tests/test_oracle_golden.py holds
 * hand traces; no reference test pins it ("parity-unpinned").  match_first / is_match of `$` patterns run on
 * the reference's OnePass automaton and have no such history. */
int mrx_compile(const char* pattern, size_t pattern_len, mrx_handle** out);
/* Options.  MRX_COMPILE_LAZYDFA_SEMANTICS routes the pattern as the reference does when
 * DFAEngine compilation fails (matcher.mojo:666-672): NFAMatcher / LazyDFA, leftmost-longest
 * over the PikeVM program (pikevm.mojo:754-867).  It is NOT what the reference returns for
 * SIMPLE patterns -- e.g. it honours the `+` of (x|y|foo|bar)+ that the DFA alternation
 * compiler drops (dfa.mojo:873-928) -- and exists so that config-5 numbers can be reported
 * under both readings.  mrx_describe() shows the option.
 *
 * MRX_COMPILE_BITSET_NFA: patterns the reference routes to LazyDFA (pikevm.mojo:664-987)
 * normally run on its eagerly determinised table; with this option -- and always when that
 * table would exceed 4096 states -- the walk runs on the bitset NFA instead (state = bit
 * mask of live PikeVM positions, up to 256).  Results are identical; only the kernel differs.
 *
 * MRX_COMPILE_NFA_ENGINE: the handle is the reference's NFAEngine used directly as the Engine
 * (engine.mojo:4-37, nfa.mojo:66-143) -- what `regex.nfa.match_first / findall`
 * (nfa.mojo:1733-1769) and the reference's tests/test_nfa.mojo drive -- instead of the
 * HybridMatcher router: greedy backtracking, first alternative wins, NFAEngine's literal
 * prefilter and `.*` fast paths, none of HybridMatcher's shortcuts.  Served by the flat program
 * of the backtracking matcher; MRX_E_UNSUPPORTED at the first matching call when the pattern
 * exceeds that form (16 nesting levels, 30 open choices, 240 items).
 *
 * MRX_COMPILE_DFA_ENGINE: likewise, the DFAEngine that compile_dfa_pattern(parse(pattern))
 * returns (dfa.mojo:2385-2496), as the comptime API (comptime_regex.mojo:59-87, 176-233) and
 * the reference's tests/test_dfa.mojo use it: no classifier, no exact-literal / prefilter /
 * required-byte shortcut in front.  MRX_E_UNSUPPORTED at compile time, with the dispatcher's
 * message, when no shape compiler takes the pattern. */
enum { MRX_COMPILE_LAZYDFA_SEMANTICS = 1, MRX_COMPILE_BITSET_NFA = 2, MRX_COMPILE_NFA_ENGINE = 4,
       MRX_COMPILE_DFA_ENGINE = 8 };
int mrx_compile_ex(const char* pattern, size_t pattern_len, uint32_t options, mrx_handle** out);
void mrx_free(mrx_handle* h);
const char* mrx_last_error(void);
/* HybridMatcher.get_engine_type(), matcher.mojo:900-918: "DFA", "NFA", "+Prefilter"... */
const char* mrx_engine_type(const mrx_handle* h);
/* CompiledRegex.get_stats(), matcher.mojo:1139-1163 */
const char* mrx_stats(const mrx_handle* h);
/* Text dump of the compiled tables (states, transitions, flags, kernel plan).
 * Returns the number of bytes needed (excluding NUL); writes at most cap. */
size_t mrx_describe(const mrx_handle* h, char* buf, size_t cap);
/* number of capture groups usable by mrx_captures_* / group references in mrx_sub_*:
 * the fixed-width (\d{N}) form (matcher.mojo:1002-1035) or the general groups of
 * NFAEngine.match_next_with_groups (nfa.mojo:500-574), in _match_group order; 0 if none */
int mrx_num_groups(const mrx_handle* h);

/* ---- device-resident batches (the measured path) --------------------------- */
/* regex.match_first(pattern, text), matcher.mojo:1396-1415: anchored at 0.
 * d_start[i] / d_end[i] = span or -1/-1. */
int mrx_match_first_dev(const mrx_handle* h, const uint8_t* d_data,
                        const int64_t* d_offsets, int64_t n,
                        int32_t* d_start, int32_t* d_end, void* stream);
/* regex.search(pattern, text), matcher.mojo:1325-1338 (= match_next(text, 0)). */
int mrx_search_dev(const mrx_handle* h, const uint8_t* d_data,
                   const int64_t* d_offsets, int64_t n,
                   int32_t* d_start, int32_t* d_end, void* stream);
/* Same two operations for texts at a fixed pitch (see header comment). */
int mrx_match_first_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride,
                                const int32_t* d_lens, int32_t len, int64_t n,
                                int32_t* d_start, int32_t* d_end, void* stream);
int mrx_search_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride,
                           const int32_t* d_lens, int32_t len, int64_t n,
                           int32_t* d_start, int32_t* d_end, void* stream);
/* CompiledRegex.is_match(text, 0), matcher.mojo:1103-1115 (DFAEngine.is_match
 * quirk included, dfa.mojo:1815-1849).  d_flag[i] = 0/1. */
int mrx_is_match_dev(const mrx_handle* h, const uint8_t* d_data,
                     const int64_t* d_offsets, int64_t n, uint8_t* d_flag,
                     void* stream);
int mrx_is_match_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride,
                             const int32_t* d_lens, int32_t len, int64_t n, uint8_t* d_flag,
                             void* stream);
/* The same three operations from a start position -- Engine.match_first(text, start)
 * (src/regex/engine.mojo:4-37), RegexMatcher / CompiledRegex.match_first / match_next / is_match
 * (matcher.mojo:181-209, 1049-1115): text i is matched from start (all texts) or d_starts[i]
 * (d_starts != NULL; int32[n] on the device).  Results are offsets from the beginning of the text, as
 * the reference's Match carries them.  Reference rules kept: a '^' pattern on the DFA or OnePass route
 * answers None for start > 0 (dfa.mojo:1866-1867, 1887-1891; onepass.mojo:445) while the LazyDFA treats
 * '^' as satisfied at every start (pikevm.mojo:714); start == len matches the empty rest; start > len
 * gives None, except that LazyDFA / OnePass match_first (and is_match, and DFAEngine.is_match with a
 * first-byte matcher) report the empty match (start, start) when the start state accepts, as upstream
 * does (pikevm.mojo:820-867, dfa.mojo:1832-1836).  start < 0 (undefined upstream) gives None.
 * match_first here is the engine-level operation: a match, if any, begins AT start. */
int mrx_match_first_at_dev(const mrx_handle* h, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                           int32_t start, const int32_t* d_starts, int32_t* d_start, int32_t* d_end,
                           void* stream);
int mrx_search_at_dev(const mrx_handle* h, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                      int32_t start, const int32_t* d_starts, int32_t* d_start, int32_t* d_end, void* stream);
int mrx_is_match_at_dev(const mrx_handle* h, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        int32_t start, const int32_t* d_starts, uint8_t* d_flag, void* stream);
int mrx_match_first_at_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride,
                                   const int32_t* d_lens, int32_t len, int64_t n, int32_t start,
                                   const int32_t* d_starts, int32_t* d_start, int32_t* d_end, void* stream);
int mrx_search_at_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride,
                              const int32_t* d_lens, int32_t len, int64_t n, int32_t start,
                              const int32_t* d_starts, int32_t* d_start, int32_t* d_end, void* stream);
int mrx_is_match_at_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride,
                                const int32_t* d_lens, int32_t len, int64_t n, int32_t start,
                                const int32_t* d_starts, uint8_t* d_flag, void* stream);
/* regex.findall(pattern, text), matcher.mojo:1341-1354.
 * d_counts_prefix[n+1]: exclusive prefix sum of matches per text (CSR);
 * d_spans[2*k], d_spans[2*k+1] = start, end of match k (text-relative), in text
 * order then match order.  span_cap = capacity of d_spans in spans.  d_spans must be 8-byte aligned (a span is
 * stored as one 8-byte word; hipMalloc and every framework allocator give far more).
 * Synchronises the stream once to return *total; MRX_E_CAPACITY if
 * *total > span_cap (nothing is ever written to d_spans beyond capacity).
 * total == NULL: nothing is read back and the call returns without synchronising;
 * d_counts_prefix[n] holds the total once the stream has drained (compare it with
 * span_cap before using the spans). */
int mrx_findall_dev(const mrx_handle* h, const uint8_t* d_data,
                    const int64_t* d_offsets, int64_t n,
                    int64_t* d_counts_prefix, int32_t* d_spans, int64_t span_cap,
                    int64_t* total, void* stream);
/* Same for a caller that knows its offsets (it built them on the host, or holds an Arrow array's): end_offset =
 * d_offsets[n], max_text_len = the longest text's length -- both may be upper bounds, neither may be too small
 * (they size scratch the kernels index with the real offsets).  mrx_findall_dev has to read the two from the device
 * -- one small kernel and one stream synchronisation before its scan can be enqueued -- which this entry point
 * spares: with total == NULL the whole call is asynchronous. */
int mrx_findall_known_dev(const mrx_handle* h, const uint8_t* d_data,
                          const int64_t* d_offsets, int64_t n, int64_t end_offset, int64_t max_text_len,
                          int64_t* d_counts_prefix, int32_t* d_spans, int64_t span_cap,
                          int64_t* total, void* stream);
/* Same, texts at a fixed pitch (see header comment).  d_lens may be NULL. */
int mrx_findall_strided_dev(const mrx_handle* h, const uint8_t* d_data,
                            int64_t stride, const int32_t* d_lens, int32_t len,
                            int64_t n, int64_t* d_counts_prefix, int32_t* d_spans,
                            int64_t span_cap, int64_t* total, void* stream);
/* Scan only: matches per text and nothing else (no span output). */
int mrx_count_dev(const mrx_handle* h, const uint8_t* d_data,
                  const int64_t* d_offsets, int64_t n, int32_t* d_counts,
                  void* stream);
int mrx_count_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride,
                          const int32_t* d_lens, int32_t len, int64_t n, int32_t* d_counts,
                          void* stream);
/* search + capture groups, in the order NFAEngine._match_group appends them
 * (src/regex/nfa.mojo:1057-1103): groups 1..g, then group 0 (whole match).
 * d_spans[(i*(g+1) + k)*2 + {0,1}]; -1 when text i has no match.
 * Fixed-width (\d{N}) groups run on the streaming kernel; other group structures on the flat-program
 * backtracker (refused only beyond its limits: 16 nesting levels, 30 open choices). */
int mrx_captures_dev(const mrx_handle* h, const uint8_t* d_data,
                     const int64_t* d_offsets, int64_t n, int32_t* d_spans,
                     void* stream);
int mrx_captures_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride,
                             const int32_t* d_lens, int32_t len, int64_t n, int32_t* d_spans,
                             void* stream);
/* regex.sub(pattern, repl, text, count), matcher.mojo:1679-1854.
 * d_out_offsets[n+1] (CSR of output bytes), d_out_data (capacity out_cap bytes).
 * Waits for the sizes to return *total_bytes (MRX_E_CAPACITY if it exceeds out_cap); the output bytes
 * themselves are written by work enqueued on `stream`, like the results of every other _dev call. */
int mrx_sub_dev(const mrx_handle* h, const char* repl, size_t repl_len, int64_t count,
                const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                int64_t* total_bytes, void* stream);
/* Same for a caller that knows its offsets (see mrx_findall_known_dev: end_offset = d_offsets[n], max_text_len = the
 * longest text; upper bounds are fine, neither may be too small): spares the small kernel and the stream
 * synchronisation with which mrx_sub_dev reads the two from the device before anything else can be enqueued. */
int mrx_sub_known_dev(const mrx_handle* h, const char* repl, size_t repl_len, int64_t count,
                      const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset,
                      int64_t max_text_len, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                      int64_t* total_bytes, void* stream);

/* Same, texts at a fixed pitch (round 3; every other operation already had this form).  Rows without padding
 * (len == stride, d_lens == NULL) take every fast path of mrx_sub_dev; padded rows run on the lane-per-text kernels. */
int mrx_sub_strided_dev(const mrx_handle* h, const char* repl, size_t repl_len, int64_t count,
                        const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                        int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                        int64_t* total_bytes, void* stream);

/* regex.split (matcher.mojo:1357-1393): the text between successive non-overlapping matches, the matches themselves
 * removed; a separator at the very start or end, or two adjacent ones, yields an empty piece.  maxsplit == 0: no limit;
 * > 0: at most that many splits per text, the rest of the text is the last piece; < 0: no split at all (the whole text
 * is the only piece) -- the reference's loop `if maxsplit != 0 and splits_done >= maxsplit: break`.
 *   d_piece_prefix[n + 1]  CSR offsets of the texts' pieces (text i has min(matches, maxsplit) + 1 of them)
 *   d_pieces[piece_cap][2] byte ranges [start, end) within the piece's own text, text order then position;
 *                          always 0 <= start <= end <= len.  The exact-literal route finds the overlapping
 *                          occurrences of a self-overlapping literal, as the reference's findall does
 *                          (matcher.mojo:815-847; 22 x "a" in 23 x "a": (0, 22), (1, 23)); the piece between two
 *                          overlapping matches is the empty range [end of the first, end of the first).
 * *total (host, may be NULL) = number of pieces; MRX_E_CAPACITY when piece_cap does not hold them (what fits is not
 * written then; *total holds the need when the limit is off, a lower bound otherwise).  One stream synchronisation. */
int mrx_split_dev(const mrx_handle* h, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t maxsplit,
                  int64_t* d_piece_prefix, int32_t* d_pieces, int64_t piece_cap, int64_t* total, void* stream);
int mrx_split_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len,
                          int64_t n, int64_t maxsplit, int64_t* d_piece_prefix, int32_t* d_pieces, int64_t piece_cap,
                          int64_t* total, void* stream);

/* captures_all: the capture groups of every match, Python's [m.groups() for m in re.finditer(p, t)] per text.
 * The reference has no such call; its one loop over every match with groups is the loop of sub() with a template that
 * names a group (_sub_impl_with_repl, matcher.mojo:1679-1854).  The matches are exactly the ones that loop visits, with
 * the groups it reads:
 *   - fixed-width form (a pattern of (\d{N}) groups and literals): match_next from pos; group j at
 *     match start + its offset, of its width.  A "concat" pattern (groups only) on a text of exactly its total width
 *     takes the whole-text shortcut: one match at 0 if every byte is a digit, else none;
 *   - otherwise NFAEngine.match_next_with_groups from pos; a group without an entry is (-1, -1);
 *   - after an empty match pos = end + 1; a match that lies in front of pos ends the text's list (the reference does
 *     not terminate there); an empty text has no match.
 * These are NOT findall's spans where the groups run on the backtracker: it is greedy and the first alternative wins,
 * while findall takes the hybrid engines' leftmost-longest walk ('(a|ab)(c|bcd)(d*)' on "abcd": findall (0, 4),
 * captures_all no match).  Exact literals differ too: findall returns overlapping occurrences, this loop does not.
 *   d_match_prefix[n + 1]  CSR offsets of the texts' matches, at most `count` per text when count > 0 (0 = all)
 *   d_groups               match k (text order, then match order) holds g + 1 pairs, g = mrx_num_groups(h): groups 1..g,
 *                          then group 0 (the whole match), the order and raw (unclamped) spans of mrx_captures_dev:
 *                          d_groups[((k * (g + 1)) + j) * 2 + {0, 1}].  A text's first row is its mrx_captures_dev row
 *                          (outside the whole-text shortcut)
 *   *total (host, not NULL) the number of matches; one stream synchronisation returns it.  MRX_E_CAPACITY when it
 *                          exceeds match_cap; no row at or beyond match_cap is ever written.
 * Negative n, count or match_cap, and null pointers: MRX_E_ARGUMENT.  A pattern that sub() with a group template refuses
 * (beyond the flat program's limits) is refused the same way, MRX_E_UNSUPPORTED, before anything is enqueued.  Routes
 *  are those of sub() with a group template; results never depend on them. */
int mrx_captures_all_dev(const mrx_handle* h, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t count,
                         int64_t* d_match_prefix, int32_t* d_groups, int64_t match_cap, int64_t* total, void* stream);
/* Same, texts at a fixed pitch (as mrx_sub_strided_dev: rows without padding take every route of the CSR form, padded
 * rows the lane-per-text kernels). */
int mrx_captures_all_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                                 int32_t len, int64_t n, int64_t count, int64_t* d_match_prefix, int32_t* d_groups,
                                 int64_t match_cap, int64_t* total, void* stream);

/* ---- pattern sets: one batch against k patterns in one call ------------------------------------------------------
 * The reference matches one pattern per call; a set answers k of them per text.  Member j's answer for text i is
 * exactly what the single-pattern call on member j's own handle returns for it (so: what the reference's search /
 * len(findall) returns).  Members whose single-pattern search or count runs the streaming kernel's one
 * left-to-right walk share ONE pass over the texts (several for more than 32 such members: each pass reads the
 * batch again); every other member runs its own single-pattern call into scratch.  Which of the two a call takes
 * depends only on the set, the operation and the batch shape, never on timing; as measured so far the members' own
 * calls win at every set size, so they are the default for every member.  The results never depend on it.  Layouts and argument rules are those of the single-pattern _dev entry points.
 *
 * Compile: options are those of the single-pattern compile, applied to every member; 1 <= k <= 256
 * (MRX_E_ARGUMENT otherwise).  A syntax error in any member fails the whole compile with MRX_E_SYNTAX, and the
 * message reads "member j: <the reference's message>".  A member that refuses an operation makes the operation
 * MRX_E_UNSUPPORTED for the set ("member j: <reason>"), reported before anything is enqueued.
 *
 * Output layout: text-major, text i / member j at i*k + j.  search: d_start / d_end int32[n][k], -1/-1 = no match.
 * count: int32[n][k] matches per member (len(findall)).  matches: uint64 words, ceil(k/64) per text; bit j % 64 of
 * word d_bits[i * ceil(k/64) + j / 64] is set when member j's search finds a match in text i.  That is a SEARCH
 * hit, not the single-pattern is_match operation, whose DFA first-byte quirk (dfa.mojo:1815-1849) answers some texts
 * differently.  search, count and matches synchronise nothing: they enqueue their work on `stream` and return. */
typedef struct mrx_set mrx_set;
int mrx_set_compile(const char* const* patterns, const size_t* lens, int32_t k, uint32_t options, mrx_set** out);
void mrx_set_free(mrx_set* s);
int32_t mrx_set_size(const mrx_set* s);
/* per member: its route for each operation ("shared(pass P/p, column g.m | class c)" or "own" with the reason);
 * returns the bytes needed (excluding NUL), writes at most cap */
size_t mrx_set_describe(const mrx_set* s, char* buf, size_t cap);
int mrx_set_search_dev(const mrx_set* s, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                       int32_t* d_start, int32_t* d_end, void* stream);
int mrx_set_search_strided_dev(const mrx_set* s, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                               int32_t len, int64_t n, int32_t* d_start, int32_t* d_end, void* stream);
int mrx_set_count_dev(const mrx_set* s, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                      int32_t* d_counts, void* stream);
int mrx_set_count_strided_dev(const mrx_set* s, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                              int32_t len, int64_t n, int32_t* d_counts, void* stream);
int mrx_set_matches_dev(const mrx_set* s, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        uint64_t* d_bits, void* stream);
int mrx_set_matches_strided_dev(const mrx_set* s, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                                int32_t len, int64_t n, uint64_t* d_bits, void* stream);
/* findall of every member, text-major (the members' findall spans regrouped by text):
 *   d_text_prefix int64[n + 1]  CSR over texts: text i's hits are [d_text_prefix[i], d_text_prefix[i + 1])
 *   d_members int32[total]      the member of each hit
 *   d_spans int32[total][2]     start, end of each hit, text-relative, raw as mrx_findall_dev returns them; a span is
 *                               one 8-byte word, so d_spans must be 8-byte aligned
 * Within text i come member 0's findall spans for text i in match order, then member 1's, and so on: d_members never
 * decreases within a text, and the run of member j in text i is exactly what mrx_findall_dev on member j's handle
 * returns for that text (overlapping occurrences of a self-overlapping exact literal, empty matches and the `$`-LazyDFA
 * contract included), so its length is cell (i, j) of mrx_set_count_dev.  Hits are not ordered by position across
 * members.
 * span_cap = capacity of d_members and d_spans in hits.  total > span_cap: MRX_E_CAPACITY, with *total and
 * d_text_prefix valid once the stream drains (retry with *total); nothing is written at or beyond span_cap.
 * The call synchronises the stream once (the members' totals size the second phase); a CSR batch
 * without known bounds adds one synchronisation per call for its byte count and longest text -- the _known form, as
 * mrx_findall_known_dev, spares it.  total may be NULL.  n == 0 gives d_text_prefix = {0}.  Negative n or span_cap,
 * and null pointers: MRX_E_ARGUMENT.  A member whose search / findall is refused makes the call MRX_E_UNSUPPORTED
 * ("member j: <reason>") before anything is enqueued or written. */
int mrx_set_findall_dev(const mrx_set* s, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        int64_t* d_text_prefix, int32_t* d_members, int32_t* d_spans, int64_t span_cap, int64_t* total,
                        void* stream);
int mrx_set_findall_known_dev(const mrx_set* s, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                              int64_t end_offset, int64_t max_text_len, int64_t* d_text_prefix, int32_t* d_members,
                              int32_t* d_spans, int64_t span_cap, int64_t* total, void* stream);
int mrx_set_findall_strided_dev(const mrx_set* s, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                                int32_t len, int64_t n, int64_t* d_text_prefix, int32_t* d_members, int32_t* d_spans,
                                int64_t span_cap, int64_t* total, void* stream);
/* sub of a set: replace the hits of every member in one call.  Defined on the hits that mrx_set_findall_dev returns,
 * not on the reference's sub() loop (the reference has no multi-pattern call).  For text i:
 *   1. the candidates are every member's findall hits in text i, (s, j, e) = start, member, end -- overlapping
 *      occurrences of a self-overlapping exact literal, empty matches and the `$`-LazyDFA contract included, exactly as
 *      set findall returns them;
 *   2. walk the candidates in ascending (s, j) order (then e), pos = 0: a candidate is SELECTED iff s >= pos, and then
 *      pos = max(e, s + 1); stop after `count` selections when count > 0;
 *   3. the output is the text with each selected [s, e) replaced by member j's replacement; every other byte is copied.
 * So at equal start the lower member wins (member order is priority order); a hit that overlaps a selected one is
 * dropped and its member is NOT searched again behind the selected hit; an empty hit is selected where no earlier
 * selection covers its position (findall of `z*` on "ab" is (0,0) (1,1) (2,2): replacement "-" gives "-a-b-"; on ""
 * it is (0,0), which gives "-").
 * A one-member set differs from mrx_sub_dev exactly where the reference's sub() loop does not visit findall's list:
 * exact literals (findall overlaps, the set drops the overlap: sub() searches again behind each match); empty
 * matches (sub() copies text[pos] behind an empty match found beyond pos, oracle/mrx_ref/hybrid.py:668, and returns
 * an empty text unchanged); and any other route whose sub is not served from findall's spans.
 * repls[k], repl_lens[k] (k = mrx_set_size): member j's replacement, bytes taken verbatim (as a single sub template
 * without group references); an entry may be NULL when its length is 0, and repls itself when every length is 0.
 * A replacement that holds a group reference \1..\9 is refused, MRX_E_UNSUPPORTED ("member j: group references are
 * not supported in a set's sub"), before anything is enqueued; no length is refused.
 *   d_out_offsets int64[n + 1], d_out_data: the output CSR, as mrx_sub_dev writes it.
 *   d_nsub int32[n] (may be NULL): the number of replacements in each text.
 *   *total_bytes (may be NULL): the output size.  Above out_cap: MRX_E_CAPACITY, nothing written at or beyond
 *   out_cap, d_out_offsets (and d_nsub) valid once the stream drains, for a retry.
 * Synchronisations: two per call -- the set findall's first phase (its member totals), and the output size -- plus,
 * for a CSR batch without known bounds, the one that reads its byte count and longest text (the _known form spares
 * it).  The output bytes are complete when the stream reaches the point of return.
 * Scratch: 12 bytes per hit of the set's findall (member and span), O(n) words, and the densest member's spans
 * while the members' findall runs: about 30 GB for 2.5 * 10^9 hits.
 * Negative n, count or out_cap, a null required pointer (set, repl_lens, d_offsets, d_out_offsets, d_out_data when
 * out_cap > 0) and a NULL entry of nonzero length: MRX_E_ARGUMENT.  (d_data may be NULL when every text is empty.)  A member whose search /
 * findall is refused makes the call MRX_E_UNSUPPORTED ("member j: <reason>"), as set findall.  n == 0 gives
 * d_out_offsets = {0}. */
int mrx_set_sub_dev(const mrx_set* s, const char* const* repls, const size_t* repl_lens, int64_t count,
                    const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_out_offsets,
                    uint8_t* d_out_data, int64_t out_cap, int32_t* d_nsub, int64_t* total_bytes, void* stream);
int mrx_set_sub_known_dev(const mrx_set* s, const char* const* repls, const size_t* repl_lens, int64_t count,
                          const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset,
                          int64_t max_text_len, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                          int32_t* d_nsub, int64_t* total_bytes, void* stream);
int mrx_set_sub_strided_dev(const mrx_set* s, const char* const* repls, const size_t* repl_lens, int64_t count,
                            const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                            int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int32_t* d_nsub,
                            int64_t* total_bytes, void* stream);

/* ---- filter: keep the matching texts as a new packed batch on the device ----
 * Text i is KEPT when the pattern's search finds a match in it: the predicate of CompiledRegex.test
 * (matcher.mojo:1091-1101), start[i] >= 0 of mrx_search_dev -- not the is_match operation.  MRX_FILTER_INVERT keeps
 * exactly the other texts.  A set keeps a text when some member's search hits (a row of mrx_set_matches_dev with a bit
 * set); with MRX_FILTER_ALL, when every member's does; MRX_FILTER_INVERT negates either, so "none" is the inverse of
 * "any".  (One pattern ignores MRX_FILTER_ALL.)  Any other flag bit: MRX_E_ARGUMENT.
 * The kept texts keep their order (ascending original index).  Outputs, all on the device:
 *   d_kept_idx int64[n]         [0, kept): the original index of each kept text
 *   d_out_offsets int64[n + 1]  [0, kept]: the CSR of the output batch; d_out_offsets[kept] = bytes.  A kept empty
 *                               text contributes no byte and its offset repeats
 *   d_out_data uint8[out_cap]   the kept texts back to back; any alignment
 *   d_totals int64[2]           {kept, bytes}
 * Entries of d_kept_idx and d_out_offsets past those are unspecified.  The output is CSR whatever the input form, so
 * it is the input of a following call as it stands (with bytes and the input's longest text as its known bounds).
 * No byte of d_out_data at or past bytes, nor at or past out_cap, is ever written.
 * Capacity: out_cap = the input's byte count always suffices.  When bytes > out_cap the indices, the offsets and
 * d_totals are still complete and correct, NO output byte is written, and a call with `totals` returns
 * MRX_E_CAPACITY with totals filled.
 * totals (host, int64[2], may be NULL) receives d_totals: the call then reads back once, at its end -- no host
 * decision sits between its kernels.  With totals == NULL the call reads nothing back and is asynchronous, as findall
 * with total == NULL: the gather decides on the device from d_totals, and the caller checks d_totals[1] against its
 * out_cap once the stream has drained.
 * The _known form takes a CSR batch's d_offsets[n] and longest text, as mrx_findall_known_dev, and needs no look at
 * the device before its first kernel (without them a search over few long texts reads them back first).  Upper
 * bounds are fine; neither may be too small.
 * n == 0 gives kept = bytes = 0 and d_out_offsets = {0}.  Negative n or out_cap, unknown flag bits, a bad pitch and a
 * null required pointer (handle, d_offsets, d_out_offsets, d_totals; d_kept_idx when n > 0; d_out_data when
 * out_cap > 0): MRX_E_ARGUMENT.  A pattern (a member) whose search is refused is refused here, MRX_E_UNSUPPORTED with
 * the same reason ("member j: <reason>" for a set), before anything is enqueued or written.
 * Reads: a text's bytes are fetched as the aligned 16-byte words that hold them, so up to 15 bytes in front of a text's
 * first byte and behind its last one are read (never used), as sub's byte mover does: the words around d_data's first
 * and last text must be readable, which every hipMalloc'ed or pooled device buffer gives (256-byte granules).
 * Scratch: 32 bytes per text and the predicate's own (8 bytes per text for one pattern; for a set its bit rows and
 * one member's search), returned to the arena when the call returns. */
enum { MRX_FILTER_INVERT = 1, MRX_FILTER_ALL = 2 };
int mrx_filter_dev(const mrx_handle* h, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                   int64_t* d_kept_idx, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                   int64_t* totals, void* stream);
int mrx_filter_known_dev(const mrx_handle* h, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                         int64_t end_offset, int64_t max_text_len, int64_t* d_kept_idx, int64_t* d_out_offsets,
                         uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);
int mrx_filter_strided_dev(const mrx_handle* h, uint32_t flags, const uint8_t* d_data, int64_t stride,
                           const int32_t* d_lens, int32_t len, int64_t n, int64_t* d_kept_idx, int64_t* d_out_offsets,
                           uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);
int mrx_set_filter_dev(const mrx_set* s, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                       int64_t* d_kept_idx, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                       int64_t* d_totals, int64_t* totals, void* stream);
int mrx_set_filter_known_dev(const mrx_set* s, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                             int64_t end_offset, int64_t max_text_len, int64_t* d_kept_idx, int64_t* d_out_offsets,
                             uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);
int mrx_set_filter_strided_dev(const mrx_set* s, uint32_t flags, const uint8_t* d_data, int64_t stride,
                               const int32_t* d_lens, int32_t len, int64_t n, int64_t* d_kept_idx,
                               int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                               int64_t* totals, void* stream);

/* ---- extract: the bytes under spans as a new packed batch on the device ----
 * The primitive, mrx_gather_spans_*, needs no pattern: it takes the spans that findall, split, captures_all or a set's
 * findall left on the device and copies the bytes they name, piece after piece, into one buffer.
 *   d_prefix int64[n + 1]             CSR over the texts: text i owns the rows [d_prefix[i], d_prefix[i + 1])
 *   d_spans int32[rows][row_pairs][2] the rows, 8-byte aligned.  row_pairs = 1 for findall / split / a set's findall,
 *                                     g + 1 for captures_all; `pair` (0 <= pair < row_pairs) is the pair of each row
 *                                     that is gathered (captures_all: group j is pair j - 1, the whole match pair g)
 *   piece_cap                         capacity, in pieces, of d_owner and d_out_offsets
 * pieces = d_prefix[n], read on the device.  Piece r belongs to the text i with d_prefix[i] <= r < d_prefix[i + 1].
 * With (s, e) its pair and L the text's length, the piece is text[s' .. e') with s' = min(max(s, 0), L) and
 * e' = min(max(e, s'), L): a group without an entry, (-1, -1), and a reversed range give an empty piece; a fixed-width
 * group that reaches behind its text (x(\d)? on "x") is cut at the text's end.  An empty piece adds no byte and its
 * offset repeats.  Overlapping spans (findall of a self-overlapping exact literal) are each copied in full, so the
 * output may hold more bytes than the input.  Outputs, all on the device, pieces in row order:
 *   d_owner int64[piece_cap]            [0, pieces): the text index of each piece
 *   d_out_offsets int64[piece_cap + 1]  [0, pieces]: the CSR of the output batch; d_out_offsets[pieces] = bytes
 *   d_out_data uint8[out_cap]           the pieces back to back; any alignment
 *   d_totals int64[2]                   {pieces, bytes}
 * Entries of d_owner and d_out_offsets past those are unspecified.  The output is a CSR batch and the input of a
 * following call as it stands (with bytes and the input's longest text as its known bounds).
 * No byte of d_out_data at or past bytes, nor at or past out_cap, is ever written, and no element of d_owner at or past
 * piece_cap, nor of d_out_offsets at or past piece_cap + 1.
 * Capacity.  pieces > piece_cap: nothing is written to d_out_data, d_owner and d_out_offsets hold nothing of use,
 * d_totals[0] is the need and d_totals[1] only a lower bound (as *total of mrx_split_dev under a limit; here 0, the
 * spans are not read).  pieces <= piece_cap and bytes > out_cap: d_owner, d_out_offsets and both totals are complete and
 * exact, and NO output byte is written.  A call with `totals` returns MRX_E_CAPACITY in either case, totals filled
 * for a retry (grow the pieces first, then the bytes: two retries at most).
 * totals (host, int64[2], may be NULL) receives d_totals: the call then reads back once, at its end -- no host
 * decision sits between its kernels.  With totals == NULL nothing is read back and the call returns without
 * synchronising: the kernels decide on the device from d_totals, as filter's gather does, and the caller checks
 * d_totals against its capacities once the stream has drained.
 * n == 0 or pieces == 0: totals {0, 0}, d_out_offsets = {0}.
 * MRX_E_ARGUMENT, before anything is enqueued: negative n, piece_cap or out_cap; row_pairs < 1 or pair out of range; a
 * misaligned d_spans; a bad pitch; a null required pointer (d_offsets, d_prefix, d_out_offsets, d_totals; d_spans and
 * d_owner when piece_cap > 0; d_out_data when out_cap > 0).
 * Reads: as filter, a piece's bytes are fetched as the aligned 16-byte words that hold them, so up to 15 bytes in
 * front of a piece's first byte and behind its last one are read (never used); no word is read for an empty piece.
 * Scratch: 16 bytes per piece of capacity (piece_cap, not pieces: the sizes are scanned over the host-known
 * capacity) and the scan's block sums, returned to the arena when the call returns. */
int mrx_gather_spans_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, const int64_t* d_prefix,
                         const int32_t* d_spans, int32_t row_pairs, int32_t pair, int64_t piece_cap, int64_t* d_owner,
                         int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals,
                         void* stream);
int mrx_gather_spans_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                                 const int64_t* d_prefix, const int32_t* d_spans, int32_t row_pairs, int32_t pair,
                                 int64_t piece_cap, int64_t* d_owner, int64_t* d_out_offsets, uint8_t* d_out_data,
                                 int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);
/* extract: findall's matches as bytes, in one call (re.findall's strings; the reference's Match.get_match_text() per
 * match).  d_piece_prefix int64[n + 1] receives findall's CSR (d_counts_prefix of mrx_findall_dev); the other outputs
 * and both capacities are the primitive's, and the pieces are exactly the bytes under mrx_findall_dev's spans, in its
 * order -- the empty matches of z* and the overlapping occurrences of an exact literal included.  The spans themselves
 * live in scratch (8 more bytes per piece of capacity: a result that fits has at most piece_cap spans).
 * mrx_extract_dev on a CSR batch pays findall's one read-back of the batch's bounds before its scan can be enqueued;
 * the _known and _strided forms with totals == NULL enqueue and return.  Null handle: MRX_E_ARGUMENT.  A pattern whose
 * findall is refused is refused here, MRX_E_UNSUPPORTED with the same text, before anything is enqueued. */
int mrx_extract_dev(const mrx_handle* h, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                    int64_t* d_piece_prefix, int64_t* d_owner, int64_t* d_out_offsets, int64_t piece_cap,
                    uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);
int mrx_extract_known_dev(const mrx_handle* h, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                          int64_t end_offset, int64_t max_text_len, int64_t* d_piece_prefix, int64_t* d_owner,
                          int64_t* d_out_offsets, int64_t piece_cap, uint8_t* d_out_data, int64_t out_cap,
                          int64_t* d_totals, int64_t* totals, void* stream);
int mrx_extract_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len,
                            int64_t n, int64_t* d_piece_prefix, int64_t* d_owner, int64_t* d_out_offsets,
                            int64_t piece_cap, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals,
                            void* stream);

/* ---- expand: one templated record per match as a new packed batch on the device ----
 * Python's [m.expand(t) for m in re.finditer(p, s)], sed -n 's/.../.../p': per match ONE record, the template with each
 * \j replaced by the bytes of the match's group j -- the bytes mrx_sub_dev puts in place of that match.  It is defined on
 * the rows of mrx_captures_all_*, with no matcher of its own.
 * The primitive, mrx_expand_spans_*, needs no pattern: it takes rows that captures_all left on the device.
 *   d_prefix int64[n + 1]            CSR over the texts: text i owns the rows [d_prefix[i], d_prefix[i + 1])
 *   d_rows int32[rows][row_pairs][2] the rows, 8-byte aligned: row_pairs = g + 1 pairs each, groups 1..g, then the match
 *   tpl, tpl_len                     the template, in the one template grammar of the library (mrx_sub_dev's): only \1..\9
 *                                    are references, every other byte is literal -- \0, \\ and a trailing \ stay as they
 *                                    are.  Any length and any number of references; an empty template is allowed
 *   piece_cap                        capacity, in records, of d_owner and d_out_offsets
 * pieces = d_prefix[n], read on the device; record r belongs to the text i with d_prefix[i] <= r < d_prefix[i + 1].  Its
 * bytes are the template's with each \j replaced by pair j - 1 of row r clamped to the text as mrx_gather_spans_dev
 * clamps a pair (s' = min(max(s, 0), L), e' = min(max(e, s'), L)): a group without an entry, (-1, -1), contributes
 * nothing, a fixed-width group that reaches behind its text is cut, and so does a reference to a group the rows do not
 * hold (j > row_pairs - 1: nothing).  A template without references gives every match the same record; an empty template
 * gives empty records, whose offset repeats.  The output may hold more bytes than the input.
 * Outputs (d_owner, d_out_offsets, d_out_data, d_totals = {pieces, bytes}), both capacity rules (pieces > piece_cap, then
 * bytes > out_cap), totals == NULL (nothing is read back, the call returns without synchronising) and n == 0 are those
 * of mrx_gather_spans_dev, word for word; the output is a CSR batch and the input of a following call as it stands (a
 * record is at most tpl_len + references x the longest text long -- NOT at most the longest text).
 * MRX_E_ARGUMENT, before anything is written or enqueued: negative n, piece_cap or out_cap; row_pairs < 1; a null tpl
 * with tpl_len > 0; a misaligned d_rows; a bad pitch; a null required pointer (d_offsets, d_prefix, d_out_offsets,
 * d_totals; d_rows and d_owner when piece_cap > 0; d_out_data when out_cap > 0).
 * Reads: as mrx_gather_spans_dev, the aligned 16-byte words that hold a group's bytes are read, so up to 15 bytes in
 * front of and behind them (never used); no word is read for a group without a byte.  The literals are read the same
 * way from the call's own padded device copy, never from around `tpl`.
 * Scratch: 16 bytes per record of capacity, 8 more per distinct referenced group, the parsed template and the scan's
 * block sums, returned to the arena when the call returns. */
int mrx_expand_spans_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, const int64_t* d_prefix,
                         const int32_t* d_rows, int32_t row_pairs, const char* tpl, size_t tpl_len, int64_t piece_cap,
                         int64_t* d_owner, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                         int64_t* totals, void* stream);
int mrx_expand_spans_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                                 const int64_t* d_prefix, const int32_t* d_rows, int32_t row_pairs, const char* tpl,
                                 size_t tpl_len, int64_t piece_cap, int64_t* d_owner, int64_t* d_out_offsets,
                                 uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);
/* expand with the matcher in front: mrx_captures_all_dev with `count` (at most that many matches per text, 0 = all),
 * its rows in scratch ((g + 1) * 8 bytes per match of capacity), then the primitive.  d_match_prefix int64[n + 1]
 * receives captures_all's CSR; match_cap is the capacity, in matches, of d_owner and d_out_offsets (piece_cap above).
 * The matches are captures_all's, which are not always findall's (see mrx_captures_all_dev).
 * captures_all returns its total through one stream synchronisation, and this call inherits it: the primitive then runs
 * over exactly the rows found, not over match_cap.  With totals == NULL nothing more is read back -- a shortage of
 * out_cap is for the caller to find in d_totals, as for the primitive, while a shortage of match_cap, which the host
 * knows from captures_all, still returns MRX_E_CAPACITY (d_totals = {matches, 0}, no byte written).
 * Null handle, negative count or match_cap: MRX_E_ARGUMENT.  A pattern that captures_all refuses is refused here with
 * the same code and text, before anything is enqueued.  There is no _known form: captures_all has none. */
int mrx_expand_dev(const mrx_handle* h, const char* tpl, size_t tpl_len, int64_t count, const uint8_t* d_data,
                   const int64_t* d_offsets, int64_t n, int64_t* d_match_prefix, int64_t* d_owner, int64_t* d_out_offsets,
                   int64_t match_cap, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);
int mrx_expand_strided_dev(const mrx_handle* h, const char* tpl, size_t tpl_len, int64_t count, const uint8_t* d_data,
                           int64_t stride, const int32_t* d_lens, int32_t len, int64_t n, int64_t* d_match_prefix,
                           int64_t* d_owner, int64_t* d_out_offsets, int64_t match_cap, uint8_t* d_out_data, int64_t out_cap,
                           int64_t* d_totals, int64_t* totals, void* stream);

/* ---- distinct: the unique texts of a batch and their counts, grouped on the device ----
 * sort | uniq -c without the sort; dict.fromkeys(texts) and collections.Counter(texts).  No pattern is involved: the call
 * takes any batch, typically the pieces that extract left on the device.  Two texts are EQUAL when their lengths and
 * their bytes are equal (the empty text is a value like any other).  The groups of equal texts are numbered in the
 * order of their first occurrence.  With n texts and u groups, all on the device:
 *   d_group_of int64[n]         the group of text i
 *   d_first int64[n]            [0, u): the lowest index of a text of group g; strictly increasing
 *   d_counts int64[n]           [0, u): the number of texts in group g; they add up to n
 *   d_out_offsets int64[n + 1]  [0, u]: the CSR of the values; value g is text d_first[g]; d_out_offsets[u] = bytes
 *   d_out_data uint8[out_cap]   the values back to back; any alignment
 *   d_totals int64[2]           {u, bytes}
 * Entries of d_first, d_counts and d_out_offsets past those are unspecified.  The values are a CSR batch whatever the
 * input form, and the input of a following call as they stand (with bytes and the input's longest text as known bounds).
 * The result is a pure function of the input, bit for bit: which lane wins a race inside the kernels decides only
 * which member of a group stands for it in scratch, never an output.  A hash decides nothing by itself: two texts share
 * a group only after their bytes have been compared.
 * No byte of d_out_data at or past bytes, nor at or past out_cap, is ever written, and no element of the n-sized arrays
 * at or past n (n + 1 for d_out_offsets).
 * Capacity: u <= n, so arrays of n always fit, and out_cap = the input's byte count always suffices.  When bytes >
 * out_cap, d_group_of, d_first, d_counts, d_out_offsets and d_totals are still complete and correct, NO value byte is
 * written, and a call with `totals` returns MRX_E_CAPACITY with totals filled (filter's contract).
 * totals (host, int64[2], may be NULL) receives d_totals: the call then reads back once, at its end -- no host decision
 * sits between its kernels.  With totals == NULL nothing is read back and the call returns without synchronising; the
 * caller checks d_totals[1] against its out_cap once the stream has drained.
 * The _known form takes a CSR batch's d_offsets[n] and longest text as mrx_filter_known_dev does; they choose between
 * filter's two byte movers and size nothing.  Upper bounds are fine.
 * n == 0 gives u = bytes = 0 and d_out_offsets = {0}.  MRX_E_ARGUMENT, before any device call: negative n, out_cap or
 * known bounds; a bad pitch; a null required pointer (d_offsets, d_out_offsets, d_totals; d_group_of, d_first and
 * d_counts when n > 0; d_out_data when out_cap > 0); n >= 2^31 (a table slot keeps a text's index in 32 bits).
 * The table is open addressing at a load of at most one half, probed at most table-size times: a probe that ran out
 * (it cannot, at that load) is reported as MRX_E_ARGUMENT by a call with `totals`, and as d_totals = {-1, -1} with no
 * byte written otherwise.
 * Reads: as filter, a text's bytes are fetched as the aligned 16-byte words that hold them, so up to 15 bytes in front
 * of a text's first byte and behind its last one are read (never used: they are masked before the hash and the
 * comparison see them); no word is read for an empty text.
 * Scratch: 60 bytes per text (hash 8, representative 4, first index and count of a representative 8 + 8, flags and
 * kept lengths 8 + 8, the two scans 8 + 8), the scans' block sums and the table, 8 bytes times the power of two >= 2 n
 * (16 to 32 bytes per text), returned to the arena when the call returns. */
int mrx_distinct_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_group_of, int64_t* d_first,
                     int64_t* d_counts, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                     int64_t* totals, void* stream);
int mrx_distinct_known_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset,
                           int64_t max_text_len, int64_t* d_group_of, int64_t* d_first, int64_t* d_counts,
                           int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                           int64_t* totals, void* stream);
int mrx_distinct_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                             int64_t* d_group_of, int64_t* d_first, int64_t* d_counts, int64_t* d_out_offsets,
                             uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);

/* ---- dictionaries: look up and filter a batch's texts against a value set ----
 * grep -F -x -f list, isin, vocab.index(token): where distinct answers a question about one batch, a dictionary relates
 * a batch to a second set of texts.  A dictionary is an immutable handle built once from a batch of m texts, the ENTRIES,
 * and probed by any number of later batches.  Two texts are EQUAL as for distinct: equal lengths and equal bytes; the
 * empty text is an entry like any other, and "a" and "a\0" differ.
 * Lookup: d_index int64[n], on the device; d_index[i] is the LOWEST j with entry j equal to text i, and -1 when there is
 * none.  Duplicates among the entries are allowed and the lowest index stands for them.  The result is a pure function of
 * the entries and the text: which lane won a race during the build decides nothing a caller can see.  A hash decides
 * nothing by itself: an index is reported only after the bytes have been compared.
 * Build: mrx_dict_build_* copies the entries into device memory that the handle owns (a packed CSR made with filter's byte
 * movers; plain device memory, not the per-call scratch arena, beside the table, 8 bytes times the power of two >= 2 m, and
 * 8 bytes an entry of offsets), so the caller's batch may be freed as soon as the build returns.  The build synchronises
 * the stream twice: once to learn the entries' byte count, which sizes the copy, and once at its end.  Its scratch, 44
 * bytes an entry and a scan's block sums, goes back to the arena when it returns.  m == 0 is a valid dictionary: every
 * lookup answers -1.  m >= 2^31: MRX_E_ARGUMENT (a table slot keeps a text's index in 32 bits).  The table is distinct's:
 * open addressing at a load of at most one half, probed at most table-size times; a build whose probe ran out (it cannot,
 * at that load) returns MRX_E_ARGUMENT and no handle.  On any error *out is left as it was.
 * The handle is immutable after the build.  Lookups and filters only read it, so concurrent calls on one handle, from
 * several threads and on several streams, are safe, as for mrx_handle.  mrx_dict_free(NULL) is a no-op; a handle must not
 * be freed while a call on it is still running on some stream.  mrx_dict_size is m, mrx_dict_distinct the number of
 * different entries (both 0 for NULL).
 * mrx_dict_lookup_* enqueues one kernel and returns: it needs no scratch, reads nothing back and never synchronises.  It
 * writes exactly d_index[0, n); n == 0 writes nothing.
 * mrx_dict_filter_*: the contract is mrx_filter_dev's, word for word -- the outputs d_kept_idx, d_out_offsets, d_out_data
 * and d_totals, both capacity rules (out_cap = the input's byte count always suffices; when bytes > out_cap the indices,
 * the offsets and d_totals are complete, NO output byte is written, and a call with `totals` returns MRX_E_CAPACITY with
 * totals filled), totals == NULL (nothing is read back, the call is asynchronous, the gather decides on the device), the
 * _known bounds (upper bounds are fine; they choose between filter's byte movers) and n == 0 (kept = bytes = 0,
 * d_out_offsets = {0}) -- with the predicate d_index[i] >= 0: text i is KEPT when it equals some entry.
 * MRX_FILTER_INVERT keeps the texts that equal no entry.  MRX_FILTER_ALL is ignored, as it is for one pattern; any other
 * flag bit: MRX_E_ARGUMENT.  d_index int64[n] may be NULL; when given it also receives the lookup result of every input
 * text, kept or not.  Scratch: filter's 32 bytes per text, and 8 more when d_index is NULL.
 * MRX_E_ARGUMENT, before any device call: negative n, m or out_cap; negative known bounds; a bad pitch; a null handle; a
 * null required pointer (d_offsets; out for a build; d_index for a lookup with n > 0; for a filter d_out_offsets,
 * d_totals, d_kept_idx when n > 0 and d_out_data when out_cap > 0).
 * Reads: as distinct, a text's bytes are fetched as the aligned 16-byte words that hold them, so up to 15 bytes in front
 * of a text's first byte and behind its last one are read (never used: they are masked before the hash and the comparison
 * see them) and no word is read for an empty text.  That holds for the probed batch and, during the build, for the
 * entries; the handle's copy is padded so that the aligned words around its first and last entry are the handle's own. */
typedef struct mrx_dict mrx_dict;
int mrx_dict_build_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t m, void* stream, mrx_dict** out);
int mrx_dict_build_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t m,
                               void* stream, mrx_dict** out);
void mrx_dict_free(mrx_dict* d);
int64_t mrx_dict_size(const mrx_dict* d);
int64_t mrx_dict_distinct(const mrx_dict* d);
int mrx_dict_lookup_dev(const mrx_dict* d, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_index,
                        void* stream);
int mrx_dict_lookup_strided_dev(const mrx_dict* d, const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len,
                                int64_t n, int64_t* d_index, void* stream);
int mrx_dict_filter_dev(const mrx_dict* d, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        int64_t* d_index, int64_t* d_kept_idx, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                        int64_t* d_totals, int64_t* totals, void* stream);
int mrx_dict_filter_known_dev(const mrx_dict* d, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                              int64_t end_offset, int64_t max_text_len, int64_t* d_index, int64_t* d_kept_idx,
                              int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals,
                              void* stream);
int mrx_dict_filter_strided_dev(const mrx_dict* d, uint32_t flags, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                                int32_t len, int64_t n, int64_t* d_index, int64_t* d_kept_idx, int64_t* d_out_offsets,
                                uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);

/* ---- sort: the stable ascending order of a batch's texts, and their dense ranks ----
 * sort, sort -u, the sorted vocabulary: sorted(range(n), key=texts.__getitem__) and numpy.unique(texts,
 * return_inverse=True).  No pattern is involved: the call takes any batch.  Texts COMPARE as Python's bytes do: bytewise
 * and unsigned (0x80 sorts above 0x7f), a proper prefix before the longer text ("" < "a" < "a\0" < "a\0\0" < "aa"),
 * and equal texts keep ascending index order: the sort is stable.  With n texts and u different ones, all on the device:
 *   d_order int64[n]    d_order[p] is the index of the text at sorted position p
 *   d_rank int64[n]     (may be NULL) the number of different texts smaller than text i; equal texts share a rank
 *   d_totals int64[1]   (may be NULL) {u}
 * The result is a pure function of the input, bit for bit: no hash is involved, every output element is written once,
 * by the one lane that the key order assigns to it, and no race decides anything.
 * Exactly [0, n) of each array is written.  n == 0 writes nothing but d_totals = {0}.  To move the texts into that
 * order, pass d_order to mrx_take_dev.
 * MRX_E_ARGUMENT, before any device call: negative n or known bounds; a bad pitch; a null required pointer (d_offsets;
 * d_order when n > 0); n >= 2^31 (a round keeps a text's index in 32 bits).
 * Rounds and synchronisation: the order is refined 8 bytes of the texts a round.  After round r (r = 0, 1, ...) a
 * position is final unless its text shares its first 8 (r + 1) bytes with more than 64 others and all of them go on
 * beyond those bytes (equal texts are final with the word in which they end); a run of at most 64 such texts is
 * finished at once by comparing them with each other, however long they are.
 * The call synchronises the stream ONCE PER ROUND (it reads one word: how many positions are left) and returns when
 * none is left, without a further synchronisation: the outputs are complete once the stream has drained.  A batch takes
 * at most longest / 8 + 1 rounds (one less when the longest text is a multiple of 8 bytes and known to the host);
 * typical batches (words, fields, log pieces) take one or two.  The worst case is a
 * batch in which more than 64 different texts share a long prefix: one round per 8 bytes of it.
 * The _known form takes a CSR batch's d_offsets[n] and longest text as mrx_filter_known_dev does.  The longest text
 * spares the radix passes over bytes that no text has, and the round that would only find that texts of that length have
 * ended (a fixed pitch is such a bound by itself).  An upper bound is
 * fine; one that is too small gives a wrong order, never an access outside the caller's buffers.
 * Reads: as distinct, a text's bytes are fetched as the aligned 16-byte words that hold them, so up to 15 bytes in front
 * of a text's first byte and behind its last one are read (never used: they are masked before a key or a comparison
 * sees them); no word is read for an empty text.
 * Scratch: 76 bytes per text (two copies of a round's key and text index, 8 + 8 + 4 each; output positions 4 + 4; group
 * heads 4; flags, a scan and the distinct-value flags 8 + 8 + 8), 4 KiB per 2048 texts of digit counts and the scans'
 * block sums, returned to the arena when the call returns. */
int mrx_sort_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_order, int64_t* d_rank,
                 int64_t* d_totals, void* stream);
int mrx_sort_known_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset, int64_t max_text_len,
                       int64_t* d_order, int64_t* d_rank, int64_t* d_totals, void* stream);
int mrx_sort_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                         int64_t* d_order, int64_t* d_rank, int64_t* d_totals, void* stream);

/* ---- take: the texts at given indices as a new packed batch ----
 * texts[index] for an index array: output text j is input text d_index[j].  d_index is int64[k] on the device, in any
 * order and with repeats, and k may exceed n.  All on the device:
 *   d_out_offsets int64[k + 1]  the CSR of the output; d_out_offsets[k] = bytes
 *   d_out_data uint8[out_cap]   the selected texts back to back; any alignment
 *   d_totals int64[2]           {k, bytes}
 * The output is a CSR batch whatever the input form, and the input of a following call as it stands (with bytes and the
 * input's longest text as known bounds).  No byte of d_out_data at or past bytes, nor at or past out_cap, is ever
 * written, and no element of d_out_offsets past k.
 * Capacity and totals are filter's: when bytes > out_cap, d_out_offsets and d_totals are still complete and correct, NO
 * output byte is written, and a call with `totals` returns MRX_E_CAPACITY with totals filled.  totals (host, int64[2],
 * may be NULL) receives d_totals: the call then reads back once, at its end.  With totals == NULL nothing is read back
 * and the call returns without synchronising; the caller checks d_totals against its out_cap once the stream has
 * drained.  Repeats make the input's byte count no bound on bytes.
 * An index outside [0, n) is found on the device and cannot be refused before the call: it gives d_totals = {-1, -1}
 * with no output byte written (d_out_offsets is then unspecified), and MRX_E_ARGUMENT from a call with `totals`, as
 * distinct reports its exhausted probe.
 * k == 0 gives d_totals = {0, 0} and d_out_offsets = {0}.  MRX_E_ARGUMENT, before any device call: negative n, k, out_cap
 * or known bounds; a bad pitch; a null required pointer (d_offsets, d_out_offsets, d_totals; d_index when k > 0;
 * d_out_data when out_cap > 0).
 * The _known form takes a CSR batch's d_offsets[n] and longest text as mrx_filter_known_dev does; they choose between
 * filter's two byte movers and size nothing.  Upper bounds are fine.
 * Reads: as filter.  Scratch: 8 bytes per index and a scan's block sums. */
int mrx_take_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, const int64_t* d_index, int64_t k,
                 int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals,
                 void* stream);
int mrx_take_known_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset, int64_t max_text_len,
                       const int64_t* d_index, int64_t k, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                       int64_t* d_totals, int64_t* totals, void* stream);
int mrx_take_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                         const int64_t* d_index, int64_t k, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                         int64_t* d_totals, int64_t* totals, void* stream);

/* ---- sorted index: bisect, prefix ranges and the longest prefix against sorted entries ----
 * bisect.bisect_left / bisect_right on a sorted vocabulary, look prefix file, the merge step of join and comm, a route or
 * block table by prefix: where sort puts one batch in order, a sorted index answers questions of that order for other
 * batches.  It is an immutable handle built once from a batch of m texts, the ENTRIES, in any layout, and probed by any
 * number of later batches, as a dictionary is.  The order is sort's, word for word: bytewise and unsigned, a proper prefix
 * first ("" < "a" < "a\0" < "aa"), equal entries in ascending original index.  POSITIONS are positions 0..m in that
 * sorted order; order[p] is the original index of the entry at position p.
 * Search: d_lo and d_hi are int64[n] on the device, and `mode` is one of
 *   MRX_SORTED_EQUAL    d_lo[i] = bisect_left(sorted, text i), d_hi[i] = bisect_right(sorted, text i): the entries equal
 *                       to text i stand at [lo, hi), and lo == hi is the insertion point when there is none
 *   MRX_SORTED_PREFIX   [d_lo[i], d_hi[i]) is exactly the positions whose entry begins with text i; without one,
 *                       lo == hi == bisect_left(text i).  The empty text gives [0, m)
 *   MRX_SORTED_LONGEST  d_lo[i] is the lowest position of the longest entry that is a prefix of text i (an entry equal to
 *                       the text counts, and so does the empty entry), -1 when no entry is one; d_hi[i] is that
 *                       entry's length, or -1
 * and any other value MRX_E_ARGUMENT.  Either output may be NULL, but not both when n > 0.  Exactly [0, n) of a given
 * array is written; n == 0 writes nothing.  m == 0 is a valid handle: EQUAL and PREFIX answer 0, 0 and LONGEST -1, -1.
 * mrx_sorted_search_* enqueues one kernel and returns: it needs no scratch, uses no atomics, reads nothing back and never
 * synchronises.  The result is a pure function of the entries and the text.  The handle is immutable after the build, so
 * concurrent searches on one handle, from several threads and on several streams, are safe.  A lane takes a probe and
 * runs about log2(m) dependent comparisons, each from the depth it has already proven against both of its bounds, so a
 * prefix that the neighbourhood shares is read once; a text of many KiB is compared by its one lane: correct, not fast.
 * LONGEST repeats a bisect_right on a shrinking prefix of the text until the entry in front of it is a prefix: one to
 * three rounds for typical tables, at most one per byte of the text.
 * Build: mrx_sorted_build_* sorts with mrx_sort_dev's own rounds, so it synchronises the stream once per round as that
 * call does, once more to learn the entries' byte count, which sizes the copy, and once at its end.  The handle owns
 * plain device memory, not the per-call scratch arena: a packed copy of the entries in sorted order (made with filter's
 * byte movers, padded as the dictionary's copy is), and PER ENTRY 8 bytes of offsets, 8 bytes of `order` and 9 bytes of
 * search aid (the entry's first 8 bytes as a big-endian word and how many of them exist), beside 9 KiB of fence posts
 * (every ceil(m / 1024)-th of those keys).  So the caller's batch may be freed as soon as the build returns.  Scratch:
 * sort's, then 8 bytes an entry.  m >= 2^31: MRX_E_ARGUMENT, as for sort.  On any error *out is left as it was.
 * mrx_sorted_free(NULL) is a no-op; a handle must not be freed while a call on it is still running on some stream.
 * mrx_sorted_size is m, mrx_sorted_distinct the number of different entries (both 0 for NULL).  mrx_sorted_order_dev
 * copies order, int64[m], into the caller's device array on `stream` (a device-to-device copy, nothing read back).
 * MRX_E_ARGUMENT, before any device call: negative n or m; a bad pitch; a null handle; a null required pointer
 * (d_offsets; out for a build; d_order when m > 0; both of d_lo and d_hi when n > 0); an unknown mode.
 * Reads: as distinct, a text's bytes are fetched as the aligned 16-byte words that hold them, so up to 15 bytes in front
 * of a text's first byte and behind its last one are read (never used: they are masked before a comparison sees them) and
 * no word is read for an empty text.  That holds for the probed batch and, during the build, for the entries; the
 * handle's copy is padded so that the aligned words around its first and last entry are the handle's own. */
#define MRX_SORTED_EQUAL 0u
#define MRX_SORTED_PREFIX 1u
#define MRX_SORTED_LONGEST 2u
typedef struct mrx_sorted mrx_sorted;
int mrx_sorted_build_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t m, void* stream, mrx_sorted** out);
int mrx_sorted_build_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t m,
                                 void* stream, mrx_sorted** out);
void mrx_sorted_free(mrx_sorted* s);
int64_t mrx_sorted_size(const mrx_sorted* s);
int64_t mrx_sorted_distinct(const mrx_sorted* s);
int mrx_sorted_order_dev(const mrx_sorted* s, int64_t* d_order, void* stream);
int mrx_sorted_search_dev(const mrx_sorted* s, uint32_t mode, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                          int64_t* d_lo, int64_t* d_hi, void* stream);
int mrx_sorted_search_strided_dev(const mrx_sorted* s, uint32_t mode, const uint8_t* d_data, int64_t stride,
                                  const int32_t* d_lens, int32_t len, int64_t n, int64_t* d_lo, int64_t* d_hi, void* stream);

/* ---- numbers: pieces parsed to int64 and float64 on the device ----
 * The step from bytes to numbers: int(piece), int(piece, 16) and float(piece) for every text of a batch, or for the
 * bytes under every span that findall, split or captures_all left on the device -- read where they lie, inside the
 * source texts; nothing is gathered in between.  No pattern is involved.
 * A PIECE is a byte range: a whole text, or a span clamped to its text exactly as mrx_gather_spans_dev clamps a pair.
 * It is parsed as a whole under one `kind`: it either is a number or it is not, and nothing is searched for inside it.
 *   MRX_NUM_INT10  [+-]?[0-9]+
 *   MRX_NUM_INT16  [+-]?(0[xX])?[0-9a-fA-F]+     "0x" with nothing behind it is malformed; the sign applies to the
 *                                                magnitude, so ffffffffffffffff is out of range, not -1
 *   MRX_NUM_FLOAT  [+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?
 * Every kind refuses whatever is outside its grammar: whitespace, underscores, "inf", "nan", NUL bytes and, for the
 * decimal and the float kind, a 0x prefix.  Any number of leading zeros, any piece length and any number of exponent
 * digits are allowed.  Each row gets a status byte and an 8-byte value:
 *   MRX_NUM_OK         parsed; the value is the number (an int64, or the bits of a double for MRX_NUM_FLOAT)
 *   MRX_NUM_EMPTY      a piece of no bytes, such as an unset group (-1, -1)
 *   MRX_NUM_MALFORMED  the piece is outside the kind's grammar
 *   MRX_NUM_RANGE      well-formed, but not answered (below)
 * A row whose status is not MRX_NUM_OK gets the caller's `fill` word, stored verbatim.
 * Integers are OK when they lie in [-2^63, 2^63 - 1]: -9223372036854775808 is OK, and -0 is 0.  An overflowing
 * magnitude saturates to MRX_NUM_RANGE; it never wraps.
 * Floats are exact or refused, never approximate.  Let d be the integer that all mantissa digits write and q the
 * exponent minus the number of fraction digits; the factors of ten of d are moved into q.  d = 0 gives +-0.0 whatever
 * q is, the sign bit kept.  Otherwise the piece is answered when d <= 2^53 and -22 <= q <= 22: the value is
 * (double)d * 10^q for q >= 0 and (double)d / 10^-q for q < 0 with the sign applied -- both operands are exact, so the
 * one IEEE operation gives the correctly rounded result, float(piece) bit for bit.  Everything else is MRX_NUM_RANGE:
 * long mantissas, 1e23, 1e999, 123e-25.  The caller can send those rows elsewhere.
 *
 * mrx_parse_*: row i is text i.  d_values int64[n] and d_status uint8[n] are written in [0, n) and nowhere else.
 * mrx_parse_spans_*: d_prefix, d_spans, row_pairs and pair are those of mrx_gather_spans_dev.  rows = d_prefix[n] is
 * read on the device and written to d_totals[0]; row r belongs to the text i with d_prefix[i] <= r < d_prefix[i + 1].
 *   d_values int64[row_cap], d_status uint8[row_cap]   [0, rows)
 *   d_owner int64[row_cap]   (may be NULL) [0, rows): the text index of each row
 *   d_totals int64[1]        {rows}
 * rows > row_cap: nothing but d_totals[0] is written.  totals (host, int64[1], may be NULL) receives d_totals: the call
 * then reads it back once, at its end, and returns MRX_E_CAPACITY in that case; with totals == NULL it enqueues and
 * returns.  n == 0 gives rows 0.
 * MRX_E_ARGUMENT, before anything is enqueued: negative n or row_cap; a kind that is none of the three; row_pairs < 1 or
 * pair out of range; a misaligned d_spans; a bad pitch; a null required pointer (d_offsets; d_values and d_status when
 * n > 0, for the spans form when row_cap > 0; d_prefix and d_totals; d_spans when row_cap > 0).
 * One kernel, a lane per row; no scratch, no atomics.  Reads: a piece's bytes are fetched as the aligned 16-byte words
 * that hold them, so up to 15 bytes in front of a piece's first byte and behind its last one are read (never used: they
 * are masked before a byte is classified); no word is read for an empty piece. */
enum { MRX_NUM_INT10 = 0, MRX_NUM_INT16 = 1, MRX_NUM_FLOAT = 2 };
enum { MRX_NUM_OK = 0, MRX_NUM_EMPTY = 1, MRX_NUM_MALFORMED = 2, MRX_NUM_RANGE = 3 };
int mrx_parse_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int32_t kind, int64_t fill,
                  int64_t* d_values, uint8_t* d_status, void* stream);
int mrx_parse_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                          int32_t kind, int64_t fill, int64_t* d_values, uint8_t* d_status, void* stream);
int mrx_parse_spans_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, const int64_t* d_prefix,
                        const int32_t* d_spans, int32_t row_pairs, int32_t pair, int32_t kind, int64_t fill,
                        int64_t row_cap, int64_t* d_values, uint8_t* d_status, int64_t* d_owner, int64_t* d_totals,
                        int64_t* totals, void* stream);
int mrx_parse_spans_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                                const int64_t* d_prefix, const int32_t* d_spans, int32_t row_pairs, int32_t pair,
                                int32_t kind, int64_t fill, int64_t row_cap, int64_t* d_values, uint8_t* d_status,
                                int64_t* d_owner, int64_t* d_totals, int64_t* totals, void* stream);

/* ---- format: number and text columns written as packed records on the device ----
 * The step from numbers back to bytes, the inverse of numbers, shaped like expand: one record per row is built from a
 * template, text columns and number columns, and the records are packed back to back as a new CSR batch, in row order.
 * The output buffer is the report as it stands, and a batch for the next call (composite keys for distinct, records
 * for a dictionary).  No pattern is involved.
 * The TEMPLATE has the one grammar of mrx_sub_dev and mrx_expand_*: \1 .. \9 are references, \j being the cell of
 * column j (1-based) in the row; every other byte is literal (\0, \\ and a trailing \ stay as they are).  A reference
 * may repeat; one to a column the call does not have contributes nothing, as expand's to a group the rows lack; an
 * empty template gives empty records whose offset repeats.
 * A COLUMN (mrx_column, host memory whose pointers are device pointers) describes the same n rows as every other one:
 *   MRX_COL_TEXT   the row's text, d_values being the batch's d_data: CSR with d_offsets int64[n + 1], or at a fixed
 *                  pitch (d_offsets NULL; stride, d_lens, len as every _strided_dev entry point has them); any
 *                  alignment; an empty text is an empty cell.  arg is not read.
 *   MRX_COL_INT10  d_values int64[n]: '-' for a negative value, then the decimal magnitude with zeros in front up to at
 *                  least K = arg digits (0 .. 20; 0 is read as 1): printf's "%.Kd".  INT64_MIN prints all its digits.
 *   MRX_COL_INT16  d_values int64[n]: '-', then the magnitude in lower-case hex without 0x, padded the same way, so
 *                  -255 is -ff: the inverse of MRX_NUM_INT16.
 *   MRX_COL_FIXED  d_values double[n]: fixed notation with P = arg digits (0 .. 9) behind the point, no point for
 *                  P = 0: printf's "%.Pf".  Correctly rounded from the exact binary value, ties to even (0.5 -> 0,
 *                  2.5 -> 2, 0.125 at P = 2 -> 0.12); the sign is the sign bit (-0.0 -> -0.000, -0.04 at P = 1 -> -0.0).
 * A FIXED cell is exact or refused, as a parsed float is: it is answered when N = round_half_even(|v| * 10^P) is below
 * 10^19, and the cell is then the digits of N, padded to P + 1, with the point put in.  No floating-point operation
 * decides this: |v| = m * 2^e with m < 2^53 (denormals: e = -1074), m * 10^P is formed in 128 bits and shifted by e,
 * rounding on the remainder.  Everything else is MRX_NUM_RANGE, NaN and the infinities included.  A number cell has at
 * most 21 bytes.
 * d_status uint8[n] (may be NULL) of a number column is what numbers wrote beside the values: a cell whose byte is not
 * MRX_NUM_OK contributes NOTHING, so a fill word is never printed; nor does a RANGE cell.  It is not read for a text
 * column.  d_row_status uint8[n] (may be NULL) receives MRX_NUM_OK when every referenced cell of the row was written,
 * else the status of the lowest-numbered referenced column whose cell was not: its input byte as it is, or
 * MRX_NUM_RANGE.
 * Outputs, capacity and totals are take's, word for word:
 *   d_out_offsets int64[n + 1]  the CSR of the records; d_out_offsets[n] = bytes
 *   d_out_data uint8[out_cap]   the records back to back; any alignment
 *   d_totals int64[2]           {n, bytes}
 * No byte of d_out_data at or past bytes, nor at or past out_cap, is ever written, and no element of d_out_offsets past
 * n.  When bytes > out_cap, d_out_offsets, d_row_status and d_totals are still complete and correct, NO output byte is
 * written, and a call with `totals` returns MRX_E_CAPACITY with totals filled.  totals (host, int64[2], may be NULL)
 * receives d_totals: the call then reads back once, at its end.  With totals == NULL nothing is read back and the call
 * returns without synchronising.  n == 0 gives d_totals = {0, 0} and d_out_offsets = {0}.  A record is at most tpl_len
 * plus, per reference, the longest text of a text column or 21 bytes long.
 * MRX_E_ARGUMENT, before any device call: negative n or out_cap; ncols outside 1 .. 9; a kind that is none of the
 * four; K outside 0 .. 20 or P outside 0 .. 9; a null tpl with tpl_len > 0; a text column with a bad pitch; a null
 * required pointer (cols; a column's d_values when n > 0; d_out_offsets; d_totals; d_out_data when out_cap > 0).
 * Three launches (k_format_sizes, a scan, k_format_gather); no atomics.  Reads: a text cell's bytes are fetched as
 * mrx_gather_spans_dev fetches a piece's, as the aligned 16-byte words that hold them and none for an empty cell; the
 * literals come from the call's own padded copy.  Scratch: 8 bytes per row, 12 per row and referenced column, a scan's
 * block sums and the template, returned to the arena when the call returns. */
enum { MRX_COL_TEXT = 0, MRX_COL_INT10 = 1, MRX_COL_INT16 = 2, MRX_COL_FIXED = 3 };
typedef struct mrx_column {
  int32_t kind, arg;        /* arg: K (INT10, INT16), P (FIXED), not read (TEXT) */
  const void* d_values;     /* int64[n] / double[n]; TEXT: the batch's d_data */
  const int64_t* d_offsets; /* TEXT, CSR: int64[n + 1]; else NULL */
  int64_t stride;           /* TEXT at a fixed pitch ... */
  const int32_t* d_lens;    /* ... with its lengths int32[n], or NULL and ... */
  int32_t len, pad_;        /* ... the common length */
  const uint8_t* d_status;  /* a number column: uint8[n], or NULL */
} mrx_column;
int mrx_format_dev(const char* tpl, size_t tpl_len, const mrx_column* cols, int32_t ncols, int64_t n, int64_t* d_out_offsets,
                   uint8_t* d_out_data, int64_t out_cap, uint8_t* d_row_status, int64_t* d_totals, int64_t* totals,
                   void* stream);

/* ---- keywords: find thousands of literals in one pass ----
 * grep -F -f list and grep -v -F -f list, keyword tagging, the search for 10^4 indicators in every log line: which of a
 * long list of literals occur INSIDE each text.  (A dictionary answers the whole-text form, grep -F -x -f list; a pattern
 * set has at most 256 members and runs every member's own call.)  A keyword set is an immutable handle built once from m
 * ENTRIES (byte strings) and probed by any number of batches.  One Aho-Corasick automaton over all entries, one pass
 * over the texts: the cost of a call does not depend on m, only the size of the table does.  No reference semantics are
 * involved; the contract is this one.
 * A HIT: entry j OCCURS in text t at [s, e) when t[s:e] == entry j.  Every occurrence counts, overlapping and nested ones
 * included: `a`, `aa`, `aaa`, `aaaa` have 18 hits in `aaaaaa`, as the overlapping findall of an exact literal.
 * Entries that are equal share the LOWEST index among them and an occurrence is reported once, under that index.  An empty
 * entry (it would occur everywhere) is MRX_E_ARGUMENT with a message that names its index.  m == 0 is valid: nothing
 * occurs.  m >= 2^31: MRX_E_ARGUMENT.
 * MRX_KW_IGNORE_CASE (build flag): ASCII A-Z are folded onto a-z in the entries and in the texts; nothing else is folded
 * and spans are unchanged.  Entries that are equal after folding are duplicates.  Any other flag bit: MRX_E_ARGUMENT.
 * Build: on the host -- a trie, failure links in breadth-first order, completed to a dense table of 4-byte words over
 * byte classes (every byte that occurs in no entry shares one class, whose column goes to the root; with
 * MRX_KW_IGNORE_CASE upper and lower case share a class), states numbered shallowest first.  mrx_kw_build takes host
 * entries (entry j = data[offsets[j], offsets[j + 1])); mrx_kw_build_dev takes a CSR batch on the device, copies it to the
 * host and synchronises the stream for that.  Both upload the automaton into device memory that the handle owns (plain
 * device memory, not the scratch arena) and synchronise once more at the end, so the entries may go when the build
 * returns.  A table (states x classes x 4 bytes) above 1 GiB is MRX_E_UNSUPPORTED with a message that gives states and
 * classes: a stated limit, never an approximation.  On any error *out is left as it was.  The handle is immutable; calls
 * on it from several threads and streams are safe; mrx_kw_free(NULL) is a no-op.  mrx_kw_size is m, mrx_kw_distinct the
 * number of different entries (0 for NULL); mrx_kw_describe writes "keywords: m=.. distinct=.. states=.. classes=..
 * lmax=.. table_bytes=.. ignore_case=.." (returns the bytes needed excluding NUL, writes at most cap).
 * Operations, over the text-batch layout of the single-pattern _dev entry points and with their argument rules:
 *   contains  d_flag uint8[n]: 1 when any entry occurs in text i
 *   count     d_count int64[n]: the number of hits in text i
 *   findall   d_text_prefix int64[n + 1], d_entries int32[total], d_spans int32[total][2] (8-byte aligned, text-relative):
 *             text i's hits are [d_text_prefix[i], d_text_prefix[i + 1]), in ascending (end, start) order -- at one end
 *             position the longest entry comes first.  The capacity rule is mrx_set_findall_dev's: total > span_cap is
 *             MRX_E_CAPACITY with *total and d_text_prefix valid, and nothing is written at or beyond span_cap (retry with
 *             *total).  total may be NULL.  n == 0 gives d_text_prefix = {0}.
 *   filter    mrx_filter_dev's contract word for word (outputs, both capacity rules, totals == NULL, the _known bounds,
 *             n == 0), as mrx_dict_filter_dev has it, with the predicate `contains`: text i is KEPT when some entry occurs
 *             in it; MRX_FILTER_INVERT keeps the texts in which no entry occurs; MRX_FILTER_ALL is ignored; any other flag
 *             bit is MRX_E_ARGUMENT.
 * How: every text is cut into pieces of P bytes; a piece walks from the root, beginning Lmax - 1 bytes (the longest
 * entry's length less one) in front of its first byte but never in front of the text, and reports exactly the hits
 * whose last byte lies in it.  Pieces are independent, so one decomposition serves every batch shape, a few texts of many
 * MiB included.  k_kw_count writes one hit count per piece; ONE exclusive scan of those gives count, contains and
 * d_text_prefix (differences and values at the texts' first pieces); k_kw_emit walks the pieces that have hits again and
 * writes them at scan[piece].  No memory atomics: every result is a pure function of entries and texts, whichever lane
 * ran first.  P: 8 x (Lmax - 1) rounded up to 16, 1024 at least; halved (down to 2 x (Lmax - 1), 64 at least) while the
 * batch has fewer than 2^18 pieces.
 * Synchronisation: contains, count and a filter with totals == NULL enqueue and return; findall synchronises once, for
 * the total.  A CSR batch without known bounds adds one synchronisation for its byte count; the _known forms (findall,
 * filter) spare it, and upper bounds are fine.
 * Reads: a text's bytes are fetched as the aligned 16-byte words that hold them, so up to 15 bytes in front of a text's
 * first byte and behind its last one are read and never used: no byte outside [0, len) of a text reaches a state or a
 * hit, the last bytes of the previous text of a packed CSR batch included.  No word is read for an empty text.
 * Scratch: 16 bytes per piece and a scan's block sums; a CSR batch 16 bytes per text more; filter's 32 bytes per text.
 * MRX_E_ARGUMENT, before any device call: negative n, m, span_cap or out_cap; negative known bounds; a bad pitch; a null
 * handle; unknown flag bits; a null required pointer (offsets, out; d_offsets; the output of contains / count when
 * n > 0; d_text_prefix; d_entries and d_spans when n > 0 and span_cap > 0; filter's as mrx_filter_dev); d_spans not 8-byte
 * aligned. */
enum { MRX_KW_IGNORE_CASE = 1 };
typedef struct mrx_kw mrx_kw;
int mrx_kw_build(const uint8_t* data, const int64_t* offsets, int64_t m, uint32_t flags, void* stream, mrx_kw** out);
int mrx_kw_build_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t m, uint32_t flags, void* stream, mrx_kw** out);
void mrx_kw_free(mrx_kw* k);
int64_t mrx_kw_size(const mrx_kw* k);
int64_t mrx_kw_distinct(const mrx_kw* k);
size_t mrx_kw_describe(const mrx_kw* k, char* buf, size_t cap);
int mrx_kw_contains_dev(const mrx_kw* k, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, uint8_t* d_flag,
                        void* stream);
int mrx_kw_contains_strided_dev(const mrx_kw* k, const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len,
                                int64_t n, uint8_t* d_flag, void* stream);
int mrx_kw_count_dev(const mrx_kw* k, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_count,
                     void* stream);
int mrx_kw_count_strided_dev(const mrx_kw* k, const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len,
                             int64_t n, int64_t* d_count, void* stream);
int mrx_kw_findall_dev(const mrx_kw* k, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_text_prefix,
                       int32_t* d_entries, int32_t* d_spans, int64_t span_cap, int64_t* total, void* stream);
int mrx_kw_findall_known_dev(const mrx_kw* k, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                             int64_t end_offset, int64_t max_text_len, int64_t* d_text_prefix, int32_t* d_entries,
                             int32_t* d_spans, int64_t span_cap, int64_t* total, void* stream);
int mrx_kw_findall_strided_dev(const mrx_kw* k, const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len,
                               int64_t n, int64_t* d_text_prefix, int32_t* d_entries, int32_t* d_spans, int64_t span_cap,
                               int64_t* total, void* stream);
int mrx_kw_filter_dev(const mrx_kw* k, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                      int64_t* d_kept_idx, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                      int64_t* totals, void* stream);
int mrx_kw_filter_known_dev(const mrx_kw* k, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                            int64_t end_offset, int64_t max_text_len, int64_t* d_kept_idx, int64_t* d_out_offsets,
                            uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);
int mrx_kw_filter_strided_dev(const mrx_kw* k, uint32_t flags, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                              int32_t len, int64_t n, int64_t* d_kept_idx, int64_t* d_out_offsets, uint8_t* d_out_data,
                              int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);

/* ---- keywords: leftmost-longest matches and replacement ----
 * Rewrite by dictionary: redact 10^4 names in every log line, normalise spellings against a vocabulary, entity tables,
 * sed -f with thousands of s/literal/replacement/g, greedy tokenisation.  (mrx_set_sub_dev has at most 256 members, runs
 * every member's own findall and resolves equal starts by member order; mrx_kw_findall_dev reports every overlapping and
 * nested occurrence.)
 * THE LEFTMOST-LONGEST MATCHES of a keyword set in a text t.  Set pos = 0 and repeat: take the smallest s >= pos at which
 * some entry occurs; among the entries that occur at s take the longest, [s, e); report it and set pos = e.  Equal
 * entries stand under their lowest index, as everywhere in a keyword set.  With MRX_KW_IGNORE_CASE entries and text are
 * compared folded and spans are unchanged.  No entry is empty, so every match has at least one byte.  With count > 0 only
 * the first `count` matches of each text are kept (count == 0: all).  This is what re.finditer of the escaped entries,
 * longest first, joined by `|` yields, and aho-corasick's LeftmostLongest.
 *   leftmost  d_text_prefix int64[n + 1], d_entries int32[total], d_spans int32[total][2] (8-byte aligned,
 *             text-relative): text i's kept matches are [d_text_prefix[i], d_text_prefix[i + 1]), in ascending start
 *             order.  The capacity rule is mrx_kw_findall_dev's: total > span_cap is MRX_E_CAPACITY with *total and
 *             d_text_prefix valid, and nothing is written at or beyond span_cap (retry with *total).  total may be NULL.
 *             n == 0 gives d_text_prefix = {0}.
 *   sub       the output is every text with each kept match replaced; every other byte is copied unchanged, also under
 *             MRX_KW_IGNORE_CASE: only the comparison folds.  The replacements are a CSR batch ON THE DEVICE with r rows
 *             (row j = d_repl_data[d_repl_offsets[j], d_repl_offsets[j + 1])): r == 1, one replacement for every entry;
 *             r == m (mrx_kw_size), a match reported under entry j takes row j; any other r is MRX_E_ARGUMENT.  The bytes
 *             are taken verbatim: there is no template grammar, and a backslash is a byte.  An empty replacement deletes
 *             the match.  The aligned 16-byte words around a replacement must be readable, as for texts.
 *             d_out_offsets int64[n + 1] and d_out_data are the output as a packed CSR batch; d_nsub int32[n] (or NULL)
 *             the replacements made in every text; d_totals int64[3] (device, or NULL) and totals int64[3] (host, or
 *             NULL) = {output bytes, longest output text, replacements}.  Output bytes > out_cap is MRX_E_CAPACITY:
 *             nothing is written at or beyond out_cap (no output byte at all), and d_out_offsets, d_nsub and the totals
 *             are valid for the retry, as mrx_set_sub_dev leaves them.  With totals == NULL the call only enqueues its
 *             last steps and the verdict is the caller's to read from d_totals.  m == 0 or no match: the output is the
 *             input.  n == 0 gives d_out_offsets = {0} and totals of 0.
 * How.  The handle keeps a host copy of its folded entries; the first leftmost / sub call builds the automaton of the
 * REVERSED entries from it and uploads it, once (the handle stays immutable and thread-safe for its callers).  A reversed
 * table above 1 GiB is MRX_E_UNSUPPORTED with states and classes in the message, at that call and every later one of
 * the two; every other operation on the handle still works.  A piece [p, pend) of P bytes (the pieces of findall) is
 * walked from min(len, pend + Lmax - 1) DOWN to p: after the step that consumes byte q the state's outputs are the
 * entries that begin at q, the longest first, so every position gives at most one CANDIDATE, and the right-hand
 * warm-up never leaves the text.  A candidate is a HEAD when every earlier candidate of its text ends at or before its
 * start; a head is selected whatever came before it, so a lane per piece starts the sequential selection at the first
 * head of its piece and stops in front of the first head of a later piece (a running maximum of the ends, seeded from
 * the ceil((Lmax - 1) / P) pieces in front, decides both).  Every flag has exactly one writer: no memory atomics, and
 * the same bits on every run.  A text with no head behind its first candidate -- `aa` in `aaaa...` -- is walked end to
 * end by one lane: exact, and as slow as one lane is (profiles/kw_sub.md).  The output of sub is described as rows
 * (length, source address): per kept match the copied stretch in front of it and its replacement, per text a tail; one
 * exclusive scan of the lengths gives d_out_offsets, and the bytes are moved by extract's block gather, balanced by
 * output bytes.
 * Synchronisation: one for the candidate total, which sizes the scratch; one read-back of the totals at the end (sub
 * with totals != NULL, leftmost always), behind everything that was enqueued -- the gather checks the capacity on the
 * device.  A CSR batch without known bounds adds the usual one for its byte count; the _known forms spare it.
 * Reads: the keywords rule unchanged -- only the aligned 16-byte words that hold a byte of the walked range, and no byte
 * outside [0, len) of a text reaches a state, a match or the output.
 * Scratch: 13 bytes per candidate, 24 per output row (2 x candidates + n at most), 36 per piece, 16 per text.
 * MRX_E_ARGUMENT, before any device call: the argument classes of the other keyword entry points, and negative count or
 * r, null replacement pointers where r > 0, r neither 1 nor m. */
int mrx_kw_leftmost_dev(const mrx_kw* k, int64_t count, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        int64_t* d_text_prefix, int32_t* d_entries, int32_t* d_spans, int64_t span_cap, int64_t* total,
                        void* stream);
int mrx_kw_leftmost_known_dev(const mrx_kw* k, int64_t count, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                              int64_t end_offset, int64_t max_text_len, int64_t* d_text_prefix, int32_t* d_entries,
                              int32_t* d_spans, int64_t span_cap, int64_t* total, void* stream);
int mrx_kw_leftmost_strided_dev(const mrx_kw* k, int64_t count, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                                int32_t len, int64_t n, int64_t* d_text_prefix, int32_t* d_entries, int32_t* d_spans,
                                int64_t span_cap, int64_t* total, void* stream);
int mrx_kw_sub_dev(const mrx_kw* k, const uint8_t* d_repl_data, const int64_t* d_repl_offsets, int64_t r, int64_t count,
                   const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_out_offsets, uint8_t* d_out_data,
                   int64_t out_cap, int32_t* d_nsub, int64_t* d_totals, int64_t* totals, void* stream);
int mrx_kw_sub_known_dev(const mrx_kw* k, const uint8_t* d_repl_data, const int64_t* d_repl_offsets, int64_t r, int64_t count,
                         const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset, int64_t max_text_len,
                         int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int32_t* d_nsub, int64_t* d_totals,
                         int64_t* totals, void* stream);
int mrx_kw_sub_strided_dev(const mrx_kw* k, const uint8_t* d_repl_data, const int64_t* d_repl_offsets, int64_t r, int64_t count,
                           const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                           int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int32_t* d_nsub, int64_t* d_totals,
                           int64_t* totals, void* stream);

/* ---- lines: a batch's texts cut at one separator byte, as a new packed batch on the device ----
 * The first step of a pipeline over a file: a buffer's bytes (one text, or the texts of a batch) become the batch of lines
 * that every other call takes.  No pattern and no automaton: with `sep` one byte, lines(t) is t.split(sep) with the last
 * piece dropped when it is empty.
 *   b""  -> []        b"\n" -> [b""]        b"a" -> [b"a"]        b"a\nb" and b"a\nb\n" -> [b"a", b"b"]
 *   b"\n\na" -> [b"", b"", b"a"]
 * Every separator ends a line, and an unterminated, non-empty tail is a line too: a text's line count is its separator
 * count, plus one if it is not empty and its last byte is no separator.  A line never crosses a text boundary, and bytes
 * outside a text never make or change a line.  flags:
 *   MRX_LINES_KEEPENDS      every terminated line keeps its separator (splitlines(keepends=True) restricted to sep)
 *   MRX_LINES_CRLF          needs sep == '\n' and no MRX_LINES_KEEPENDS: one '\r' directly in front of a dropped '\n' of
 *                           the same text is dropped with it.  A '\r' anywhere else stays, a text's last byte included.
 *   MRX_LINES_DROP_PARTIAL  every text's unterminated tail is left out (reading a file in chunks)
 * Outputs, all on the device, lines in text order:
 *   d_line_prefix int64[n + 1]          CSR over the texts: text i owns the lines [d_line_prefix[i], d_line_prefix[i + 1]);
 *                                       right for empty texts too, wherever they stand
 *   d_owner int64[piece_cap]            [0, lines): the text index of each line
 *   d_out_offsets int64[piece_cap + 1]  [0, lines]: the CSR of the output batch; d_out_offsets[lines] = bytes
 *   d_out_data uint8[out_cap]           the lines back to back; any alignment
 *   d_totals int64[4]                   {lines, bytes, longest line, tail}
 * tail is the byte count of the LAST text's unterminated tail, whatever the flags say (0 when it ends in a separator or
 * n == 0): a caller that reads a file in chunks carries buf[len - tail, len) into the next one.  The longest line counts
 * the separator under MRX_LINES_KEEPENDS.  The output is a CSR batch and the input of a following call as it stands, with
 * bytes and the longest line as its known bounds -- both exact.  Entries of d_owner and d_out_offsets past the lines are
 * unspecified.  No byte of d_out_data at or past bytes, nor at or past out_cap, is ever written, and no element of
 * d_owner at or past piece_cap, nor of d_out_offsets at or past piece_cap + 1.
 * Capacity.  lines > piece_cap: nothing is written to d_out_data, d_owner and d_out_offsets hold nothing of use;
 * d_line_prefix, d_totals[0] (the need), d_totals[1] and d_totals[3] are exact, d_totals[2] is 0.  lines <= piece_cap and
 * bytes > out_cap: d_line_prefix, d_owner, d_out_offsets and all four totals are complete and exact, and NO output byte is
 * written (out_cap == 0 with MRX_LINES_KEEPENDS on one text is how a caller gets the offsets of the lines inside its
 * own buffer, which the output would only repeat).  A call with `totals` returns MRX_E_CAPACITY in either case, totals
 * filled for a retry (grow the lines first, then the bytes: two retries at most).
 * totals (host, int64[4], may be NULL) receives d_totals: the call then reads back once, at its end -- no host decision
 * sits between its kernels.  With totals == NULL the call returns without synchronising behind its kernels: they decide
 * on the device from d_totals, and the caller checks d_totals against its capacities once the stream has drained.
 * n == 0 or no line: totals {0, 0, 0, tail}, d_out_offsets = {0}.
 * MRX_E_ARGUMENT, before anything is enqueued: an unknown flag; MRX_LINES_CRLF with another separator than '\n' or with
 * MRX_LINES_KEEPENDS; negative n, piece_cap, out_cap, end_offset or max_text_len; a bad pitch; a null required pointer (d_offsets, d_line_prefix,
 * d_out_offsets, d_totals; d_owner when piece_cap > 0; d_out_data when out_cap > 0).
 * Sizes: every position is 64-bit.  The CSR form serves a text of 2^31 bytes and more; the strided form keeps its int32
 * length.
 * Reads: as filter and extract, the aligned 16-byte words that hold a text's bytes, so up to 15 bytes in front of a
 * text's first byte and behind its last one are read (never used); no word is read for an empty text.
 * Scratch: 40 bytes per piece of the input (a text is cut into pieces of 4 KiB; an empty text has none), up to 48 per
 * text, and the scans' block sums: nothing is sized by a capacity.  It is returned to the arena when the call returns.  The CSR
 * form reads d_offsets[0] and d_offsets[n] back (one synchronisation, before its first kernel) to size it; the strided
 * form sizes it from its arguments and mrx_lines_known_dev from end_offset, the batch's byte count d_offsets[n] -
 * d_offsets[0] or an upper bound of it (max_text_len is not used), and neither reads anything: with totals == NULL they
 * enqueue and return.  end_offset must not be too small, and d_offsets must not decrease anywhere: the kernels index the
 * scratch with the real offsets.
 * The result is the same bit for bit on every run: no atomics, and no wavefront waits for another. */
enum { MRX_LINES_KEEPENDS = 1, MRX_LINES_CRLF = 2, MRX_LINES_DROP_PARTIAL = 4 };
int mrx_lines_dev(uint32_t flags, uint8_t sep, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                  int64_t* d_line_prefix, int64_t* d_owner, int64_t* d_out_offsets, int64_t piece_cap, uint8_t* d_out_data,
                  int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream);
int mrx_lines_known_dev(uint32_t flags, uint8_t sep, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        int64_t end_offset, int64_t max_text_len, int64_t* d_line_prefix, int64_t* d_owner,
                        int64_t* d_out_offsets, int64_t piece_cap, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                        int64_t* totals, void* stream);
int mrx_lines_strided_dev(uint32_t flags, uint8_t sep, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                          int32_t len, int64_t n, int64_t* d_line_prefix, int64_t* d_owner, int64_t* d_out_offsets,
                          int64_t piece_cap, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals,
                          void* stream);

/* ---- fields: the columns of every text as span rows on the device ----
 * What cut -d, -f2,5, awk '{print $1, $NF}' and line.split()[3] do first: for every text of a batch, the byte ranges of
 * f requested columns, one fixed-width row per text.  No pattern and no automaton.  Two modes define a text's parts:
 *   delimiter mode   (delim one byte d) parts = t.split(d): every delimiter separates and empty fields exist; the
 *                    field count is nf = count(d) + 1.  The empty text has one empty field, (0, 0): awk says NF = 0
 *                    there, this call follows Python.
 *   whitespace mode  (MRX_FIELDS_WHITESPACE, delim ignored) parts = t.split() of Python bytes: whitespace is exactly the
 *                    six bytes 0x09 .. 0x0D and 0x20; runs separate, leading and trailing runs make no field, and a
 *                    text without any other byte has nf = 0.
 * columns (host, int32[f], 1 <= f <= MRX_FIELDS_MAX_COLUMNS) may repeat and stand in any order: c > 0 names
 * parts[c - 1], as cut and awk count; c < 0 names parts[nf + c], so -1 is $NF; 0 is refused.
 *   MRX_FIELDS_REST  every column must be positive.  With cmax the largest column the parts are t.split(d, cmax - 1)
 *                    (or t.split(None, cmax - 1)): column cmax, if it exists, runs to the end of the text -- a log line's
 *                    message -- and nf is min(nf, cmax).
 * Pair j of text i's row is (start, end) of that part, relative to the text's first byte; a part that does not exist
 * gives (-1, -1), which mrx_gather_spans_* turns into an empty piece, mrx_parse_spans_* into MRX_NUM_EMPTY, and which
 * contributes nothing to mrx_expand_spans_*.  (mrx_expand_spans_* takes a row's last pair for the whole match, which no
 * reference names: \j is pair j - 1 for j < row_pairs.  A caller that expands all of its columns asks for one more.)
 *   text          call                               row                                      nf
 *   b""           ",", {1, -1}                       (0,0) (0,0)                              1
 *   b""           whitespace, {1, -1}                (-1,-1) (-1,-1)                          0
 *   b" a  b c "   whitespace, {1, 2, 3, -1}          (1,2) (4,5) (6,7) (6,7)                  3
 *   b" a  b c "   whitespace, rest, {2}              (4,8)                                    2
 *   b"a,b,,c"     ",", {3, 4, 5, -4, -5}             (4,4) (5,6) (-1,-1) (0,1) (-1,-1)        4
 *   b"a,b,,c"     ",", rest, {2}                     (2,6)                                    2
 * Outputs, all on the device:
 *   d_rows int32[n][f][2]   8-byte aligned: a captures_all row block with one row per text (row_pairs = f)
 *   d_nf int32[n]           (may be NULL) the field counts
 *   d_prefix int64[n + 1]   (may be NULL) the values 0 .. n: the identity CSR of the rows over the texts that
 *                           mrx_gather_spans_*, mrx_parse_spans_* and mrx_expand_spans_* ask for
 * No totals, no capacity and no scratch, and no synchronisation on any form: the call enqueues and returns.  n == 0
 * enqueues nothing (and writes nothing, d_prefix[0] included).  Spans are int32 (texts of up to 2 GiB - 1).  Bytes outside
 * a text never make or change a field.
 * Reads: as filter, the aligned 16-byte words that hold a text's bytes, so up to 15 bytes in front of a text's first
 * byte and behind its last one are read (never used: they are masked before a byte is compared); no word is read for an
 * empty text.  Under MRX_FIELDS_REST, and when d_nf is NULL and no column is negative, a text is read only up to the end
 * of its largest column; the results do not differ.  Negative columns read a text twice.
 * The _known form takes a CSR batch's d_offsets[n] and longest text as mrx_filter_known_dev does; here they only choose
 * the route (the lanes that share a text, from the mean length end_offset / n; the strided form takes the pitch or the
 * common length).  They size nothing, so a wrong bound costs time, never memory.
 * One kernel, a group of 1 to 64 lanes per text.  Fields are a per-line operation: a text longer than the group's
 * 16 bytes per lane takes more rounds of the same group, so one text of many MiB is answered correctly and slowly.
 * The result is the same bit for bit on every run: no atomics, and no wavefront waits for another.
 * MRX_E_ARGUMENT, before anything is enqueued: an unknown flag; f < 1 or f > MRX_FIELDS_MAX_COLUMNS; a column 0;
 * MRX_FIELDS_REST with a negative column; negative n, end_offset or max_text_len; a bad pitch; a null d_rows, d_offsets
 * or columns; a d_rows that is not 8-byte aligned. */
enum { MRX_FIELDS_WHITESPACE = 1, MRX_FIELDS_REST = 2 };
#define MRX_FIELDS_MAX_COLUMNS 32
int mrx_fields_dev(uint32_t flags, uint8_t delim, const int32_t* columns, int32_t f, const uint8_t* d_data,
                   const int64_t* d_offsets, int64_t n, int32_t* d_rows, int32_t* d_nf, int64_t* d_prefix, void* stream);
int mrx_fields_known_dev(uint32_t flags, uint8_t delim, const int32_t* columns, int32_t f, const uint8_t* d_data,
                         const int64_t* d_offsets, int64_t n, int64_t end_offset, int64_t max_text_len, int32_t* d_rows,
                         int32_t* d_nf, int64_t* d_prefix, void* stream);
int mrx_fields_strided_dev(uint32_t flags, uint8_t delim, const int32_t* columns, int32_t f, const uint8_t* d_data,
                           int64_t stride, const int32_t* d_lens, int32_t len, int64_t n, int32_t* d_rows, int32_t* d_nf,
                           int64_t* d_prefix, void* stream);

/* ---- quoted fields: CSV and log-line quoting in fields, on the device ----
 * fields with one more input, `quote` (one byte Q), and one more optional output, d_quoted: x,"Doe, Jane",42 is three
 * cells, and the request and the agent of a combined-format access log line are one column each.  flags are fields':
 * MRX_FIELDS_WHITESPACE and MRX_FIELDS_REST.  mrx_fields_* itself is unchanged, and knows no quote.
 *   inside           byte p of a text t is inside when the number of Q bytes in t[0..p], p included, is odd.  An opening
 *                    quote is inside, a closing one is not.  "" within a quoted stretch closes and opens again with
 *                    nothing between, so doubled quotes need no rule of their own.
 *   delimiter mode   a delimiter byte separates only when it is not inside.  The rest is fields': nf is the number of
 *                    separating delimiters plus 1, columns count from 1 or from -1, MRX_FIELDS_REST lets column cmax
 *                    run to L after cmax - 1 separations, and the empty text has one empty field.
 *   whitespace mode  a whitespace byte that is inside counts as a byte that is no whitespace.  Starts, ends and nf are
 *                    whitespace mode's own rules over that mask.
 *   content          let a part be [s, e) as above.  If e - s >= 2, t[s] == Q and t[e - 1] == Q, the pair written is
 *                    (s + 1, e - 1) and d_quoted[i][j] = 1.  Otherwise the pair is (s, e) and the byte is 0.  A part
 *                    that does not exist is (-1, -1) and 0.  d_quoted is uint8[n][f] and may be NULL.
 *   decoded cell     (documented, not computed by this call) the content with every leftmost non-overlapping QQ
 *                    replaced by Q: what mrx_kw_sub_* does with the one entry QQ and the replacement Q.
 * For every row that Python's csv.writer produces with QUOTE_MINIMAL or QUOTE_ALL from cells without \r and \n, the
 * decoded cells are csv.reader's.  Malformed input is defined by the rules above, not by csv:
 *   text           call                           rows                            quoted
 *   a,"b,c",d      ",", {1, 2, 3}                 (0,1) (3,6) (8,9)               0 1 0
 *   a,"b""c",d     ",", {2}                       (3,7): content b""c             1
 *   x,"",y         ",", {2}                       (3,3)                           1
 *   "a,b           ",", {1, 2}                    (0,4) (-1,-1)                   0 0
 *   a"b,c"d        ",", {1}                       (0,7): csv says two cells       0
 *   "ab"cd,e       ",", {1, 2}                    (0,6) (7,8)                     0 0
 *   "              ",", {1}                       (0,1)                           0
 *   a "b c"  d     whitespace, {1, 2, 3, -1}      (0,1) (3,6) (9,10) (9,10)       0 1 0 0
 *   a,"b,c",d      ",", rest, {2}                 (2,9)                           0
 * Bytes outside a text never make, open or close a quote: every walk of a text begins outside.  Reads are as for fields,
 * and t[s] and t[e - 1] of every part that exists are read once more.  The early stop stays where the results cannot
 * differ: under MRX_FIELDS_REST, and when d_nf is NULL and no column is negative.  No scratch, no atomics, nothing read
 * back, the same bits on every run, and no synchronisation on any form.  n == 0 enqueues nothing.
 * MRX_E_ARGUMENT, before anything is enqueued: everything mrx_fields_* refuses; quote == delim in delimiter mode; a quote
 * that is one of the six whitespace bytes in whitespace mode; a d_quoted given with d_rows NULL.
 * Forms: CSR and fixed pitch.  There is no form that takes a CSR batch's known bounds: the CSR form cannot know the mean
 * text length and shares a text among the default number of lanes (2), the fixed-pitch form routes by its pitch or length
 * as mrx_fields_strided_dev does.
 * Not here: an escape byte (\"), open / close pairs such as [ ... ], records with a newline inside quotes (mrx_lines_*
 * knows no quote), and a CSV writer. */
int mrx_fields_quoted_dev(uint32_t flags, uint8_t delim, uint8_t quote, const int32_t* columns, int32_t f, const uint8_t* d_data,
                          const int64_t* d_offsets, int64_t n, int32_t* d_rows, int32_t* d_nf, uint8_t* d_quoted,
                          int64_t* d_prefix, void* stream);
int mrx_fields_quoted_strided_dev(uint32_t flags, uint8_t delim, uint8_t quote, const int32_t* columns, int32_t f,
                                  const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                                  int32_t* d_rows, int32_t* d_nf, uint8_t* d_quoted, int64_t* d_prefix, void* stream);

/* ---- translate: bytes.translate and tr -s for every text, as a new batch on the device ----
 * The step that normalises bytes: tr A-Z a-z, tr -d '\r"', tr '\t' ' ', tr -s ' ', sed y/../../.  No pattern and no
 * automaton.  For every text t of the batch:
 *   1. u = t.translate(table, delete): the bytes of the delete set are dropped, the others go through `table`
 *   2. with a squeeze set, byte k > 0 of u is dropped when u[k] is in the set and u[k] == u[k - 1] (tr -s on the mapped
 *      bytes).  A run never reaches across a text boundary, and a text's first byte is always kept.
 * table (host, uint8[256]) may be NULL, the identity.  delete_set and squeeze_set (host, 32-byte bitmaps: byte c is a
 * member when bit c & 7 of byte c >> 3 is set) may be NULL, empty.  Both with a member in one call is refused: the byte
 * in front of a squeezed one would be the last SURVIVING byte, any distance back; two calls do it.  All three empty is
 * a copy.
 *   text            call                                       result
 *   b"GET /A b"     table = bytes.lower's                      b"get /a b"
 *   b"a\r\n"        delete {\r}                                b"a\n"
 *   b"a  b   c"     squeeze {' '}                              b"a b c"
 *   b"a\t b"        table \t -> ' ', squeeze {' '}             b"a b"         (the run exists only behind the map)
 *   b"aab"          squeeze {' '}                              b"aab"         (a run of a byte outside the set stays)
 * Same-length form (delete and squeeze empty): the output has the input's layout, so no offsets are written:
 *   CSR          byte p of d_data, d_offsets[0] <= p < d_offsets[n], goes to byte p of d_out_data: the result is the batch
 *                (d_out_data, d_offsets).  out_cap must be at least d_offsets[n].
 *   fixed pitch  the rows' region, bytes [0, (n - 1) * stride + (d_lens ? stride : len)) of both buffers: the result is
 *                the batch (d_out_data, stride, d_lens, len).  Both buffers hold that region; out_cap must be at least
 *                its size.
 * The texts of a CSR batch are contiguous, so the region is exactly the texts; the bytes of a fixed-pitch region outside
 * the texts (row padding) are unspecified in the output.  Nothing outside the region is written.  d_out_offsets,
 * d_totals and totals may be NULL and are not touched; known bounds of the input are those of the output.  One kernel,
 * a lane per aligned 16-byte block of the output region, no scratch, nothing scanned.  MRX_E_CAPACITY, before anything is
 * enqueued, when the region does not fit out_cap; mrx_translate_known_dev tells from end_offset, which must then be at
 * least d_offsets[n] (the kernel compares d_offsets[n] itself and writes nothing when it does not fit).
 * Packed form (a delete or a squeeze set): the output is a packed CSR batch:
 *   d_out_offsets int64[n + 1]   the CSR of the output; d_out_offsets[n] = bytes
 *   d_out_data uint8[out_cap]    the texts back to back; any alignment
 *   d_totals int64[2]            {bytes, longest text}, both exact: the known bounds of the output
 * The input's byte count is always capacity enough.  bytes > out_cap: d_out_offsets and d_totals are complete and exact
 * and NO output byte is written; a call with `totals` returns MRX_E_CAPACITY.  totals (host, int64[2], may be NULL)
 * receives d_totals: the call then reads back once, at its end.  With totals == NULL the call only enqueues.  n == 0:
 * totals {0, 0}, d_out_offsets = {0}.  No byte of d_out_data at or past bytes, nor at or past out_cap, is ever written.
 * Input and output must not overlap, in either form.
 * MRX_E_ARGUMENT, before anything is enqueued: delete and squeeze together; negative n, out_cap, end_offset or
 * max_text_len; a bad pitch; a null required pointer (d_offsets; d_out_data when out_cap > 0; in the packed form
 * d_out_offsets and d_totals).
 * Sizes: every position is 64-bit; the CSR form serves a text of 2^31 bytes and more, the strided form keeps its int32
 * length.  Empty texts are served wherever they stand.
 * Reads: the aligned 16-byte words that hold a text's bytes (same-length form: the region's), so up to 15 bytes in front
 * and behind are read and never used: they are masked before a byte is looked up.
 * Scratch (packed form): 16 bytes per piece of the input (a text is cut into pieces of 4 KiB; an empty text has none),
 * 16 per text of a CSR batch, and the scan's block sums; returned to the arena when the call returns.  mrx_translate_dev
 * reads d_offsets[0] and d_offsets[n] back (one synchronisation, before its first kernel); the strided form and
 * mrx_translate_known_dev (end_offset: d_offsets[n] - d_offsets[0] or an upper bound, max_text_len is not used) read
 * nothing.  end_offset must not be too small, and d_offsets must not decrease anywhere.
 * Lookup: one table of 256 entries (the mapped byte and the sets' flags) in LDS, filled once per workgroup.
 * The result is the same bit for bit on every run: no atomics, and no wavefront waits for another. */
int mrx_translate_dev(const uint8_t* table, const uint8_t* delete_set, const uint8_t* squeeze_set, const uint8_t* d_data,
                      const int64_t* d_offsets, int64_t n, uint8_t* d_out_data, int64_t out_cap, int64_t* d_out_offsets,
                      int64_t* d_totals, int64_t* totals, void* stream);
int mrx_translate_known_dev(const uint8_t* table, const uint8_t* delete_set, const uint8_t* squeeze_set,
                            const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset,
                            int64_t max_text_len, uint8_t* d_out_data, int64_t out_cap, int64_t* d_out_offsets,
                            int64_t* d_totals, int64_t* totals, void* stream);
int mrx_translate_strided_dev(const uint8_t* table, const uint8_t* delete_set, const uint8_t* squeeze_set,
                              const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                              uint8_t* d_out_data, int64_t out_cap, int64_t* d_out_offsets, int64_t* d_totals,
                              int64_t* totals, void* stream);

/* ---- strip: bytes.strip of every text as span rows on the device ----
 * For every text of L bytes one pair (start, end), relative to the text's first byte, in the shape of fields' rows with
 * f = 1.  set (host, 32-byte bitmap as above) holds the bytes to strip; NULL is the six whitespace bytes of
 * bytes.strip(): 0x09 .. 0x0D and 0x20, the ones fields splits at.
 *   start  the number of leading bytes in the set under MRX_STRIP_LEFT, else 0
 *   end    L minus the trailing bytes in the set counted inside [start, L) under MRX_STRIP_RIGHT, else L
 * A text of set bytes alone gives (L, L) with MRX_STRIP_LEFT and (0, 0) with MRX_STRIP_RIGHT alone.
 *   text        flags           row            text        flags    row
 *   b"  42 "    left | right    (2, 4)         b"   "      left     (3, 3)
 *   b"  42 "    left            (2, 5)         b"   "      right    (0, 0)
 *   b"  42 "    right           (0, 4)         b""         any      (0, 0)
 * Outputs, on the device:
 *   d_rows int32[n][1][2]   8-byte aligned
 *   d_prefix int64[n + 1]   (may be NULL) the values 0 .. n: the identity CSR of the rows over the texts, so that rows
 *                           and prefix go into mrx_gather_spans_*, mrx_parse_spans_* and mrx_expand_spans_* as they stand
 * No totals, no capacity, no scratch and no synchronisation on any form: the call enqueues and returns.  n == 0
 * enqueues nothing (and writes nothing, d_prefix[0] included).  Spans are int32 (texts of up to 2 GiB - 1).  The _known
 * form's bounds are not used.  Bytes outside a text never change a row.
 * One kernel, a lane per text: it walks the aligned 16-byte words of the text in from the front and then from the back
 * and reads only the words that hold a stripped byte or the first byte that stays.  A text of set bytes alone is walked
 * whole by its one lane: right, not fast.  Reads as translate.
 * MRX_E_ARGUMENT, before anything is enqueued: flags with an unknown bit or with none; negative n, end_offset or
 * max_text_len; a bad pitch; a null d_rows or d_offsets; a d_rows that is not 8-byte aligned. */
enum { MRX_STRIP_LEFT = 1, MRX_STRIP_RIGHT = 2 };
int mrx_strip_dev(const uint8_t* set, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                  int32_t* d_rows, int64_t* d_prefix, void* stream);
int mrx_strip_known_dev(const uint8_t* set, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        int64_t end_offset, int64_t max_text_len, int32_t* d_rows, int64_t* d_prefix, void* stream);
int mrx_strip_strided_dev(const uint8_t* set, uint32_t flags, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                          int32_t len, int64_t n, int32_t* d_rows, int64_t* d_prefix, void* stream);

/* ---- host-buffer convenience wrappers (copy in, run, copy out) -------------- */
/* mrx_translate_dev on host buffers: out_offsets int64[n + 1], out_data uint8[out_cap], totals int64[2] = {bytes, longest
 * text} (may be NULL).  The output is packed in both forms: out_offsets begins at 0 (the same-length form's are the
 * input's, relative to its first text).  out_offsets and totals are always copied out, out_data only when all of it fits
 * (MRX_E_CAPACITY otherwise). */
int mrx_translate_batch(const uint8_t* table, const uint8_t* delete_set, const uint8_t* squeeze_set, const uint8_t* data,
                        const int64_t* offsets, int64_t n, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap,
                        int64_t* totals);
/* mrx_strip_dev on host buffers: rows int32[n][2], prefix int64[n + 1] (may be NULL). */
int mrx_strip_batch(const uint8_t* set, uint32_t flags, const uint8_t* data, const int64_t* offsets, int64_t n, int32_t* rows,
                    int64_t* prefix);
/* mrx_fields_dev on host buffers: rows int32[n][f][2], nf int32[n] (may be NULL), prefix int64[n + 1] (may be NULL). */
int mrx_fields_batch(uint32_t flags, uint8_t delim, const int32_t* columns, int32_t f, const uint8_t* data,
                     const int64_t* offsets, int64_t n, int32_t* rows, int32_t* nf, int64_t* prefix);
/* mrx_fields_quoted_dev on host buffers: as mrx_fields_batch, and quoted uint8[n][f] (may be NULL). */
int mrx_fields_quoted_batch(uint32_t flags, uint8_t delim, uint8_t quote, const int32_t* columns, int32_t f, const uint8_t* data,
                            const int64_t* offsets, int64_t n, int32_t* rows, int32_t* nf, uint8_t* quoted, int64_t* prefix);
/* mrx_lines_dev on host buffers: line_prefix int64[n + 1], owner int64[piece_cap], out_offsets int64[piece_cap + 1],
 * out_data uint8[out_cap], totals int64[4] (may be NULL).  line_prefix is always copied out, owner[0, lines) and
 * out_offsets[0, lines] when the lines fit, out_data only when the bytes fit too (MRX_E_CAPACITY otherwise). */
int mrx_lines_batch(uint32_t flags, uint8_t sep, const uint8_t* data, const int64_t* offsets, int64_t n,
                    int64_t* line_prefix, int64_t* owner, int64_t* out_offsets, int64_t piece_cap, uint8_t* out_data,
                    int64_t out_cap, int64_t* totals);
/* mrx_kw_findall_dev on host buffers: text_prefix is always copied out, entries and spans only when all hits fit */
int mrx_kw_findall_batch(const mrx_kw* k, const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* text_prefix,
                         int32_t* entries, int32_t* spans, int64_t span_cap, int64_t* total);
/* mrx_kw_leftmost_dev on host buffers: text_prefix is always copied out, entries and spans only when all matches fit */
int mrx_kw_leftmost_batch(const mrx_kw* k, int64_t count, const uint8_t* data, const int64_t* offsets, int64_t n,
                          int64_t* text_prefix, int32_t* entries, int32_t* spans, int64_t span_cap, int64_t* total);
/* mrx_kw_sub_dev on host buffers, the replacements included (repl_offsets int64[r + 1]); out_offsets, nsub (may be NULL)
 * and totals int64[3] (may be NULL) are always copied out, the output's bytes only when they fit */
int mrx_kw_sub_batch(const mrx_kw* k, const uint8_t* repl_data, const int64_t* repl_offsets, int64_t r, int64_t count,
                     const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* out_offsets, uint8_t* out_data,
                     int64_t out_cap, int32_t* nsub, int64_t* totals);
/* mrx_format_dev on host buffers: the columns' pointers are host pointers (a text column's offsets may begin anywhere
 * and must not decrease); out_offsets int64[n + 1], out_data uint8[out_cap], row_status uint8[n] (may be NULL), totals
 * int64[2] = {n, bytes} (may be NULL).  out_offsets[0, n] and row_status are copied out, out_data only when all of it
 * fits (MRX_E_CAPACITY otherwise). */
int mrx_format_batch(const char* tpl, size_t tpl_len, const mrx_column* cols, int32_t ncols, int64_t n, int64_t* out_offsets,
                     uint8_t* out_data, int64_t out_cap, uint8_t* row_status, int64_t* totals);
/* mrx_parse_dev on host buffers: values int64[n], status uint8[n]. */
int mrx_parse_batch(const uint8_t* data, const int64_t* offsets, int64_t n, int32_t kind, int64_t fill, int64_t* values,
                    uint8_t* status);
/* mrx_gather_spans_dev / mrx_extract_dev on host buffers: owner int64[piece_cap], out_offsets int64[piece_cap + 1],
 * out_data uint8[out_cap], totals int64[2] = {pieces, bytes} (may be NULL); spans holds prefix[n] rows.  piece_prefix
 * (extract) is always copied out, owner[0, pieces) and out_offsets[0, pieces] when the pieces fit, out_data only when
 * the bytes fit too (MRX_E_CAPACITY otherwise). */
int mrx_gather_spans_batch(const uint8_t* data, const int64_t* offsets, int64_t n, const int64_t* prefix,
                           const int32_t* spans, int32_t row_pairs, int32_t pair, int64_t piece_cap, int64_t* owner,
                           int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals);
int mrx_extract_batch(const mrx_handle* h, const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* piece_prefix,
                      int64_t* owner, int64_t* out_offsets, int64_t piece_cap, uint8_t* out_data, int64_t out_cap,
                      int64_t* totals);
/* mrx_expand_spans_dev / mrx_expand_dev on host buffers, shaped as the two above with the same rules for what is copied
 * out when: rows holds prefix[n] rows; match_prefix (expand) is always copied out, owner[0, pieces) and
 * out_offsets[0, pieces] when the records fit, out_data only when the bytes fit too (MRX_E_CAPACITY otherwise). */
int mrx_expand_spans_batch(const uint8_t* data, const int64_t* offsets, int64_t n, const int64_t* prefix, const int32_t* rows,
                           int32_t row_pairs, const char* tpl, size_t tpl_len, int64_t piece_cap, int64_t* owner,
                           int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals);
int mrx_expand_batch(const mrx_handle* h, const char* tpl, size_t tpl_len, int64_t count, const uint8_t* data,
                     const int64_t* offsets, int64_t n, int64_t* match_prefix, int64_t* owner, int64_t* out_offsets,
                     int64_t match_cap, uint8_t* out_data, int64_t out_cap, int64_t* totals);
/* mrx_filter_dev / mrx_set_filter_dev on host buffers: kept_idx int64[n], out_offsets int64[n + 1], out_data
 * uint8[out_cap], totals int64[2] = {kept, bytes} (may be NULL).  kept_idx[0, kept) and out_offsets[0, kept] are
 * copied out, out_data only when all of it fits (MRX_E_CAPACITY otherwise). */
int mrx_filter_batch(const mrx_handle* h, uint32_t flags, const uint8_t* data, const int64_t* offsets, int64_t n,
                     int64_t* kept_idx, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals);
int mrx_set_filter_batch(const mrx_set* s, uint32_t flags, const uint8_t* data, const int64_t* offsets, int64_t n,
                         int64_t* kept_idx, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals);
/* mrx_distinct_dev on host buffers: group_of, first and counts int64[n], out_offsets int64[n + 1], out_data
 * uint8[out_cap], totals int64[2] = {u, bytes} (may be NULL).  group_of[0, n), first[0, u), counts[0, u) and
 * out_offsets[0, u] are copied out, out_data only when all of it fits (MRX_E_CAPACITY otherwise). */
int mrx_distinct_batch(const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* group_of, int64_t* first,
                       int64_t* counts, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals);
/* mrx_sort_dev on host buffers: order int64[n], rank int64[n] (may be NULL), totals int64[1] = {u} (may be NULL). */
int mrx_sort_batch(const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* order, int64_t* rank, int64_t* totals);
/* mrx_take_dev on host buffers: index int64[k], out_offsets int64[k + 1], out_data uint8[out_cap], totals int64[2] =
 * {k, bytes} (may be NULL; {-1, -1} with MRX_E_ARGUMENT behind an index outside [0, n)).  out_offsets[0, k] is copied
 * out, out_data only when all of it fits (MRX_E_CAPACITY otherwise). */
int mrx_take_batch(const uint8_t* data, const int64_t* offsets, int64_t n, const int64_t* index, int64_t k,
                   int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals);
/* mrx_dict_build_dev and mrx_dict_lookup_dev on host buffers: the entries (dict_data, dict_offsets int64[m + 1]) and the
 * texts are copied in, a dictionary is built, probed once and freed; index int64[n] receives the result. */
int mrx_dict_lookup_batch(const uint8_t* dict_data, const int64_t* dict_offsets, int64_t m, const uint8_t* data,
                          const int64_t* offsets, int64_t n, int64_t* index);
/* mrx_sorted_build_dev and mrx_sorted_search_dev on host buffers: the entries (entry_data, entry_offsets int64[m + 1]) and
 * the texts are copied in, an index is built, searched once in `mode` and freed; lo and hi int64[n] receive the result
 * (either may be NULL, not both when n > 0). */
int mrx_sorted_search_batch(const uint8_t* entry_data, const int64_t* entry_offsets, int64_t m, uint32_t mode,
                            const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* lo, int64_t* hi);
int mrx_match_first_batch(const mrx_handle* h, const uint8_t* data,
                          const int64_t* offsets, int64_t n, int32_t* start,
                          int32_t* end);
int mrx_search_batch(const mrx_handle* h, const uint8_t* data, const int64_t* offsets,
                     int64_t n, int32_t* start, int32_t* end);
int mrx_is_match_batch(const mrx_handle* h, const uint8_t* data, const int64_t* offsets,
                       int64_t n, uint8_t* flag);
int mrx_split_batch(const mrx_handle* h, const uint8_t* data, const int64_t* offsets, int64_t n, int64_t maxsplit,
                    int64_t* piece_prefix, int32_t* pieces, int64_t piece_cap, int64_t* total);
int mrx_findall_batch(const mrx_handle* h, const uint8_t* data, const int64_t* offsets,
                      int64_t n, int64_t* counts_prefix, int32_t* spans,
                      int64_t span_cap, int64_t* total);
int mrx_captures_batch(const mrx_handle* h, const uint8_t* data, const int64_t* offsets,
                       int64_t n, int32_t* spans);
/* mrx_captures_all_dev on host buffers: groups holds match_cap rows of g + 1 pairs (copied out only when all fit) */
int mrx_captures_all_batch(const mrx_handle* h, const uint8_t* data, const int64_t* offsets, int64_t n, int64_t count,
                           int64_t* match_prefix, int32_t* groups, int64_t match_cap, int64_t* total);
/* mrx_set_findall_dev on host buffers: members and spans are copied out only when all hits fit */
int mrx_set_findall_batch(const mrx_set* s, const uint8_t* data, const int64_t* offsets, int64_t n,
                          int64_t* text_prefix, int32_t* members, int32_t* spans, int64_t span_cap, int64_t* total);
/* mrx_set_sub_dev on host buffers: out_data is copied out only when all output fits; nsub (int32[n]) may be NULL */
int mrx_set_sub_batch(const mrx_set* s, const char* const* repls, const size_t* repl_lens, int64_t count,
                      const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* out_offsets, uint8_t* out_data,
                      int64_t out_cap, int32_t* nsub, int64_t* total_bytes);
int mrx_sub_batch(const mrx_handle* h, const char* repl, size_t repl_len, int64_t count,
                  const uint8_t* data, const int64_t* offsets, int64_t n,
                  int64_t* out_offsets, uint8_t* out_data, int64_t out_cap,
                  int64_t* total_bytes);

/* Per-call scratch (counts, event records, block sums) is kept in a grow-only arena per calling
 * thread and stream and reused by the next call on that stream.  mrx_release_scratch() frees the
 * calling thread's arenas (it synchronises their streams first).  Size: findall needs up to one
 * byte of records per text byte (+ 4 KiB per 64 texts); on the stepper kernels with texts of 2 KiB
 * and more, two bytes of span slots per text byte.  The arena settles within two calls of a new
 * batch shape (a call that had to grow it is followed by one that merges its chunks).
 *
 * Batch shape and kernel choice (all automatic, results never depend on it): one lane per text by
 * default; batches of few long texts put a wavefront on each text (stepper plans) or cut the texts
 * into pieces at bytes after which the scan does not depend on its past (streaming plans); ragged
 * CSR batches with a few texts far longer than the rest are handled the same way for findall.
 * CSR entry points read the batch's byte count (and longest text) back once per call; the strided
 * entry points with total == NULL never synchronise. */
void mrx_release_scratch(void);

const char* mrx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MRX_H */
