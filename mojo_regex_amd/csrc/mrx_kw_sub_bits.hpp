// Keywords, leftmost and sub (include/mrx.h, "keywords: leftmost-longest matches and replacement"): the index logic of the
// two operations.  Host and device code, written like mrx_kw_bits.hpp: what the kernels of mrx_kw_sub.hip run per lane
// is what mrx_debug_kw_host_leftmost / mrx_debug_kw_host_sub and tools/kw_sub_check.cpp run on the CPU, over the same
// pieces (kw_sub_host at the end of this file).
//
// Candidates.  The automaton here is kw_build over the REVERSED entries, walked right to left.  After the step that
// consumes byte q the state's outputs are the reversed entries that are suffixes of reverse(text[q .. start of the walk)),
// that is the entries that BEGIN at q; the first of the output chain is the longest.  A piece [p, pend) walks from
// min(L, pend + Lmax - 1) down to p: an entry that begins in the piece ends at most Lmax - 1 bytes behind it, so the
// walk has seen all of it, and the warm-up never leaves the text.  Each position gives at most one candidate, (q, q +
// depth, entry): the longest entry there, under its lowest index.  The candidates of a text in piece order, each piece's
// written from the back of its slot, are sorted by start.
//
// Selection.  The leftmost-longest matches are the chain: take the first candidate, then the first candidate that
// starts at or behind the end of the one taken, and so on.  Candidate c is a HEAD when every earlier candidate of its
// text ends at or before c.start.  A head is taken whatever happened before it: the chain reaches it with pos <=
// c.start (the candidate taken last is an earlier one, and ends at or before c.start), and no candidate lies between
// the chain's position and c that it would take instead without being taken itself.  From a head on, the chain is that
// of a fresh start.  So the lane of a piece finds the first head in its piece (the running maximum of the ends, seeded
// from reach[] of the ceil((Lmax - 1) / P) pieces in front: only candidates that start within Lmax - 1 bytes in front
// of c can end behind c.start), walks the chain from there and writes the flag of every candidate it passes, until it
// stands in front of a head in a LATER piece -- which that piece's lane starts from.  Every flag is written by exactly
// one lane.  A text without a head behind its first candidate (`aa` in `aaaa...`) is walked end to end by one lane.
//
// Segments.  The output of sub is a list of rows, each a length and a source address: for the kept match g (counted
// over the whole batch) of text i the row 2 g + i is the stretch of the text between the previous kept match and it and
// the row 2 g + i + 1 its replacement; behind a text's last kept match comes its tail row.  An exclusive scan of the
// lengths is the CSR of the rows over the output, and the byte mover is the block gather of extract with a source
// address per row (kw_sub_fill).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "mrx_kw_bits.hpp"

namespace mrx {

// one walk back: bytes [p, s1) of the text at tp from s1 - 1 down to p, candidates reported at q in [p, pend);
// p == s1: nothing to do
struct KwBackJob {
  const uint8_t* tp;
  int32_t p, pend, s1;
};
MRX_HD KwBackJob kw_back_job(const uint8_t* tp, int64_t L, int64_t lp, int64_t P, int32_t lmax) {
  const int64_t p = lp * P;
  if (p >= L) return KwBackJob{tp, 0, 0, 0};
  const int64_t warm = lmax > 0 ? lmax - 1 : 0;
  const int64_t pend = p + P < L ? p + P : L;
  return KwBackJob{tp, (int32_t)p, (int32_t)pend, (int32_t)(pend + warm < L ? pend + warm : L)};
}
MRX_HD KwBackJob kw_no_back_job() { return KwBackJob{nullptr, 0, 0, 0}; }

// The mirror of kw_walk: an aligned 16-byte word of the text a round, from the word of byte s1 - 1 down to the word of
// byte p, the bytes of a word from the highest down.  Only those words are loaded; their bytes outside [p, s1) take the
// step's loads and the result is dropped.  sink.cand(state, q) for every step inside the piece onto a state with outputs.
template <class Tab, class Sink>
MRX_HD void kw_walk_back(const Tab& t, const KwBackJob& job, Sink& sink) {
  if (job.p >= job.s1) return;
  const uintptr_t lo = ((uintptr_t)job.tp + (uintptr_t)job.p) >> 4, hi = ((uintptr_t)job.tp + (uintptr_t)job.s1 - 1) >> 4;
  const int32_t rounds = (int32_t)(hi - lo) + 1;
  uint32_t state = 0;
  for (int32_t r = 0; r < rounds; ++r) {
    const uintptr_t w = (hi - (uintptr_t)r) << 4;
    const g_u64x2 x = *(const g_u64x2*)w;
    const int32_t q0 = (int32_t)((int64_t)w - (int64_t)(uintptr_t)job.tp);
#pragma unroll
    for (int k = 15; k >= 0; --k) {
      const int32_t q = q0 + k;
      const uint32_t byte = (uint32_t)((k < 8 ? x.x : x.y) >> (8 * (k & 7))) & 255u;
      const uint32_t word = t.word(state, byte);   // (a valid address whatever the byte: every byte has a class)
      const bool in = q >= job.p && q < job.s1;
      state = in ? (word & ~kKwFlag) : state;
      if (in && (word & kKwFlag) && q < job.pend) sink.cand(state, q);
    }
  }
}

// the longest entry of a state with outputs
MRX_HD KwMeta kw_longest_out(const KwMeta* meta, uint32_t st) {
  KwMeta m = meta[st];
  if (m.entry < 0) m = meta[(uint32_t)m.out];   // (a flagged state without an entry of its own has a chain behind it)
  return m;
}

// the candidates of a call: start, end and entry of each, and the flag that the selection writes
struct KwCands {
  int32_t* start;
  int32_t* end;
  int32_t* entry;
  uint8_t* sel;
};

struct KwCandCount {
  const KwMeta* meta;
  int64_t cnt;
  int32_t reach;   // the largest end of a candidate that starts in the piece (0: none)
  MRX_HD void cand(uint32_t st, int32_t q) {
    const int32_t e = q + kw_longest_out(meta, st).depth;
    ++cnt;
    reach = e > reach ? e : reach;
  }
};
struct KwCandEmit {
  const KwMeta* meta;
  KwCands c;
  int64_t at;   // the piece's last slot: the walk meets its candidates in descending start order
  MRX_HD void cand(uint32_t st, int32_t q) {
    const KwMeta m = kw_longest_out(meta, st);
    c.start[at] = q;
    c.end[at] = q + m.depth;
    c.entry[at] = m.entry;
    --at;
  }
};

// The lane of `piece`, the lp-th of its text: scan[] is the exclusive scan of the pieces' candidate counts, tend the end
// of the text's candidates, back = ceil((Lmax - 1) / P).
MRX_HD void kw_sub_select(const KwCands& c, const int64_t* scan, const int32_t* reach, int64_t piece, int64_t lp, int64_t tend,
                          int64_t back) {
  const int64_t a = scan[piece], b = scan[piece + 1];
  if (a == b) return;
  int32_t mx = 0;   // the largest end of the text's candidates in front of the one looked at, as far as it can matter
  for (int64_t k = 1; k <= back && k <= lp; ++k) {
    const int32_t r = reach[piece - k];
    mx = r > mx ? r : mx;
  }
  int64_t h = a;
  for (; h < b; ++h) {
    if (mx <= c.start[h]) break;
    const int32_t e = c.end[h];
    mx = e > mx ? e : mx;
  }
  if (h == b) return;   // no head here: a chain from an earlier piece passes through
  int32_t pos = c.end[h];
  mx = pos;             // (every candidate in front of a head ends at or before its start)
  c.sel[h] = 1;
  for (int64_t q = h + 1; q < tend; ++q) {
    const int32_t s = c.start[q], e = c.end[q];
    if (q >= b && mx <= s) break;   // a head in a later piece: that piece's lane goes on from here
    const bool take = s >= pos;
    c.sel[q] = take ? 1 : 0;
    pos = take ? e : pos;
    mx = e > mx ? e : mx;
  }
}

MRX_HD int64_t kw_sub_selected(const uint8_t* sel, int64_t a, int64_t b) {
  int64_t k = 0;
  for (int64_t q = a; q < b; ++q) k += sel[q];
  return k;
}

// the matches of a text that are kept: all the selected ones, or the first `count` of them
MRX_HD int64_t kw_sub_kept(int64_t selected, int64_t count) { return count > 0 && selected > count ? count : selected; }

// the rows of the output
struct KwSegs {
  int64_t* len;          // [2 K + n] (the scan's input)
  const uint8_t** src;   // [2 K + n]
};
// the replacements: r == 1 (one row for every entry) or r == m rows
struct KwRepl {
  const uint8_t* data;
  const int64_t* off;
  int64_t r;
  MRX_HD int64_t row(int32_t entry) const { return r == 1 ? 0 : (int64_t)entry; }
};
// where leftmost leaves its matches
struct KwSpansOut {
  int32_t* entries;
  int32_t* spans;   // 8-byte aligned
  int64_t cap;
};

// The lane of a piece behind the selection, for text i (tp, L) whose candidates begin at tfirst: sel_rank is the rank in
// the text of the piece's first selected candidate, kb[i] the number of kept matches in the texts before i, kept the
// number kept in this text.  SUB: the rows of the piece's kept matches, and the text's tail row behind its last one.
// Else: the kept matches at their ranks, clamped at the capacity.
template <bool SUB>
MRX_HD void kw_sub_rows(const KwCands& c, int64_t a, int64_t b, int64_t tfirst, int64_t sel_rank, int64_t kb, int64_t kept,
                        int64_t i, const uint8_t* tp, int32_t L, const KwRepl& R, const KwSegs& S, const KwSpansOut& O) {
  int64_t r = sel_rank;
  int32_t prev = -1;
  for (int64_t q = a; q < b && r < kept; ++q) {
    if (!c.sel[q]) continue;
    const int32_t s = c.start[q], e = c.end[q];
    const int64_t g = kb + r;
    if (SUB) {
      if (prev < 0) {   // the match taken before this one: everything between the two overlaps it, Lmax steps at most
        int64_t j = q - 1;
        while (j >= tfirst && !c.sel[j]) --j;
        prev = j >= tfirst ? c.end[j] : 0;
      }
      const int64_t row = 2 * g + i, rr = R.row(c.entry[q]);
      S.len[row] = s - prev;
      S.src[row] = tp + prev;
      S.len[row + 1] = R.off[rr + 1] - R.off[rr];
      S.src[row + 1] = R.data + R.off[rr];
      if (r == kept - 1) {
        S.len[row + 2] = L - e;
        S.src[row + 2] = tp + e;
      }
      prev = e;
    } else if (g < O.cap) {
      O.entries[g] = c.entry[q];
      ((uint64_t*)O.spans)[g] = (uint64_t)(uint32_t)s | ((uint64_t)(uint32_t)e << 32);
    }
    ++r;
  }
}

// the block of the byte mover (gather_blocks): bytes [pos, endp) of the output, byte p at block position p - p0; row r
// holds byte pos, and hi is the last row that the block can reach
MRX_HD g_u128 kw_sub_fill(const int64_t* off, const uint8_t* const* src, int64_t r, int64_t hi, int64_t p0, int64_t pos,
                          int64_t endp) {
  g_u128 acc = 0;
  while (true) {
    const int64_t s = off[r], e = off[r + 1];
    const int take = (int)((e < endp ? e : endp) - pos);
    acc = gather_place(acc, src[r] + (pos - s), take, (int)(pos - p0));
    pos += take;
    if (pos >= endp) break;
    r = gather_gallop(off, r + 1, hi + 1, pos);   // the next row with a byte: empty ones are stepped over
  }
  return acc;
}

// ---- host only: the whole route on host buffers, step by step as the launches of mrx_kw_sub.hip ---------------------
struct KwSubHostResult {
  std::vector<int64_t> kb;         // [n + 1]: the kept matches in front of every text (leftmost's text prefix)
  std::vector<int32_t> entries;    // leftmost (sub == false): [K], clamped at span_cap
  std::vector<uint64_t> spans;
  std::vector<int64_t> out_off;    // sub: [n + 1]
  int64_t bytes = 0, longest = 0;
};
// A: the automaton of the reversed entries.  Text i is data[off[i], off[i + 1]); the aligned 16-byte words around every
// text and every replacement must be readable.  sub: the output's bytes go to out when they fit out_cap (and nothing is
// written otherwise); else the kept matches go to res->entries / spans, those below span_cap.
inline void kw_sub_host(const KwAutomaton& A, int64_t P, int64_t count, const uint8_t* data, const int64_t* off, int64_t n,
                        bool sub, const KwRepl& R, uint8_t* out, int64_t out_cap, int64_t span_cap, KwSubHostResult* res) {
  const KwHostTab tab{A.table.data(), A.cls.data(), A.ncls};
  std::vector<int64_t> first((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) first[(size_t)i + 1] = first[(size_t)i] + (off[i + 1] - off[i] + P - 1) / P;
  const int64_t np = first[(size_t)n];
  const KwPieces pc{P, 0, first.data(), np};
  std::vector<int64_t> scan((size_t)np + 1, 0), sscan((size_t)np + 1, 0);
  std::vector<int32_t> reach((size_t)np + 1, 0);
  auto job_of = [&](int64_t piece, int64_t* i, int64_t* lp) {
    if (!kw_piece_text(pc, n, piece, i, lp)) return kw_no_back_job();
    return kw_back_job(data + off[*i], off[*i + 1] - off[*i], *lp, P, A.lmax);
  };
  int64_t i = 0, lp = 0;
  for (int64_t piece = 0; piece < np; ++piece) {
    KwCandCount cs{A.meta.data(), 0, 0};
    kw_walk_back(tab, job_of(piece, &i, &lp), cs);
    scan[(size_t)piece + 1] = scan[(size_t)piece] + cs.cnt;
    reach[(size_t)piece] = cs.reach;
  }
  const int64_t C = scan[(size_t)np];
  std::vector<int32_t> cs_((size_t)C + 1), ce_((size_t)C + 1), cj_((size_t)C + 1);
  std::vector<uint8_t> sel((size_t)C + 1, 0xEE);   // (every flag is written by the selection)
  const KwCands c{cs_.data(), ce_.data(), cj_.data(), sel.data()};
  for (int64_t piece = 0; piece < np; ++piece) {
    if (scan[(size_t)piece + 1] == scan[(size_t)piece]) continue;
    KwCandEmit es{A.meta.data(), c, scan[(size_t)piece + 1] - 1};
    kw_walk_back(tab, job_of(piece, &i, &lp), es);
  }
  const int64_t warm = A.lmax > 0 ? A.lmax - 1 : 0, back = (warm + P - 1) / P;
  for (int64_t piece = 0; piece < np; ++piece) {
    if (!kw_piece_text(pc, n, piece, &i, &lp)) continue;
    kw_sub_select(c, scan.data(), reach.data(), piece, lp, scan[(size_t)first[(size_t)i + 1]], back);
  }
  for (int64_t piece = 0; piece < np; ++piece)
    sscan[(size_t)piece + 1] = sscan[(size_t)piece] + kw_sub_selected(sel.data(), scan[(size_t)piece], scan[(size_t)piece + 1]);
  res->kb.assign((size_t)n + 1, 0);
  for (int64_t t = 0; t < n; ++t)
    res->kb[(size_t)t + 1] = res->kb[(size_t)t] + kw_sub_kept(sscan[(size_t)first[(size_t)t + 1]] - sscan[(size_t)first[(size_t)t]], count);
  const int64_t K = res->kb[(size_t)n], rows = 2 * K + n;
  std::vector<int64_t> slen((size_t)rows + 1, 0), soff((size_t)rows + 1, 0);
  std::vector<const uint8_t*> ssrc((size_t)rows + 1, nullptr);
  const KwSegs S{slen.data(), ssrc.data()};
  const int64_t held = K < span_cap ? K : span_cap;
  res->entries.assign((size_t)held, 0);
  res->spans.assign((size_t)held, 0);
  const KwSpansOut O{res->entries.data(), (int32_t*)res->spans.data(), held};
  for (int64_t t = 0; t < n && sub; ++t)
    if (res->kb[(size_t)t + 1] == res->kb[(size_t)t]) {   // a text without a kept match is its tail row
      slen[(size_t)(2 * res->kb[(size_t)t] + t)] = off[t + 1] - off[t];
      ssrc[(size_t)(2 * res->kb[(size_t)t] + t)] = data + off[t];
    }
  for (int64_t piece = 0; piece < np; ++piece) {
    if (!kw_piece_text(pc, n, piece, &i, &lp)) continue;
    const int64_t kb = res->kb[(size_t)i], kept = res->kb[(size_t)i + 1] - kb;
    const int64_t rank = sscan[(size_t)piece] - sscan[(size_t)first[(size_t)i]];
    if (sub)
      kw_sub_rows<true>(c, scan[(size_t)piece], scan[(size_t)piece + 1], scan[(size_t)first[(size_t)i]], rank, kb, kept, i,
                        data + off[i], (int32_t)(off[i + 1] - off[i]), R, S, O);
    else
      kw_sub_rows<false>(c, scan[(size_t)piece], scan[(size_t)piece + 1], scan[(size_t)first[(size_t)i]], rank, kb, kept, i,
                         data + off[i], (int32_t)(off[i + 1] - off[i]), R, S, O);
  }
  if (!sub) return;
  for (int64_t r = 0; r < rows; ++r) soff[(size_t)r + 1] = soff[(size_t)r] + slen[(size_t)r];
  res->out_off.assign((size_t)n + 1, 0);
  res->longest = 0;
  for (int64_t t = 0; t <= n; ++t) {
    res->out_off[(size_t)t] = soff[(size_t)(2 * res->kb[(size_t)t] + t)];
    if (t > 0) res->longest = std::max(res->longest, res->out_off[(size_t)t] - res->out_off[(size_t)t - 1]);
  }
  const int64_t bytes = res->bytes = soff[(size_t)rows];
  if (bytes <= 0 || bytes > out_cap) return;
  // the blocks of gather_blocks, one after the other
  const uintptr_t ob = (uintptr_t)out, a0 = ob & ~(uintptr_t)15;
  const int64_t head = (int64_t)(ob - a0), nblk = (head + bytes + 15) >> 4;
  int64_t cur = 0;
  for (int64_t b = 0; b < nblk; ++b) {
    const int64_t p0 = b * 16 - head, pos = p0 > 0 ? p0 : 0, endp = p0 + 16 < bytes ? p0 + 16 : bytes;
    const int64_t hi = gather_gallop(soff.data(), cur, rows, endp - 1);
    cur = gather_last_le(soff.data(), cur, hi + 1, pos);
    const g_u128 acc = kw_sub_fill(soff.data(), ssrc.data(), cur, hi, p0, pos, endp);
    for (int q = (int)(pos - p0); q < (int)(endp - p0); ++q) out[b * 16 - head + q] = (uint8_t)(acc >> (8 * q));
  }
}

// the automaton of the reversed entries: entry j is data[off[j], off[j + 1]) (already folded, or to be folded by `flags`)
inline int kw_build_reversed(const uint8_t* data, const int64_t* off, int64_t m, uint32_t flags, KwAutomaton* A, std::string* err) {
  const int64_t base = m > 0 ? off[0] : 0, total = m > 0 ? off[m] - off[0] : 0;
  std::vector<uint8_t> rev((size_t)total);
  std::vector<int64_t> roff((size_t)m + 1, 0);
  for (int64_t j = 0; j < m; ++j) {
    if (off[j + 1] < off[j]) return *err = "offsets must not decrease", MRX_E_ARGUMENT;
    roff[(size_t)j + 1] = off[j + 1] - base;
    std::reverse_copy(data + off[j], data + off[j + 1], rev.begin() + (off[j] - base));
  }
  return kw_build(rev.data(), roff.data(), m, flags, A, err);
}

}  // namespace mrx
