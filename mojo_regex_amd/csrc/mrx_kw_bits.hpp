// Keywords (include/mrx.h, "keywords"): the Aho-Corasick automaton of a keyword set and the walk of one piece of a text
// through it.  Host and device code: the build runs on the host only; the walk is what k_kw_count and k_kw_emit run
// (mrx_keywords.hip) and what mrx_debug_kw_host_findall and tools/kw_check.cpp run on the CPU, over the same pieces.
//
// The automaton is a trie of the (folded) entries with failure links, completed to a dense table over byte classes:
//   cls[256]                    byte -> class; every byte that occurs in no entry is class 0, whose column goes to the root
//   table[states][ncls] uint32  the low 31 bits are the target state, bit 31 says that the target's output chain is not
//                               empty: the per-byte path tests that one bit
//   meta[states]                entry: the lowest index of an entry that ends exactly here, or -1; depth: that entry's
//                               length (the state's depth); out: the nearest proper-suffix state with an entry, or 0;
//                               nout: the length of the output chain from here, this state's own entry included
// States are numbered shallowest first, so the rows that a walk over text without hits lives in come first (the tier of
// the table that the kernels keep in LDS is a prefix).  The output chain strictly decreases in depth: at one end
// position the longest entry comes first, and the chain is at most Lmax long.
//
// Pieces.  A text is cut into pieces of P bytes.  The piece [p, p + P) walks from the root, beginning at
// max(0, p - (Lmax - 1)), and reports exactly the hits whose last byte lies in the piece.  The state reached from a root
// start at s has as outputs the entries that are suffixes of text[s .. q); a hit that ends in the piece is at most Lmax
// long, so it begins at or behind the warm-up's start and the piece sees it.  Pieces are independent of each other, the
// warm-up never leaves the text, and the hits of a text in piece order are in (end, start) order.
//
// Reading.  A walk loads the aligned 16-byte words that hold a byte of [start, end) of its job and nothing else; the
// bytes of those words outside the job take the step's loads (of valid addresses: every byte has a class) and their
// result is dropped, so they never reach a state or a hit.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/mrx.h"
#include "mrx_gather_bits.hpp"

namespace mrx {

constexpr uint32_t kKwFlag = 0x80000000u;
constexpr int64_t kKwTableLimit = (int64_t)1 << 30;   // bytes of the dense table above which the build refuses

struct KwMeta {
  int32_t entry, depth, out, nout;
};

// one walk: bytes [s0, pend) of the text at tp, hits reported when they end in (p, pend]; s0 == pend: nothing to do
struct KwJob {
  const uint8_t* tp;
  int32_t s0, p, pend;
};

// piece lp (P bytes each) of a text of L bytes
MRX_HD KwJob kw_job(const uint8_t* tp, int64_t L, int64_t lp, int64_t P, int32_t lmax) {
  const int64_t p = lp * P;
  if (p >= L) return KwJob{tp, 0, 0, 0};
  const int64_t warm = lmax > 0 ? lmax - 1 : 0;
  const int64_t pend = p + P < L ? p + P : L;
  return KwJob{tp, (int32_t)(p > warm ? p - warm : 0), (int32_t)p, (int32_t)pend};
}
MRX_HD KwJob kw_no_job() { return KwJob{nullptr, 0, 0, 0}; }

// The pieces of a call, numbered text-major.  Fixed pitch: every text has per_text of them, so piece -> text is a
// division.  CSR: first[n + 1] is the first piece of every text and piece -> text a bisection of it; npieces is then an
// upper bound, and the pieces beyond the last text's do nothing.
struct KwPieces {
  int64_t P;
  int64_t per_text;       // fixed pitch: pieces of every text
  const int64_t* first;   // CSR: [n + 1], the first piece of every text
  int64_t npieces;        // to walk (CSR: an upper bound)
};
// the text of a piece and the piece's number inside it; false: the piece lies behind the last text's
MRX_HD bool kw_piece_text(const KwPieces& pc, int64_t n, int64_t piece, int64_t* i, int64_t* lp) {
  if (piece >= pc.npieces) return false;
  if (pc.first) {
    if (piece >= pc.first[n]) return false;
    *i = gather_last_le(pc.first, 0, n, piece);
    *lp = piece - pc.first[*i];
  } else {
    *i = piece / pc.per_text;
    *lp = piece - *i * pc.per_text;
  }
  return true;
}

// The piece size without a pin (mrx_debug_kw_piece): the warm-up, Lmax - 1 bytes, is at most an eighth of the piece,
// and a piece has 1024 bytes at least (measured: 8 % faster than 256 on 1 KiB texts and on texts of 16 MiB alike,
// profiles/keywords.md) -- unless the batch then has fewer than 2^18 pieces, too few to fill the device: the piece is
// halved down to twice the warm-up (64 bytes at least) until it has.  A multiple of 16.
MRX_HD int64_t kw_piece_rule(int32_t lmax, int64_t total_bytes) {
  const int64_t warm = lmax > 0 ? lmax - 1 : 0;
  int64_t P = (8 * warm + 15) / 16 * 16;
  if (P < 1024) P = 1024;
  int64_t least = (2 * warm + 15) / 16 * 16;
  if (least < 64) least = 64;
  while (P / 2 >= least && total_bytes / P < ((int64_t)1 << 18)) P = (P / 2 + 15) / 16 * 16;
  return P;
}

// One walk through `t` (word(state, byte) -> the transition word), an aligned 16-byte word of the text a round.
// sink.hit(state, end) is called for every step that ends inside the piece on a state with outputs.
template <class Tab, class Sink>
MRX_HD void kw_walk(const Tab& t, const KwJob& job, Sink& sink) {
  if (job.s0 >= job.pend) return;
  const uintptr_t a = (uintptr_t)job.tp + (uintptr_t)job.s0, w = a & ~(uintptr_t)15;
  const int32_t rounds = (int32_t)((((uintptr_t)job.tp + (uintptr_t)job.pend - 1) >> 4) - (a >> 4)) + 1;
  uint32_t state = 0;
  for (int32_t r = 0; r < rounds; ++r) {
    const g_u64x2 x = *(const g_u64x2*)(w + 16 * (uintptr_t)r);
    // the text position of the word's first byte (down to -15 for a text's first word)
    const int32_t q0 = (int32_t)((int64_t)(w + 16 * (uintptr_t)r) - (int64_t)(uintptr_t)job.tp);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int32_t q = q0 + k;
      const uint32_t byte = (uint32_t)((k < 8 ? x.x : x.y) >> (8 * (k & 7))) & 255u;
      const uint32_t word = t.word(state, byte);   // (a valid address whatever the byte: every byte has a class)
      const bool in = q >= job.s0 && q < job.pend;
      state = in ? (word & ~kKwFlag) : state;
      if (in && (word & kKwFlag) && q >= job.p) sink.hit(state, q + 1);
    }
  }
}

// the sinks of the two passes
struct KwCountSink {
  const KwMeta* meta;
  int64_t cnt;
  MRX_HD void hit(uint32_t st, int32_t) { cnt += meta[st].nout; }
};
struct KwEmitSink {
  const KwMeta* meta;
  int32_t* entries;
  int32_t* spans;   // 8-byte aligned
  int64_t cap;
  int64_t pos;
  MRX_HD void hit(uint32_t st, int32_t e) {
    KwMeta m = meta[st];
    if (m.entry < 0) {   // (a flagged state without an entry of its own has a chain behind it)
      st = (uint32_t)m.out;
      m = meta[st];
    }
    while (st != 0) {
      if (pos < cap) {
        entries[pos] = m.entry;
        ((uint64_t*)spans)[pos] = (uint64_t)(uint32_t)(e - m.depth) | ((uint64_t)(uint32_t)e << 32);
      }
      ++pos;
      st = (uint32_t)m.out;
      if (st != 0) m = meta[st];
    }
  }
};

// ---- host only: the build -------------------------------------------------------------------------------------------
struct KwAutomaton {
  int64_t m = 0, distinct = 0;
  int32_t states = 1, ncls = 1, lmax = 0;
  uint32_t flags = 0;
  std::vector<uint32_t> table;   // [states * ncls]
  std::vector<uint8_t> cls;      // [256]
  std::vector<KwMeta> meta;      // [states]
  int64_t table_bytes() const { return (int64_t)states * ncls * 4; }
};
struct KwHostTab {
  const uint32_t* table;
  const uint8_t* cls;
  int32_t ncls;
  uint32_t word(uint32_t st, uint32_t byte) const { return table[(size_t)st * ncls + cls[byte]]; }
};

// MRX_OK, or MRX_E_ARGUMENT / MRX_E_UNSUPPORTED with the message in *err; *A is complete only on MRX_OK.  Entry j is
// data[off[j], off[j + 1]); m >= 0, off != nullptr, and data != nullptr where an entry has bytes are the caller's checks.
inline int kw_build(const uint8_t* data, const int64_t* off, int64_t m, uint32_t flags, KwAutomaton* A, std::string* err) {
  const bool fold = (flags & MRX_KW_IGNORE_CASE) != 0;
  for (int64_t j = 0; j < m; ++j) {
    if (off[j + 1] < off[j]) return *err = "offsets must not decrease", MRX_E_ARGUMENT;
    if (off[j + 1] == off[j]) return *err = "entry " + std::to_string(j) + " is empty: it would occur everywhere", MRX_E_ARGUMENT;
  }
  const int64_t base = m > 0 ? off[0] : 0, total = m > 0 ? off[m] - off[0] : 0;
  std::vector<uint8_t> buf((size_t)total);
  bool used[256] = {};
  for (int64_t k = 0; k < total; ++k) {
    uint8_t c = data[base + k];
    if (fold && c >= 'A' && c <= 'Z') c |= 0x20;
    buf[(size_t)k] = c;
    used[c] = true;
  }
  A->m = m;
  A->flags = flags;
  A->cls.assign(256, 0);
  int ncls = 1;
  for (int c = 0; c < 256; ++c) ncls += used[c];
  if (ncls > 256) {   // every byte value occurs: nothing is left for class 0, and the classes are the bytes
    ncls = 256;
    for (int c = 0; c < 256; ++c) A->cls[c] = (uint8_t)c;
  } else {
    int next = 1;
    for (int c = 0; c < 256; ++c)
      if (used[c]) A->cls[c] = (uint8_t)next++;
  }
  if (fold)
    for (int c = 'A'; c <= 'Z'; ++c) A->cls[c] = A->cls[c | 0x20];
  A->ncls = ncls;
  auto ptr = [&](int64_t j) { return buf.data() + (off[j] - base); };
  auto len = [&](int64_t j) { return off[j + 1] - off[j]; };
  std::vector<int32_t> ord((size_t)m);
  std::iota(ord.begin(), ord.end(), 0);
  std::sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) {
    const int64_t la = len(a), lb = len(b);
    const int c = memcmp(ptr(a), ptr(b), (size_t)std::min(la, lb));
    if (c != 0) return c < 0;
    if (la != lb) return la < lb;
    return a < b;
  });
  auto lcp = [&](int64_t a, int64_t b) {
    const int64_t lim = std::min(len(a), len(b));
    int64_t l = 0;
    while (l < lim && ptr(a)[l] == ptr(b)[l]) ++l;
    return l;
  };
  // the states of the trie, counted before anything of their size is allocated
  int64_t states = 1, distinct = 0, lmax = 0;
  std::vector<int32_t> uniq;   // the different entries in sorted order, each by its lowest index
  for (int64_t k = 0; k < m; ++k) {
    const int32_t j = ord[(size_t)k];
    int64_t l = 0;
    if (!uniq.empty()) {
      l = lcp(uniq.back(), j);
      if (l == len(j) && l == len(uniq.back())) continue;   // equal to the one before: that one has the lower index
    }
    states += len(j) - l;
    lmax = std::max(lmax, len(j));
    uniq.push_back(j);
    ++distinct;
  }
  A->distinct = distinct;
  if (states * ncls * 4 > kKwTableLimit || lmax > 0x7fffffff)
    return *err = "keywords: the table of " + std::to_string(states) + " states x " + std::to_string(ncls) +
                  " classes is above 1 GiB",
           MRX_E_UNSUPPORTED;
  A->states = (int32_t)states;
  A->lmax = (int32_t)lmax;
  // created along the sorted entries (depth first), then renumbered by depth
  const size_t S = (size_t)states;
  std::vector<int32_t> parent(S, 0), depth(S, 0), entry0(S, -1), path(1, 0);
  std::vector<uint16_t> pcls(S, 0);
  int32_t made = 1;
  for (size_t k = 0; k < uniq.size(); ++k) {
    const int32_t j = uniq[k];
    const int64_t l = k ? lcp(uniq[k - 1], j) : 0;
    path.resize((size_t)l + 1);
    for (int64_t d = l; d < len(j); ++d) {
      parent[(size_t)made] = path.back();
      pcls[(size_t)made] = A->cls[ptr(j)[d]];
      depth[(size_t)made] = (int32_t)d + 1;
      path.push_back(made++);
    }
    entry0[(size_t)path.back()] = j;
  }
  std::vector<int32_t> first_at((size_t)lmax + 2, 0), newid(S, 0);
  for (size_t s = 0; s < S; ++s) ++first_at[(size_t)depth[s] + 1];
  for (size_t d = 1; d < first_at.size(); ++d) first_at[d] += first_at[d - 1];
  for (size_t s = 0; s < S; ++s) newid[s] = first_at[(size_t)depth[s]]++;
  constexpr uint32_t kNone = 0xffffffffu;
  A->table.assign(S * (size_t)ncls, kNone);
  A->meta.assign(S, KwMeta{-1, 0, 0, 0});
  for (size_t s = 0; s < S; ++s) {
    const size_t id = (size_t)newid[s];
    A->meta[id].entry = entry0[s];
    A->meta[id].depth = depth[s];
    if (s) A->table[(size_t)newid[(size_t)parent[s]] * ncls + pcls[s]] = (uint32_t)id;
  }
  std::vector<int32_t> fail(S, 0);
  for (size_t s = 0; s < S; ++s) {   // shallowest first: the row of fail[s] is complete, and fail[s] was set by s's parent
    uint32_t* row = &A->table[s * (size_t)ncls];
    const uint32_t* frow = &A->table[(size_t)fail[s] * (size_t)ncls];
    for (int c = 0; c < ncls; ++c) {
      if (row[c] != kNone) fail[row[c]] = s ? (int32_t)frow[c] : 0;
      else row[c] = s ? frow[c] : 0;
    }
    if (s) {
      const KwMeta& f = A->meta[(size_t)fail[s]];
      KwMeta& me = A->meta[s];
      me.out = f.entry >= 0 ? fail[s] : f.out;
      me.nout = (me.entry >= 0) + A->meta[(size_t)me.out].nout;
    }
  }
  for (uint32_t& cell : A->table)
    if (A->meta[cell].nout > 0) cell |= kKwFlag;
  return MRX_OK;
}

// findall on host buffers, piece by piece as the kernels take them: a counting walk, then an emitting walk at the place
// that the counts give.  Text i is data[off[i], off[i + 1]); the aligned 16-byte words around every text must be
// readable.  Returns the number of hits; those below cap are written (entries[q], spans[2 q], spans[2 q + 1]);
// prefix[n + 1].
inline int64_t kw_host_findall(const KwAutomaton& A, int64_t P, const uint8_t* data, const int64_t* off, int64_t n,
                               int64_t* prefix, int32_t* entries, int32_t* spans, int64_t cap) {
  const KwHostTab tab{A.table.data(), A.cls.data(), A.ncls};
  int64_t total = 0;
  std::vector<int32_t> ents;
  std::vector<uint64_t> sp;
  for (int64_t i = 0; i < n; ++i) {
    prefix[i] = total;
    const int64_t L = off[i + 1] - off[i], pieces = (L + P - 1) / P;
    for (int64_t lp = 0; lp < pieces; ++lp) {
      const KwJob job = kw_job(data + off[i], L, lp, P, A.lmax);
      KwCountSink cs{A.meta.data(), 0};
      kw_walk(tab, job, cs);
      ents.assign((size_t)cs.cnt + 1, 0);
      sp.assign((size_t)cs.cnt + 1, 0);
      KwEmitSink es{A.meta.data(), ents.data(), (int32_t*)sp.data(), cs.cnt, 0};
      kw_walk(tab, job, es);
      for (int64_t q = 0; q < cs.cnt; ++q, ++total) {
        if (total >= cap) continue;
        entries[total] = ents[(size_t)q];
        spans[2 * total] = (int32_t)(uint32_t)sp[(size_t)q];
        spans[2 * total + 1] = (int32_t)(uint32_t)(sp[(size_t)q] >> 32);
      }
    }
  }
  prefix[n] = total;
  return total;
}

}  // namespace mrx
