// The sorted index's judgements (mrx_sorted.hip): where a text falls among sorted entries.  Host and device code, so that
// the searches also run on the CPU against std::lower_bound / std::upper_bound (tools/sorted_check.cpp).
//
// The order is sort's (mrx_sort_bits.hpp): bytewise, unsigned, a proper prefix first.  Every text is read through
// sort_word, so only the aligned 16-byte words that hold a byte of it are loaded, what they hold outside the text is
// masked away, and no word is loaded for an empty text.
//
// One comparison carries everything: sorted_compare_depth gives the sign and the DEPTH, a multiple of 8 such that both
// texts have at least that many bytes and agree on them.  A binary search keeps the depth proven against the entry under
// its lower bound and the one at its upper bound; every entry between the two shares the smaller of them with the probe
// (the entries are sorted), so the next comparison starts there and a long shared prefix is read once, not once a step.
#pragma once
#include <cstdint>

#include "mrx_sort_bits.hpp"

namespace mrx {

// what a search reads of the handle.  keys / valids (nullptr = the aid is off): sort_word(entry, 0) and its valid count
// for every position.  fkey / fvalid (fcount == 0 = off): the keys of positions 0, fstep, 2 fstep, ...
struct SortedView {
  const uint8_t* data;
  const int64_t* offsets;   // [m + 1]
  int64_t m;
  const uint64_t* keys;
  const uint8_t* valids;
  const uint64_t* fkey;
  const uint8_t* fvalid;
  int64_t fstep;
  int fcount;
};

enum { SORTED_AID_KEYS = 1, SORTED_AID_FENCE = 2 };   // mrx_debug_sorted_aids()
constexpr int kSortedFence = 1024;                     // fence posts at most

// positions between two fence posts: the least step with at most kSortedFence posts
MRX_HD int64_t sorted_fence_step(int64_t m) { return m <= kSortedFence ? 1 : (m + kSortedFence - 1) / kSortedFence; }

// < 0, 0, > 0 as text a sorts before, equal to, behind text b, given that both have `from` bytes (a multiple of 8) and
// agree on them.  *depth: the multiple of 8 at which the deciding word begins: both texts have that many bytes and agree
// on them (their common prefix rounded down to 8; for equal texts, the word in which they end).
MRX_HD int sorted_compare_depth(const uint8_t* a, int64_t La, const uint8_t* b, int64_t Lb, int64_t from, int64_t* depth) {
  for (int64_t d = from;; d += 8) {
    int va, vb;
    const uint64_t wa = sort_word(a, La, d, &va), wb = sort_word(b, Lb, d, &vb);
    if (wa != wb || va != vb || va < 8) {
      *depth = d;
      if (wa != wb) return wa < wb ? -1 : 1;
      return va < vb ? -1 : va > vb ? 1 : 0;
    }
  }
}

// the same with entry e cut to the probe's length: 0 when the probe is a prefix of e (PREFIX's upper bound).  The
// full comparison follows from it: where it is 0, e is behind the probe when it is longer, else equal.
MRX_HD int sorted_compare_trunc(const uint8_t* e, int64_t Le, const uint8_t* p, int64_t Lp, int64_t from, int64_t* depth) {
  return sorted_compare_depth(e, Le < Lp ? Le : Lp, p, Lp, from, depth);
}

// the number of bytes on which two texts agree from their first byte on
MRX_HD int64_t sorted_lcp(const uint8_t* a, int64_t La, const uint8_t* b, int64_t Lb) {
  const int64_t lim = La < Lb ? La : Lb;
  for (int64_t d = 0; d < lim; d += 8) {
    int va, vb;
    const uint64_t x = sort_word(a, La, d, &va) ^ sort_word(b, Lb, d, &vb);
    if (x) {
      const int64_t l = d + (__builtin_clzll(x) >> 3);
      return l < lim ? l : lim;
    }
  }
  return lim;
}

MRX_HD const uint8_t* sorted_entry(const SortedView& V, int64_t pos, int64_t* L) {
  const int64_t a = V.offsets[pos];
  *L = V.offsets[pos + 1] - a;
  return V.data + a;
}

// positions [lo, hi) still to decide; dlo / dhi: a depth that the probe shares with every entry of [lo, hi) as long as
// the bound has not moved, then the depth of the comparison that moved it
struct SortedRange {
  int64_t lo, hi, dlo, dhi;
};

enum { SORTED_LOWER = 0, SORTED_UPPER = 1, SORTED_PREFIX_UPPER = 2 };

// The first position of [r.lo, r.hi) whose entry does not go to the left of the answer, r.hi when all do: an entry goes
// left when it is smaller than the probe (LOWER), not greater (UPPER), not greater once cut to the probe's length
// (PREFIX_UPPER).  `up`, for LOWER only and where given, leaves the range of the search that follows for the upper bound:
// from the answer to the lowest position seen that is behind every equal entry (strict_trunc: behind every entry that
// begins with the probe).
MRX_HD int64_t sorted_bisect(const SortedView& V, const uint8_t* p, int64_t L, int kind, SortedRange r, SortedRange* up,
                             bool strict_trunc) {
  if (up) *up = r;
  while (r.lo < r.hi) {
    const int64_t mid = r.lo + ((r.hi - r.lo) >> 1);
    int64_t Le, dm;
    const uint8_t* e = sorted_entry(V, mid, &Le);
    const int ct = sorted_compare_trunc(e, Le, p, L, r.dlo < r.dhi ? r.dlo : r.dhi, &dm);
    const int c = ct ? ct : (Le > L ? 1 : 0);
    const bool left = kind == SORTED_LOWER ? c < 0 : kind == SORTED_UPPER ? c <= 0 : ct <= 0;
    if (left) {
      r.lo = mid + 1;
      r.dlo = dm;
    } else {
      r.hi = mid;
      r.dhi = dm;
      if (up && (strict_trunc ? ct > 0 : c > 0)) {
        up->hi = mid;
        up->dhi = dm;
      }
    }
  }
  if (up) {
    up->lo = r.lo;
    up->dlo = r.dlo;
  }
  return r.lo;
}

// Does the key of the entry at position `at` go to the left of the answer for the probe's key (pw, pv)?  sh
// (PREFIX_UPPER, pv in 1..7): the bits of a word behind the probe's bytes.  The valid count is loaded only where the
// words are equal: most steps of a search are one 8-byte load.
MRX_HD bool sorted_key_left(const uint64_t* keys, const uint8_t* valids, int64_t at, uint64_t pw, int pv, int kind, int sh) {
  const uint64_t k = keys[at];
  if (kind == SORTED_PREFIX_UPPER) return (k >> sh) <= (pw >> sh);
  if (k != pw) return k < pw;
  const int v = (int)valids[at];
  return kind == SORTED_LOWER ? v < pv : v <= pv;
}

// sorted_bisect on the first words alone: the first position of [lo, hi) whose key does not go left.  The fence posts,
// where the view has them, give the window of at most fstep positions that holds it.  up_hi (where given, with up_kind
// the kind of the search that follows for the upper bound): the lowest position seen whose key does not go left for
// that search either, hi when there was none.
MRX_HD int64_t sorted_key_bound(const SortedView& V, uint64_t pw, int pv, int kind, int64_t lo, int64_t hi, int up_kind,
                                int64_t* up_hi) {
  const int sh = 8 * (8 - pv);
  if (up_hi) *up_hi = hi;   // (not the posts' window below: its end may still go left for the search that follows)
  if (V.fcount > 0) {
    int a = 0, b = V.fcount;
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (sorted_key_left(V.fkey, V.fvalid, mid, pw, pv, kind, sh)) a = mid + 1; else b = mid;
    }
    // post a - 1 goes left, post a does not: the answer lies in ((a - 1) fstep, a fstep]
    int64_t flo = a > 0 ? (int64_t)(a - 1) * V.fstep + 1 : 0, fhi = a < V.fcount ? (int64_t)a * V.fstep : V.m;
    if (flo < lo) flo = lo;
    if (fhi > hi) fhi = hi;
    if (flo <= fhi) {   // (else the answer lies outside [lo, hi): the loop below ends at the nearer bound)
      lo = flo;
      hi = fhi;
    }
  }
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (sorted_key_left(V.keys, V.valids, mid, pw, pv, kind, sh)) {
      lo = mid + 1;
    } else {
      hi = mid;
      if (up_hi && !sorted_key_left(V.keys, V.valids, mid, pw, pv, up_kind, sh)) *up_hi = mid;
    }
  }
  return lo;
}

// the positions [*a, *b) whose keys are those of an entry equal to the probe (pv < 8), that begins with the probe (pv <
// 8, up_kind PREFIX_UPPER) or that shares its first 8 bytes (pv == 8): the lower bound, and the upper one from there to
// the lowest position that the lower search saw behind it
MRX_HD void sorted_key_run(const SortedView& V, uint64_t pw, int pv, int up_kind, int64_t* a, int64_t* b) {
  int64_t up_hi;
  *a = sorted_key_bound(V, pw, pv, SORTED_LOWER, 0, V.m, up_kind, &up_hi);
  *b = sorted_key_bound(V, pw, pv, up_kind, *a, up_hi, 0, nullptr);
}

// [*lo, *hi) of mode EQUAL (prefix == false) or PREFIX for the probe p[0, L)
MRX_HD void sorted_range(const SortedView& V, const uint8_t* p, int64_t L, bool prefix, int64_t* lo, int64_t* hi) {
  SortedRange r{0, V.m, 0, 0};
  if (V.keys) {
    int pv;
    const uint64_t pw = sort_word(p, L, 0, &pv);
    if (pv < 8) {   // the probe ends inside its first word: the keys decide
      if (prefix && pv == 0) {
        *lo = 0;
        *hi = V.m;
      } else {
        sorted_key_run(V, pw, pv, prefix ? SORTED_PREFIX_UPPER : SORTED_UPPER, lo, hi);
      }
      return;
    }
    // the run of entries that begin with the probe's first 8 bytes holds both bounds
    sorted_key_run(V, pw, 8, SORTED_UPPER, &r.lo, &r.hi);
    r.dlo = r.dhi = 8;
  }
  SortedRange up;
  *lo = sorted_bisect(V, p, L, SORTED_LOWER, r, &up, prefix);
  *hi = sorted_bisect(V, p, L, prefix ? SORTED_PREFIX_UPPER : SORTED_UPPER, up, nullptr, false);
}

// bisect_left (SORTED_LOWER) or bisect_right (SORTED_UPPER) of p[0, L)
MRX_HD int64_t sorted_bound(const SortedView& V, const uint8_t* p, int64_t L, int kind) {
  SortedRange r{0, V.m, 0, 0};
  if (V.keys) {
    int pv;
    const uint64_t pw = sort_word(p, L, 0, &pv);
    if (pv < 8) return sorted_key_bound(V, pw, pv, kind, 0, V.m, 0, nullptr);
    sorted_key_run(V, pw, 8, SORTED_UPPER, &r.lo, &r.hi);
    r.dlo = r.dhi = 8;
  }
  return sorted_bisect(V, p, L, kind, r, nullptr, false);
}

// Mode LONGEST: *pos = the lowest position of the longest entry that is a prefix of p[0, L), *len its length; -1, -1
// when there is none.  Every entry that is a prefix of p[0, len) is also a prefix of e, the entry in front of
// bisect_right(p[0, len)): e is that entry, or the search goes on with len = lcp(e, p), which is smaller than len.
MRX_HD void sorted_longest(const SortedView& V, const uint8_t* p, int64_t L, int64_t* pos, int64_t* len) {
  int64_t cur = L;
  while (true) {
    const int64_t r = sorted_bound(V, p, cur, SORTED_UPPER);
    if (r == 0) break;
    int64_t Le;
    const uint8_t* e = sorted_entry(V, r - 1, &Le);
    const int64_t l = sorted_lcp(e, Le, p, cur);
    if (l == Le) {
      *pos = sorted_bound(V, p, Le, SORTED_LOWER);
      *len = Le;
      return;
    }
    cur = l;
  }
  *pos = -1;
  *len = -1;
}

// one probe of a search in `mode` (MRX_SORTED_EQUAL 0, MRX_SORTED_PREFIX 1, MRX_SORTED_LONGEST 2)
MRX_HD void sorted_search_one(const SortedView& V, uint32_t mode, const uint8_t* p, int64_t L, int64_t* lo, int64_t* hi) {
  if (mode == 2) sorted_longest(V, p, L, lo, hi);
  else sorted_range(V, p, L, mode == 1, lo, hi);
}

}  // namespace mrx
