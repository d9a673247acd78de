// Fields (include/mrx.h, "fields"): the delimiter-separated columns of a text as (start, end) pairs.  Host and device
// code: the mask arithmetic of one aligned 16-byte word, the k-th set bit and the selection of a row's pairs from a
// lane's word are what k_fields runs per lane (mrx_fields.hip), and what mrx_debug_fields_host and
// tools/fields_check.cpp run on the CPU, over the same groups and rounds.
//
// Events.  A text is read as the aligned 16-byte words that hold its bytes; bit k of word w is text position
// 16 w - head + k (head: the text's first byte within its word), and bits outside [0, L) are masked before anything
// looks at them.  A word becomes two 16-bit masks:
//   delimiter mode   a = b = the delimiters.  Field q begins one behind delimiter q - 1 (field 0 at 0) and ends at
//                    delimiter q, or at L when there is none; nf = delimiters + 1
//   whitespace mode  a = the field starts (a byte that is no whitespace behind one that is, or behind the text's front),
//                    b = the field ends (a byte that is whitespace or behind the text, behind one that is not): one carry
//                    bit, the word in front's last byte.  Field q begins at start q and ends at end q, or at L when the
//                    text's last byte belongs to it; nf = starts
// So a pair is two ranks in two sequences of set bits, and a missing end is L.  A group of G lanes takes G words a
// round, ranks them with a prefix sum of popcounts, and the lane whose word holds a wanted rank writes the position.
// Under MRX_FIELDS_REST the largest column has no end to find: it stays L.
// Quoted fields (include/mrx.h, "quoted fields") change the masks and nothing behind them: a delimiter between quotes is
// no event, a whitespace byte between quotes counts as a byte that is none, and a finished pair loses its outer quotes.
#pragma once
#include <cstdint>

#include "../../include/mrx.h"
#include "mrx_gather_bits.hpp"
#include "mrx_lines_bits.hpp"

namespace mrx {

constexpr uint32_t kFieldsFlags = MRX_FIELDS_WHITESPACE | MRX_FIELDS_REST;
// G without a pin and without a known mean length (mrx_debug_fields_group)
constexpr int kFieldsDefaultGroup = 2;

// what a call asks for, by value to the kernel
struct FieldsPlan {
  int32_t f;
  uint32_t flags;
  uint32_t delim;
  int32_t cmax;      // MRX_FIELDS_REST: the largest column, else 0
  int32_t any_neg;   // some column is negative: a second walk, once nf is known
  int32_t stop;      // the walk may end once every positive column has ended (REST, or no nf and no negative column)
  int64_t k_a, k_b;  // the largest rank that a positive column asks of the a- and of the b-events (-1: none)
  int32_t cols[MRX_FIELDS_MAX_COLUMNS];
};

MRX_HD bool fields_ws_mode(const FieldsPlan& P) { return (P.flags & MRX_FIELDS_WHITESPACE) != 0; }
// the rank of field q's start among the a-events (delimiter mode: delimiter q - 1, and 1 is added to its position)
MRX_HD int64_t fields_rank_a(const FieldsPlan& P, int64_t q) { return fields_ws_mode(P) ? q : q - 1; }
// does pair j end at an event (not under REST when it is the largest column: it runs to L)
MRX_HD bool fields_has_end(const FieldsPlan& P, int32_t c) { return !((P.flags & MRX_FIELDS_REST) && c == P.cmax); }

// MRX_OK-style: fills the plan from the caller's columns; returns a message for MRX_E_ARGUMENT, or nullptr
inline const char* fields_plan(uint32_t flags, uint8_t delim, const int32_t* columns, int32_t f, bool want_nf, FieldsPlan* P) {
  if (flags & ~kFieldsFlags) return "unknown flag";
  if (f < 1 || f > MRX_FIELDS_MAX_COLUMNS) return "f must be in [1, MRX_FIELDS_MAX_COLUMNS]";
  if (!columns) return "null argument";
  P->f = f;
  P->flags = flags;
  P->delim = delim;
  P->cmax = 0;
  P->any_neg = 0;
  for (int j = 0; j < MRX_FIELDS_MAX_COLUMNS; ++j) P->cols[j] = j < f ? columns[j] : 1;
  for (int j = 0; j < f; ++j) {
    if (columns[j] == 0) return "a column must not be 0 (columns count from 1, or from -1 at the end)";
    if (columns[j] < 0) P->any_neg = 1;
    if (columns[j] > P->cmax) P->cmax = columns[j];
  }
  if (!(flags & MRX_FIELDS_REST)) P->cmax = 0;
  else if (P->any_neg) return "MRX_FIELDS_REST needs positive columns";
  P->k_a = P->k_b = -1;
  for (int j = 0; j < f; ++j) {
    const int64_t q = (int64_t)columns[j] - 1;
    if (columns[j] < 0) continue;
    if (fields_rank_a(*P, q) > P->k_a) P->k_a = fields_rank_a(*P, q);
    if (fields_has_end(*P, columns[j]) && q > P->k_b) P->k_b = q;
  }
  P->stop = (flags & MRX_FIELDS_REST) || (!want_nf && !P->any_neg) ? 1 : 0;
  return nullptr;
}

// G by the rule, from the sweep of profiles/fields.md (mean lengths 64, 99, 544 and 1024): a text's fixed cost -- the
// row's staging, the prefix sum's shuffles, the loop over the columns once per round -- is paid per group, so few lanes
// per text win as long as there are texts enough to fill the device, and G = 64 loses by a factor of ten on 100-byte
// lines.  The last step is a guess and says so: no input with a mean of 16 KiB or more has been measured; there the
// texts are few and the lanes of a group are all the parallelism there is.
inline int fields_group_rule(int64_t mean_len) {
  if (mean_len < 0) return kFieldsDefaultGroup;
  if (mean_len < 96) return 1;
  if (mean_len < 768) return 2;
  if (mean_len < 16384) return 4;
  return 64;
}

// bit k: byte k of w is one of 0x09 .. 0x0D, 0x20 -- bytes.isspace().  Exact, as lines_eq8: no carry leaves a byte
MRX_HD uint32_t fields_ws8(uint64_t w) {
  const uint64_t low7 = 0x7f7f7f7f7f7f7f7full, hi = 0x8080808080808080ull;
  const uint64_t y = w & low7;
  const uint64_t ge9 = y + 0x7777777777777777ull, ge14 = y + 0x7272727272727272ull;   // bit 7: y >= 9, y >= 14
  const uint64_t z = ge9 & ~ge14 & ~w & hi;
  return (uint32_t)(((z >> 7) * 0x0102040810204080ull) >> 56) | lines_eq8(w, 0x20);
}
MRX_HD uint32_t fields_ws16(g_u128 x) { return fields_ws8((uint64_t)x) | (fields_ws8((uint64_t)(x >> 64)) << 8); }

// the aligned words of a text of L bytes whose first byte is byte `head` of its word
MRX_HD int64_t fields_words(int head, int64_t L) { return L > 0 ? ((int64_t)head + L + 15) >> 4 : 0; }
// the bits of word w that are text
MRX_HD uint32_t fields_valid(int head, int64_t L, int64_t w) {
  const int64_t room = (int64_t)head + L - 16 * w;   // > 0: the word holds a byte of the text
  const uint32_t below = room >= 16 ? 0xffffu : (1u << (int)room) - 1u;
  return w == 0 ? below & ~((1u << head) - 1u) : below;
}
// delimiter mode: the word's delimiters.  whitespace mode: its bytes that are text and no whitespace
MRX_HD uint32_t fields_word_mask(const FieldsPlan& P, g_u128 word, uint32_t valid) {
  return fields_ws_mode(P) ? ~fields_ws16(word) & valid : lines_eq16(word, P.delim) & valid;
}
// whitespace mode: the starts and ends of a word from its mask m and the carry (the byte in front is text and no whitespace)
MRX_HD uint32_t fields_starts(uint32_t m, uint32_t carry) { return m & ~((m << 1) | carry) & 0xffffu; }
MRX_HD uint32_t fields_ends(uint32_t m, uint32_t carry) { return ~m & ((m << 1) | carry) & 0xffffu; }

// ---- quoted fields (include/mrx.h, "quoted fields") ---------------------------------------------------------------------
// Byte p of a text is inside when the quote bytes in t[0..p], p included, are odd in number: an opening quote is
// inside, a closing one is not.  A word's inside mask is the inclusive prefix-xor of its quote bits, turned over when
// the quotes of the text in front of the word are odd.  Within a round that parity comes from one ballot of the lanes'
// quote parities, cut to the lanes of the group in front of this one, and over the rounds it is carried as one bit.
MRX_HD bool fields_quote_ok_byte(uint32_t q) { return !((q >= 9 && q <= 13) || q == 32); }
// MRX_E_ARGUMENT's message for a quote that the mode cannot take, or nullptr
inline const char* fields_quote_check(uint32_t flags, uint8_t delim, uint8_t quote) {
  if (flags & ~kFieldsFlags) return nullptr;   // the plan refuses it by its own name
  if (flags & MRX_FIELDS_WHITESPACE) return fields_quote_ok_byte(quote) ? nullptr : "quote must not be a whitespace byte in whitespace mode";
  return quote != delim ? nullptr : "quote must differ from delim";
}
MRX_HD int fields_popc64(uint64_t m) { return lines_popc((uint32_t)m) + lines_popc((uint32_t)(m >> 32)); }
// bit k: the bits 0 .. k of q are odd in number (q: 16 bits)
MRX_HD uint32_t fields_prefix_xor16(uint32_t q) {
  q ^= q << 1;
  q ^= q << 2;
  q ^= q << 4;
  q ^= q << 8;
  return q & 0xffffu;
}
// a word's inside mask from its quote bits and the parity (0 or 1) of the quotes in front of it
MRX_HD uint32_t fields_inside(uint32_t q, uint32_t parity) { return (fields_prefix_xor16(q) ^ (0u - parity)) & 0xffffu; }
// the bits of group t's G lanes in a wavefront's ballot, lane 0 of the group at bit 0
MRX_HD uint64_t fields_group_bits(uint64_t ballot, int t, int G) {
  return G >= 64 ? ballot : (ballot >> (t * G)) & ((1ull << G) - 1ull);
}
// the parity of the group's lanes in front of lane gl, and of all of them
MRX_HD uint32_t fields_parity_front(uint64_t group_bits, int gl) { return (uint32_t)fields_popc64(group_bits & ((1ull << gl) - 1ull)) & 1u; }
MRX_HD uint32_t fields_parity_all(uint64_t group_bits) { return (uint32_t)fields_popc64(group_bits) & 1u; }
// fields_word_mask under quotes: a delimiter that is inside separates nothing; a whitespace byte that is inside counts
// as a byte that is none
MRX_HD uint32_t fields_word_mask_quoted(const FieldsPlan& P, g_u128 word, uint32_t valid, uint32_t inside) {
  return fields_ws_mode(P) ? (~fields_ws16(word) | inside) & valid : lines_eq16(word, P.delim) & ~inside & valid;
}
// A finished pair's content: a part of two bytes or more that begins and ends with the quote loses both.  tp: the
// text's first byte; only t[s] and t[e - 1] are read, and only of a part that exists.  Returns the quoted byte.
MRX_HD uint8_t fields_unquote(const uint8_t* tp, uint32_t quote, int32_t* s, int32_t* e) {
  if (*s < 0 || *e - *s < 2 || tp[*s] != quote || tp[*e - 1] != quote) return 0;
  *s += 1;
  *e -= 1;
  return 1;
}

// the position of set bit r of m (0 <= r < popcount(m))
MRX_HD int fields_kth(uint32_t m, int r) {
  for (; r > 0; --r) m &= m - 1;
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffs((int)m) - 1;
#else
  return __builtin_ctz(m);
#endif
}

// the field that column c names in a text of nf fields (0-based; outside [0, nf): none).  nf is read for c < 0 only
MRX_HD int64_t fields_index(int32_t c, int32_t nf) { return c > 0 ? (int64_t)c - 1 : (int64_t)nf + c; }

// A row's pairs before a walk: the pairs of this walk (negative = false: the positive columns; true: the negative
// ones, nf known) are (-1, L), or (0, L) for field 0 in delimiter mode.  j runs over the lane's share.
MRX_HD void fields_row_init(const FieldsPlan& P, bool negative, int32_t nf, int32_t L, int32_t* row, int j0, int step) {
  for (int j = j0; j < P.f; j += step) {
    const int32_t c = P.cols[j];
    if ((c < 0) != negative) continue;
    row[2 * j] = !fields_ws_mode(P) && fields_index(c, nf) == 0 ? 0 : -1;
    row[2 * j + 1] = L;
  }
}

// One lane's word in a walk: a and b are its event masks, ra and rb the events of the text in front of the word, p0 the
// text position of the word's bit 0.  Every pair of this walk whose start or end is one of the word's events gets it.
MRX_HD void fields_select(const FieldsPlan& P, bool negative, int32_t nf, uint32_t a, uint32_t b, int64_t ra, int64_t rb,
                          int64_t p0, int32_t* row) {
  const int ca = lines_popc(a), cb = lines_popc(b);
  const int64_t sadd = fields_ws_mode(P) ? 0 : 1;
  for (int j = 0; j < P.f; ++j) {
    const int32_t c = P.cols[j];
    if ((c < 0) != negative) continue;
    const int64_t q = fields_index(c, nf);
    if (q < 0) continue;
    const int64_t sa = fields_rank_a(P, q) - ra;
    if (sa >= 0 && sa < ca) row[2 * j] = (int32_t)(p0 + fields_kth(a, (int)sa) + sadd);
    const int64_t sb = q - rb;
    if (sb >= 0 && sb < cb && fields_has_end(P, c)) row[2 * j + 1] = (int32_t)(p0 + fields_kth(b, (int)sb));
  }
}
// has a walk that may stop seen all it needs (ra, rb: the events so far)
MRX_HD bool fields_done(const FieldsPlan& P, int64_t ra, int64_t rb) { return ra > P.k_a && rb > P.k_b; }
// nf from the a-events of a whole walk, or of one that stopped under REST
MRX_HD int32_t fields_count(const FieldsPlan& P, int64_t ra) {
  const int64_t nf = fields_ws_mode(P) ? ra : ra + 1;
  return (int32_t)((P.flags & MRX_FIELDS_REST) && nf > P.cmax ? P.cmax : nf);
}
// a finished pair as it leaves: a part that does not exist is (-1, -1)
MRX_HD void fields_finish(int32_t* s, int32_t* e) { if (*s < 0) *e = -1; }

// ---- host only: one text, as a group of G lanes walks it ---------------------------------------------------------------
// The aligned 16-byte words around the text must be readable.  row: int32[f][2].  quote >= 0: quoted fields with that
// quote byte, and quoted (uint8[f], may be null) takes the row's quoted bytes.
inline void fields_host_text(const FieldsPlan& P, int G, const uint8_t* tp, int64_t L, int32_t* row, int32_t* nf_out,
                             int quote = -1, uint8_t* quoted = nullptr) {
  const int head = (int)((uintptr_t)tp & 15);
  const uint8_t* base = tp - head;
  const int64_t nwords = fields_words(head, L);
  int32_t nf = 0;
  for (int pass = 0; pass < (P.any_neg ? 2 : 1); ++pass) {
    const bool negative = pass == 1;
    for (int l = 0; l < G; ++l) fields_row_init(P, negative, nf, (int32_t)L, row, l, G);
    int64_t ra = 0, rb = 0;
    uint32_t carry = 0, parity = 0;   // every walk begins outside
    for (int64_t w0 = 0; w0 < nwords; w0 += G) {
      if (!negative && P.stop && fields_done(P, ra, rb)) break;
      int64_t ea = ra, eb = rb;   // the running prefix over the lanes of the round
      uint64_t ballot = 0;        // the group's lanes whose word holds an odd number of quotes
      if (quote >= 0)
        for (int l = 0; l < G && w0 + l < nwords; ++l) {
          const uint32_t q = lines_eq16(gather_window(base + 16 * (w0 + l), 16), (uint32_t)quote) & fields_valid(head, L, w0 + l);
          ballot |= (uint64_t)(lines_popc(q) & 1) << l;
        }
      for (int l = 0; l < G && w0 + l < nwords; ++l) {
        const int64_t w = w0 + l;
        const g_u128 word = gather_window(base + 16 * w, 16);
        const uint32_t valid = fields_valid(head, L, w);
        uint32_t m;
        if (quote >= 0) {
          const uint32_t q = lines_eq16(word, (uint32_t)quote) & valid;
          m = fields_word_mask_quoted(P, word, valid, fields_inside(q, fields_parity_front(fields_group_bits(ballot, 0, G), l) ^ parity));
        } else {
          m = fields_word_mask(P, word, valid);
        }
        uint32_t a = m, b = m;
        if (fields_ws_mode(P)) {
          a = fields_starts(m, carry);
          b = fields_ends(m, carry);
          carry = (m >> 15) & 1u;
        }
        if (a | b) fields_select(P, negative, nf, a, b, ea, eb, 16 * w - head, row);
        ea += lines_popc(a);
        eb += lines_popc(b);
      }
      ra = ea;
      rb = eb;
      parity ^= fields_parity_all(fields_group_bits(ballot, 0, G));
    }
    if (!negative) nf = fields_count(P, ra);
  }
  for (int j = 0; j < P.f; ++j) {
    fields_finish(&row[2 * j], &row[2 * j + 1]);
    if (quote >= 0) {
      const uint8_t was = fields_unquote(tp, (uint32_t)quote, &row[2 * j], &row[2 * j + 1]);
      if (quoted) quoted[j] = was;
    }
  }
  if (nf_out) *nf_out = nf;
}

}  // namespace mrx
