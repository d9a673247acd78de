// Sort's judgements of a text (mrx_sort.hip): the 8 bytes of a text at depth d as one big-endian word with the number of
// them that exist, the radix digit of a round's key, and the three-way comparison of two texts from a depth on.  All
// read a text through gather_window, so only the aligned 16-byte words that hold a byte of the text are loaded, and
// whatever those words hold outside the text is masked away before it can reach a result.  Host and device code, so
// that they also run on the CPU against std::lexicographical_compare (tools/sort_check.cpp).
//
// The order is that of Python's bytes: bytewise, unsigned, a proper prefix first.  A big-endian word compares as its
// bytes do; behind a text's end the word is zero, and `valid`, the number of real bytes in it, breaks the tie that the
// padding leaves: "a" and "a\0" have equal words and valid 1 < 2.  Texts whose (word, valid) agree at every depth up
// to one with valid < 8 are equal.
#pragma once
#include <cstdint>

#include "mrx_gather_bits.hpp"

namespace mrx {

// bytes [d, d + 8) of the text of L bytes at p, the first one in the highest byte, zero behind the text's end;
// *valid = clamp(L - d, 0, 8).  Nothing is loaded when valid is 0.
MRX_HD uint64_t sort_word(const uint8_t* p, int64_t L, int64_t d, int* valid) {
  const int64_t left = L - d;
  const int v = left <= 0 ? 0 : left < 8 ? (int)left : 8;
  *valid = v;
  if (v == 0) return 0;
  uint64_t w = (uint64_t)gather_window(p + d, v);
  if (v < 8) w &= ((uint64_t)1 << (8 * v)) - 1;
  return __builtin_bswap64(w);
}

// A round's comparison key is (group, word, valid), kept as two words: `word`, and gv = group << 8 | valid.  The radix
// passes take its 8-bit digits from the least significant one: pass 0 is valid, passes 1..8 the word's bytes from its
// last to its first, passes 9.. the bytes of the group number.
MRX_HD unsigned sort_digit(uint64_t word, uint64_t gv, int pass) {
  if (pass == 0) return (unsigned)(gv & 0xff);
  if (pass <= 8) return (unsigned)(word >> (8 * (pass - 1))) & 0xff;
  return (unsigned)(gv >> (8 * (pass - 8))) & 0xff;
}

// how many passes over the group number a round with `groups` groups needs (none for one group)
MRX_HD int sort_group_passes(int64_t groups) {
  int passes = 0;
  for (int64_t top = groups - 1; top > 0; top >>= 8) ++passes;
  return passes;
}

// < 0, 0, > 0 as text a sorts before, equal to, behind text b, given that their first `from` bytes agree (both texts
// have them, or both end before): 8 bytes a step
MRX_HD int sort_compare(const uint8_t* a, int64_t La, const uint8_t* b, int64_t Lb, int64_t from) {
  for (int64_t d = from;; d += 8) {
    int va, vb;
    const uint64_t wa = sort_word(a, La, d, &va), wb = sort_word(b, Lb, d, &vb);
    if (wa != wb) return wa < wb ? -1 : 1;
    if (va != vb) return va < vb ? -1 : 1;
    if (va < 8) return 0;
  }
}

}  // namespace mrx
