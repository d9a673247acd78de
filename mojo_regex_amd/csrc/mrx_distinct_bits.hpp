// Distinct's two judgements of a text (mrx_distinct.hip): its 64-bit hash and the bytewise comparison with another
// text.  Both read a text as its 16-byte blocks -- block j is bytes [16 j, 16 j + 16) of the text, the last one cut at
// the text's end -- through gather_window, so only the aligned 16-byte words that hold a byte of the text are loaded,
// and whatever those words hold outside the text is masked away before it can reach a result.  Host and device code, so
// that both also run on the CPU against memcmp and under every block order (tools/distinct_check.cpp).
//
// The hash is order free: every block is mixed with its index on its own, the mixed blocks are ADDED (wrapping 64-bit
// addition: commutative and associative), and the sum is mixed once more with the length.  Any partition of the blocks
// over lanes, walked in any order, therefore gives the same value; k_distinct_hash stripes a text's blocks over 16
// lanes, a host restatement may walk them front to back.
#pragma once
#include <cstdint>

#include "mrx_gather_bits.hpp"

namespace mrx {

// the finalizer of splitmix64: a bijection of 64 bits
MRX_HD uint64_t distinct_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// block j of a text of L bytes at p (0 <= 16 j < L): its bytes as a little-endian value, zero behind the text's end
MRX_HD g_u128 distinct_load(const uint8_t* p, int64_t L, int64_t j) {
  const int64_t left = L - 16 * j;
  const int need = left < 16 ? (int)left : 16;
  g_u128 v = gather_window(p + 16 * j, need);
  if (need < 16) v &= ((g_u128)1 << (8 * need)) - 1;
  return v;
}

// one block's term of the sum: both halves and the block's index go through the mixer
MRX_HD uint64_t distinct_term(g_u128 v, int64_t j) {
  const uint64_t a = distinct_mix((uint64_t)v + 0x9e3779b97f4a7c15ull * (uint64_t)(2 * j + 1));
  const uint64_t b = distinct_mix((uint64_t)(v >> 64) ^ a ^ (0xc2b2ae3d27d4eb4full * (uint64_t)(2 * j + 2)));
  return a + 3 * b;
}

// the terms of the blocks first, first + step, ... of the text, added up
MRX_HD uint64_t distinct_partial(const uint8_t* p, int64_t L, int64_t first, int64_t step) {
  uint64_t sum = 0;
  for (int64_t j = first; 16 * j < L; j += step) sum += distinct_term(distinct_load(p, L, j), j);
  return sum;
}

// the hash from the sum of all the blocks' terms.  The length goes in here: "a" and "a\0" have the same one block
MRX_HD uint64_t distinct_finish(uint64_t sum, int64_t L) {
  return distinct_mix(sum ^ distinct_mix(0xd6e8feb86659fd93ull + (uint64_t)L));
}

MRX_HD uint64_t distinct_hash(const uint8_t* p, int64_t L) { return distinct_finish(distinct_partial(p, L, 0, 1), L); }

// are the L bytes at a and at b the same?  (The lengths have been compared by the caller; L == 0 loads nothing.)
MRX_HD bool distinct_equal(const uint8_t* a, const uint8_t* b, int64_t L) {
  for (int64_t j = 0; 16 * j < L; ++j)
    if (distinct_load(a, L, j) != distinct_load(b, L, j)) return false;
  return true;
}

}  // namespace mrx
