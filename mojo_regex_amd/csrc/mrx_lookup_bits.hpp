// A dictionary's table (mrx_lookup.hip): the encoding of a slot and the walk that answers a probe.  Host and device
// code on top of mrx_distinct_bits.hpp, so that the walk also runs on the CPU against std::map, inside poisoned buffers
// and under the host sanitizers (tools/lookup_check.cpp).
//
// The table is open addressing over `slots` 64-bit words, a power of two.  A word is 0 (empty) or
//   (high 32 bits of the entry's hash) << 32 | (an entry's index + 1).
// While the table is built the index is the representative's, whichever entry of a group took the slot (distinct's
// insert rule, k_distinct_insert); the build's last kernel rewrites it to the LOWEST index of the group, and from then
// on the table is read-only and answers a probe alone.  A text's home slot is hash & (slots - 1); groups that collide
// step on to the next slot, so a walk passes every slot its text could have been put in before it meets an empty one.
#pragma once
#include <cstdint>

#include "mrx_distinct_bits.hpp"

namespace mrx {

MRX_HD uint64_t lookup_slot_word(uint64_t hash, int64_t index) { return ((hash >> 32) << 32) | (uint64_t)(index + 1); }
MRX_HD uint64_t lookup_slot_tag(uint64_t word) { return word >> 32; }
MRX_HD int64_t lookup_slot_index(uint64_t word) { return (int64_t)(word & 0xffffffffull) - 1; }

// The index that the table holds for the text of L bytes at tp with hash h (already masked as the table's hashes
// were), or -1: from the home slot on, an empty slot ends the walk with -1, a slot with the hash's tag is compared
// bytewise with its entry -- text e of the CSR (e_data, e_offsets) -- and equal ends the walk with the slot's index,
// anything else steps on.  A hash decides nothing by itself.  At most `slots` probes; plain loads, no store.
MRX_HD int64_t lookup_walk(const uint64_t* table, uint64_t slots, uint64_t h, const uint8_t* tp, int64_t L,
                           const uint8_t* e_data, const int64_t* e_offsets) {
  const uint64_t tag = h >> 32;
  for (uint64_t probe = 0; probe < slots; ++probe) {
    const uint64_t word = table[(h + probe) & (slots - 1)];
    if (word == 0) return -1;
    if (lookup_slot_tag(word) != tag) continue;
    const int64_t e = lookup_slot_index(word);
    const int64_t a = e_offsets[e];
    if (e_offsets[e + 1] - a == L && distinct_equal(tp, e_data + a, L)) return e;
  }
  return -1;   // (a table at load <= 1/2 always has an empty slot: unreachable)
}

}  // namespace mrx
