// Host check of a dictionary's probe walk (mojo_regex_amd/csrc/mrx_lookup_bits.hpp, on top of mrx_distinct_bits.hpp)
// against std::map, meant for the host sanitizers: no kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/lookup_check.cpp -o lookup_check && ./lookup_check
//
// The table is built on the CPU with the slot encoding of mrx_lookup_bits.hpp and the insert rule of k_distinct_insert:
// an entry walks from its home slot, takes the first empty slot or stops at a slot with its tag whose entry has its
// bytes.  The entries are inserted in a shuffled order, as a race on the device would have it, so the representative of
// a group is not its lowest index; the lowest index per representative is then written into the slots, as the build's
// last kernel does.  Under hash masks all ones, 3 (four chains) and 0 (one chain with equal tags: every decision is a
// byte comparison):
//   - the entries' packed bytes lie at every alignment 0..15 inside a buffer of exactly the aligned 16-byte words that
//     hold them, and every probed text in a buffer of its own of the same kind, so a read outside the words that the
//     read contract of include/mrx.h allows is the sanitizer's to report; everything else in the buffers is poison, and
//     the poison is changed between two evaluations;
//   - lookup_walk must return what std::map says: the lowest index of an equal entry, or -1.  The probes are the
//     entries themselves, each with its last byte changed, with a trailing \0 more and without its last byte, and
//     random texts over the entries' alphabet.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the headers' host + device qualifiers)

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_lookup_bits.hpp"

using namespace mrx;

namespace {

using Text = std::vector<uint8_t>;

// `bytes` at alignment `skew` in a fresh buffer of exactly the aligned words that hold them; the rest is `poison`
struct Placed {
  uint8_t* buf;
  const uint8_t* p;
  Placed(const Text& bytes, int skew, uint8_t poison) {
    const size_t words = bytes.empty() ? 1 : (skew + bytes.size() + 15) / 16;
    buf = (uint8_t*)aligned_alloc(16, words * 16);
    memset(buf, poison, words * 16);
    if (!bytes.empty()) memcpy(buf + skew, bytes.data(), bytes.size());
    p = buf + skew;
  }
  ~Placed() { free(buf); }
  Placed(const Placed&) = delete;
};

struct Table {
  std::vector<uint64_t> words;
  uint64_t slots = 2, mask = ~0ull;
};

// k_distinct_insert, k_distinct_first and k_dict_fixup on the CPU, the entries taken in `order`
bool build(const std::vector<Text>& entries, const std::vector<size_t>& order, uint64_t mask, Table* t) {
  const size_t m = entries.size();
  t->mask = mask;
  t->slots = 2;
  while (t->slots < 2 * (uint64_t)m) t->slots <<= 1;
  t->words.assign((size_t)t->slots, 0);
  std::vector<int64_t> rep_of(m, -1), first_at(m, INT64_MAX);
  for (size_t i : order) {
    const Text& e = entries[i];
    const Placed own(e, (int)(i % 16), 0x5A);   // (the hash reads whole aligned words: not from the vector's own memory)
    const uint64_t h = distinct_hash(own.p, (int64_t)e.size()) & mask;
    for (uint64_t probe = 0; probe < t->slots && rep_of[i] < 0; ++probe) {
      uint64_t& word = t->words[(size_t)((h + probe) & (t->slots - 1))];
      if (word == 0) {
        word = lookup_slot_word(h, (int64_t)i);
        rep_of[i] = (int64_t)i;
      } else if (lookup_slot_tag(word) == (h >> 32)) {
        if (entries[(size_t)lookup_slot_index(word)] == e) rep_of[i] = lookup_slot_index(word);
      }
    }
    if (rep_of[i] < 0) return false;   // the probe ran out
  }
  for (size_t i = 0; i < m; ++i) first_at[(size_t)rep_of[i]] = std::min(first_at[(size_t)rep_of[i]], (int64_t)i);
  for (uint64_t& word : t->words)
    if (word) word = lookup_slot_word(word, first_at[(size_t)lookup_slot_index(word)]);
  return true;
}

std::vector<Text> make_entries(std::mt19937& rng) {
  std::vector<Text> e;
  for (int L = 0; L <= 49; ++L) {   // lengths 0..49 over four letters: prefixes and near misses abound
    Text t((size_t)L);
    for (auto& c : t) c = (uint8_t)('a' + rng() % 4);
    e.push_back(t);
  }
  for (int L : {63, 64, 65, 255, 256, 257, 1000, 4097}) {
    Text t((size_t)L);
    for (auto& c : t) c = (uint8_t)rng();
    e.push_back(t);
  }
  e.push_back({});
  e.push_back({'a'});
  e.push_back({'a', 0});
  e.push_back({0});
  e.push_back(Text(33, 0));
  e.push_back(Text(33, 0xFF));
  for (int k = 0; k < 60; ++k) {   // many short ones, with repeats
    Text t((size_t)(rng() % 4));
    for (auto& c : t) c = (uint8_t)('a' + rng() % 2);
    e.push_back(t);
  }
  for (int k : {0, 7, 16, 33, 49, 55, 57}) e.push_back(e[(size_t)k]);   // duplicates at distance
  return e;
}

std::vector<Text> make_probes(const std::vector<Text>& entries, std::mt19937& rng) {
  std::vector<Text> p(entries);
  for (const Text& e : entries) {
    if (!e.empty()) {
      Text other(e);
      other.back() ^= 1;
      p.push_back(other);
      p.push_back(Text(e.begin(), e.end() - 1));
    }
    Text nul(e);
    nul.push_back(0);
    p.push_back(nul);
  }
  for (int k = 0; k < 200; ++k) {
    Text t((size_t)(rng() % 20));
    for (auto& c : t) c = (uint8_t)('a' + rng() % 4);
    p.push_back(t);
  }
  return p;
}

}  // namespace

int main() {
  std::mt19937 rng(20260401);
  const std::vector<Text> entries = make_entries(rng);
  const std::vector<Text> probes = make_probes(entries, rng);
  const size_t m = entries.size();
  std::map<Text, int64_t> lowest;
  for (size_t i = 0; i < m; ++i) lowest.emplace(entries[i], (int64_t)i);   // (emplace keeps the first)
  Text packed;
  std::vector<int64_t> offsets(m + 1, 0);
  for (size_t i = 0; i < m; ++i) {
    packed.insert(packed.end(), entries[i].begin(), entries[i].end());
    offsets[i + 1] = (int64_t)packed.size();
  }
  std::vector<size_t> order(m);
  for (size_t i = 0; i < m; ++i) order[i] = i;
  long walks = 0, hits = 0;
  for (uint64_t mask : {~0ull, 3ull, 0ull}) {
    std::shuffle(order.begin(), order.end(), rng);
    Table t;
    if (!build(entries, order, mask, &t)) {
      printf("FAIL: mask %llx: the build's probe ran out\n", (unsigned long long)mask);
      return 1;
    }
    size_t occupied = 0;
    for (uint64_t w : t.words) occupied += w != 0;
    if (occupied != lowest.size()) {
      printf("FAIL: mask %llx: %zu occupied slots for %zu different entries\n", (unsigned long long)mask, occupied, lowest.size());
      return 1;
    }
    for (int eskew = 0; eskew < 16; ++eskew) {
      const Placed ecopy(packed, eskew, eskew % 2 ? 0x00 : 0xA5);
      for (size_t q = 0; q < probes.size(); ++q) {
        const Text& text = probes[q];
        const auto it = lowest.find(text);
        const int64_t want = it == lowest.end() ? -1 : it->second;
        // every alignment of the probed text against this alignment of the entries for the short ones, four for the rest
        const int step = text.size() <= 49 ? 1 : 5;
        for (int skew = (eskew * 3) % step; skew < 16; skew += step) {
          const Placed a(text, skew, (skew + eskew) % 2 ? 0xA5 : 0x00);
          const uint64_t h = distinct_hash(a.p, (int64_t)text.size()) & t.mask;
          const int64_t got = lookup_walk(t.words.data(), t.slots, h, a.p, (int64_t)text.size(), ecopy.p, offsets.data());
          if (got != want) {
            printf("FAIL: mask %llx: probe %zu (length %zu) at alignment %d, entries at %d: got %lld, want %lld\n",
                   (unsigned long long)mask, q, text.size(), skew, eskew, (long long)got, (long long)want);
            return 1;
          }
          ++walks;
          hits += got >= 0;
        }
      }
    }
  }
  printf("ok: %zu entries (%zu different), %zu probes, %ld walks of which %ld hit: lookup_walk agrees with std::map under "
         "hash masks all ones, 3 and 0 at every alignment\n", m, lowest.size(), probes.size(), walks, hits);
  return 0;
}
