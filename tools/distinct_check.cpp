// Host check of distinct's hash and comparison (mojo_regex_amd/csrc/mrx_distinct_bits.hpp, on top of
// mrx_gather_bits.hpp) against memcmp and against themselves under every block order, meant for the host sanitizers: no
// kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/distinct_check.cpp -o distinct_check && ./distinct_check
//
// A text of every length 0..49 (and a few long ones) is placed at every alignment 0..15 inside a buffer of whole
// 16-byte words and not a byte more than the words that hold the text, as the read contract of include/mrx.h allows, so
// a read outside them is the sanitizer's to report.  Everything in the buffer that is not the text is poison, and the
// poison is changed between two evaluations:
//   - the hash must be the same at every alignment and under both poisons: nothing outside the text reaches it;
//   - the hash must be the same under every block order: front to back, backwards, and striped over 2, 4 and 16
//     "lanes" whose parts are added in lane order and in reverse (the sum k_distinct_hash builds with its shuffles);
//   - distinct_equal must agree with memcmp for the text against itself at another alignment, against the text with
//     one byte changed (every position), and against texts that differ only behind a zero byte;
//   - a text and the same text with a trailing \0, and a text and its proper prefix, must hash differently (they are
//     different texts; a collision here would be a defect of the length mix, not a wrong result).
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the header's host + device qualifiers)

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_distinct_bits.hpp"

using namespace mrx;

namespace {

// `text` at alignment `skew` in a fresh buffer of exactly the aligned words that hold it; the rest is `poison`
struct Placed {
  uint8_t* buf;
  const uint8_t* p;
  Placed(const std::vector<uint8_t>& text, int skew, uint8_t poison) {
    const size_t words = text.empty() ? 1 : (skew + text.size() + 15) / 16;
    buf = (uint8_t*)aligned_alloc(16, words * 16);
    memset(buf, poison, words * 16);
    if (!text.empty()) memcpy(buf + skew, text.data(), text.size());
    p = buf + skew;
  }
  ~Placed() { free(buf); }
  Placed(const Placed&) = delete;
};

uint64_t hash_backwards(const uint8_t* p, int64_t L) {
  uint64_t sum = 0;
  for (int64_t j = (L + 15) / 16 - 1; j >= 0; --j) sum += distinct_term(distinct_load(p, L, j), j);
  return distinct_finish(sum, L);
}

uint64_t hash_striped(const uint8_t* p, int64_t L, int lanes, bool reverse) {
  uint64_t sum = 0;
  for (int k = 0; k < lanes; ++k) sum += distinct_partial(p, L, reverse ? lanes - 1 - k : k, lanes);
  return distinct_finish(sum, L);
}

int check_text(const std::vector<uint8_t>& text, int* checked) {
  const int64_t L = (int64_t)text.size();
  uint64_t want = 0;
  for (int skew = 0; skew < 16; ++skew) {
    for (int pz = 0; pz < 2; ++pz) {
      const Placed a(text, skew, pz ? 0x00 : 0xA5);
      const uint64_t h = distinct_hash(a.p, L);
      if (skew == 0 && pz == 0) want = h;
      if (h != want) {
        printf("FAIL: length %lld: the hash at alignment %d, poison %d differs\n", (long long)L, skew, pz);
        return 1;
      }
      if (hash_backwards(a.p, L) != want) {
        printf("FAIL: length %lld: the hash backwards differs\n", (long long)L);
        return 1;
      }
      for (int lanes : {2, 4, 16})
        for (int rev = 0; rev < 2; ++rev)
          if (hash_striped(a.p, L, lanes, rev != 0) != want) {
            printf("FAIL: length %lld: the hash over %d lanes differs\n", (long long)L, lanes);
            return 1;
          }
      // the comparison: the same text at another alignment under the other poison
      const Placed b(text, (skew * 7 + 3) & 15, pz ? 0xA5 : 0x00);
      if (!distinct_equal(a.p, b.p, L) || !distinct_equal(b.p, a.p, L)) {
        printf("FAIL: length %lld: equal texts compare unequal (alignment %d)\n", (long long)L, skew);
        return 1;
      }
      ++*checked;
    }
    // one byte changed, at every position
    const Placed a(text, skew, 0x5A);
    for (int64_t q = 0; q < L; ++q) {
      std::vector<uint8_t> other(text);
      other[(size_t)q] ^= (uint8_t)(q % 2 ? 0x01 : 0x80);
      const Placed b(other, (skew + 5) & 15, 0x5A);
      const bool eq = distinct_equal(a.p, b.p, L), ref = memcmp(text.data(), other.data(), (size_t)L) == 0;
      if (eq != ref) {
        printf("FAIL: length %lld: byte %lld changed, equal = %d\n", (long long)L, (long long)q, (int)eq);
        return 1;
      }
      if (distinct_hash(b.p, L) == want) {
        printf("FAIL: length %lld: byte %lld changed and the hash did not\n", (long long)L, (long long)q);
        return 1;
      }
    }
  }
  // a trailing \0 and a proper prefix are other texts: same leading blocks, another length
  std::vector<uint8_t> nul(text);
  nul.push_back(0);
  const Placed a(text, 3, 0x00), b(nul, 3, 0x00);
  if (distinct_hash(b.p, L + 1) == want) {
    printf("FAIL: length %lld: a trailing zero byte does not change the hash\n", (long long)L);
    return 1;
  }
  if (L > 0) {
    std::vector<uint8_t> prefix(text.begin(), text.end() - 1);
    const Placed c(prefix, 9, 0xA5);
    if (distinct_hash(c.p, L - 1) == want) {
      printf("FAIL: length %lld: the proper prefix has the same hash\n", (long long)L);
      return 1;
    }
    if (!distinct_equal(a.p, c.p, L - 1)) {   // (the caller compares lengths first: over L - 1 bytes they are equal)
      printf("FAIL: length %lld: the prefix's bytes compare unequal\n", (long long)L);
      return 1;
    }
  }
  return 0;
}

}  // namespace

int main() {
  std::mt19937 rng(20260301);
  int checked = 0;
  std::vector<int> lengths;
  for (int L = 0; L <= 49; ++L) lengths.push_back(L);
  for (int L : {63, 64, 65, 255, 256, 257, 1000, 4097}) lengths.push_back(L);
  for (int L : lengths)
    for (int kind = 0; kind < 3; ++kind) {   // random bytes, all zero, all 0xFF
      std::vector<uint8_t> text((size_t)L);
      for (auto& c : text) c = kind == 0 ? (uint8_t)rng() : kind == 1 ? 0x00 : 0xFF;
      if (check_text(text, &checked)) return 1;
    }
  printf("ok: %d placements: the hash sees the text alone and is the same under every block order, "
         "the comparison agrees with memcmp\n", checked);
  return 0;
}
