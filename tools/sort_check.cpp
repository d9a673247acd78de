// Host check of sort's judgements of a text (mojo_regex_amd/csrc/mrx_sort_bits.hpp) against
// std::lexicographical_compare and std::stable_sort, meant for the host sanitizers: no kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/sort_check.cpp -o sort_check && ./sort_check
//
// Every text lies at some alignment 0..15 inside a buffer of exactly the aligned 16-byte words that hold it, so a read
// outside the words that the read contract of include/mrx.h allows is the sanitizer's to report; everything else in
// the buffers is poison (zero bytes, 0xFF, the text's own letters), which a missing mask would turn into a wrong key.
//   - sort_word and its `valid` at every depth 0, 8, ... of every text against the bytes themselves;
//   - sort_compare, from 0 and from every multiple of 8 inside the common prefix, against
//     std::lexicographical_compare, on every pair of lengths 0..40 that share a prefix (the prefix rule), continue
//     differently (bytes 0x00, 0x7f, 0x80, 0xff among them) or are equal;
//   - the route of mrx_sort.hip restated on the CPU with the same helpers -- rounds of 8 bytes, stable counting passes
//     over sort_digit in the order valid, word bytes, group bytes, groups from key changes, groups of at most `small`
//     members finished by sort_compare -- against std::stable_sort, with small = 64, 3 and 0, on texts with heavy
//     ties, long shared prefixes and trailing NULs.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the headers' host + device qualifiers)

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_sort_bits.hpp"

using namespace mrx;

namespace {

using Text = std::vector<uint8_t>;

// `bytes` at alignment `skew` in a fresh buffer of exactly the aligned words that hold them; the rest is `poison`
struct Placed {
  uint8_t* buf;
  const uint8_t* p;
  int64_t L;
  Placed(const Text& bytes, int skew, uint8_t poison) : L((int64_t)bytes.size()) {
    const size_t words = bytes.empty() ? 1 : (skew + bytes.size() + 15) / 16;
    buf = (uint8_t*)aligned_alloc(16, words * 16);
    memset(buf, poison, words * 16);
    if (!bytes.empty()) memcpy(buf + skew, bytes.data(), bytes.size());
    p = buf + skew;
  }
  ~Placed() { free(buf); }
  Placed(const Placed&) = delete;
};

int sign(int x) { return x < 0 ? -1 : x > 0 ? 1 : 0; }

int reference_compare(const Text& a, const Text& b) {
  if (std::lexicographical_compare(a.begin(), a.end(), b.begin(), b.end())) return -1;
  if (std::lexicographical_compare(b.begin(), b.end(), a.begin(), a.end())) return 1;
  return 0;
}

bool check_words(const Text& t, const Placed& at) {
  for (int64_t d = 0; d <= (int64_t)t.size() + 8; d += 8) {
    int valid = -1;
    const uint64_t got = sort_word(at.p, at.L, d, &valid);
    const int64_t left = (int64_t)t.size() - d;
    const int want_valid = left <= 0 ? 0 : left < 8 ? (int)left : 8;
    uint64_t want = 0;
    for (int k = 0; k < want_valid; ++k) want |= (uint64_t)t[(size_t)(d + k)] << (8 * (7 - k));
    if (got != want || valid != want_valid) {
      printf("FAIL: sort_word of a text of %zu bytes at depth %lld: %016llx / %d, want %016llx / %d\n", t.size(), (long long)d,
             (unsigned long long)got, valid, (unsigned long long)want, want_valid);
      return false;
    }
  }
  return true;
}

// mrx_sort.hip's rounds on the CPU.  Returns the order; *rounds receives the number of rounds.
std::vector<int64_t> route_sort(const std::vector<Placed*>& texts, int small, int* rounds) {
  const size_t n = texts.size();
  std::vector<int64_t> order(n, -1);
  struct Elem { uint64_t word, gv; uint32_t idx; };
  std::vector<Elem> cur(n);
  std::vector<size_t> pos(n);
  for (size_t j = 0; j < n; ++j) { cur[j] = Elem{0, 0, (uint32_t)j}; pos[j] = j; }
  int64_t groups = 1;
  *rounds = 0;
  for (int64_t d = 0; !cur.empty(); d += 8, ++*rounds) {
    const size_t m = cur.size();
    for (Elem& e : cur) {
      int valid;
      e.word = sort_word(texts[e.idx]->p, texts[e.idx]->L, d, &valid);
      e.gv |= (uint64_t)valid;
    }
    for (int pass = 0; pass <= 8 + sort_group_passes(groups); ++pass) {   // a stable counting pass per digit
      std::vector<size_t> first(257, 0);
      for (const Elem& e : cur) ++first[sort_digit(e.word, e.gv, pass) + 1];
      for (int q = 0; q < 256; ++q) first[q + 1] += first[q];
      std::vector<Elem> out(m);
      for (const Elem& e : cur) out[first[sort_digit(e.word, e.gv, pass)]++] = e;
      cur.swap(out);
    }
    std::vector<Elem> next;
    std::vector<size_t> next_pos;
    int64_t next_groups = 0;
    for (size_t h = 0; h < m;) {
      size_t e = h + 1;
      while (e < m && cur[e].word == cur[h].word && cur[e].gv == cur[h].gv) ++e;
      const size_t size = e - h;
      if (size == 1 || (cur[h].gv & 0xff) < 8) {
        for (size_t j = h; j < e; ++j) order[pos[h] + (j - h)] = cur[j].idx;
      } else if (size <= (size_t)small) {
        for (size_t j = h; j < e; ++j) {
          size_t smaller = 0;
          for (size_t q = h; q < e; ++q) {
            if (q == j) continue;
            const int c = sort_compare(texts[cur[q].idx]->p, texts[cur[q].idx]->L, texts[cur[j].idx]->p, texts[cur[j].idx]->L, d + 8);
            if (c < 0 || (c == 0 && q < j)) ++smaller;
          }
          order[pos[h] + smaller] = cur[j].idx;
        }
      } else {
        for (size_t j = h; j < e; ++j) {
          next.push_back(Elem{0, (uint64_t)next_groups << 8, cur[j].idx});
          next_pos.push_back(pos[j]);
        }
        ++next_groups;
      }
      h = e;
    }
    cur.swap(next);
    pos.swap(next_pos);
    groups = next_groups;
  }
  return order;
}

bool check_route(const std::vector<Text>& texts, const char* what) {
  std::vector<Placed*> placed;
  for (size_t i = 0; i < texts.size(); ++i) placed.push_back(new Placed(texts[i], (int)(i * 7 % 16), i % 3 == 0 ? 0x00 : i % 3 == 1 ? 0xFF : 'a'));
  std::vector<int64_t> want(texts.size());
  std::iota(want.begin(), want.end(), 0);
  std::stable_sort(want.begin(), want.end(), [&](int64_t a, int64_t b) { return reference_compare(texts[(size_t)a], texts[(size_t)b]) < 0; });
  bool ok = true;
  for (int small : {64, 3, 0}) {
    int rounds = 0;
    const std::vector<int64_t> got = route_sort(placed, small, &rounds);
    if (got != want) {
      printf("FAIL: %s with small = %d: the route's order differs from std::stable_sort\n", what, small);
      ok = false;
    } else {
      printf("ok: %s: %zu texts, small = %d, %d rounds\n", what, texts.size(), small, rounds);
    }
  }
  for (Placed* p : placed) delete p;
  return ok;
}

}  // namespace

int main() {
  std::mt19937 rng(20260501);
  long words = 0, compares = 0;
  // every pair of lengths 0..40: a common prefix of c bytes, then the texts go on in every way that matters
  const uint8_t edge[] = {0x00, 0x01, 0x7f, 0x80, 0xff, 'a'};
  for (int la = 0; la <= 40; ++la) {
    for (int lb = 0; lb <= 40; ++lb) {
      const int lo = std::min(la, lb);
      for (int c : {lo, lo / 2, std::max(0, lo - 1), std::max(0, lo - 8)}) {
        Text a((size_t)la), b((size_t)lb);
        for (int k = 0; k < la; ++k) a[(size_t)k] = (k + 1) % 9 == 0 ? 0 : (uint8_t)rng();
        for (int k = 0; k < lb; ++k) b[(size_t)k] = k < c ? a[(size_t)k] : edge[rng() % 6];
        if (c < la && c < lb && a[(size_t)c] == b[(size_t)c]) a[(size_t)c] = (uint8_t)(b[(size_t)c] ^ 0x80);
        int common = 0;
        while (common < lo && a[(size_t)common] == b[(size_t)common]) ++common;
        const int want = reference_compare(a, b);
        const int ska = (la * 5 + lb) % 16, skb = (lb * 3 + la + c) % 16;
        for (uint8_t poison : {(uint8_t)0x00, (uint8_t)0xFF}) {
          const Placed pa(a, ska, poison), pb(b, skb, (uint8_t)~poison);
          if (!check_words(a, pa) || !check_words(b, pb)) return 1;
          words += 2;
          // from: any multiple of 8 that both texts reach inside their common prefix, or that both end before
          for (int from = 0; from <= common; from += 8) {
            if (from > 0 && from > lo) break;
            const int got = sign(sort_compare(pa.p, la, pb.p, lb, from));
            if (got != want) {
              printf("FAIL: sort_compare of lengths %d and %d (common prefix %d) from %d: got %d, want %d\n", la, lb, common, from,
                     got, want);
              return 1;
            }
            ++compares;
          }
        }
      }
    }
  }
  printf("ok: sort_word on %ld texts at every depth, %ld sort_compare calls agree with std::lexicographical_compare\n", words, compares);

  std::vector<Text> ties;   // heavy ties over two letters, lengths 0..12
  for (int k = 0; k < 400; ++k) {
    Text t((size_t)(rng() % 13));
    for (auto& c : t) c = (uint8_t)('a' + rng() % 2);
    ties.push_back(t);
  }
  std::vector<Text> shared;   // 80 texts behind one prefix of 100 bytes, some equal, some a prefix of another
  Text prefix(100);
  for (auto& c : prefix) c = (uint8_t)rng();
  for (int k = 0; k < 80; ++k) {
    Text t(prefix);
    const int more = (int)(rng() % 12);
    for (int q = 0; q < more; ++q) t.push_back(edge[rng() % 6]);
    shared.push_back(t);
  }
  std::vector<Text> mixed;   // lengths 0..49, trailing NULs, high bytes, duplicates at distance
  for (int L = 0; L < 50; ++L) {
    Text t((size_t)L);
    for (auto& c : t) c = (uint8_t)('a' + rng() % 4);
    mixed.push_back(t);
    Text nul(t);
    nul.push_back(0);
    mixed.push_back(nul);
  }
  for (uint8_t c : edge) mixed.push_back(Text(1, c));
  for (int k : {0, 3, 16, 17, 33, 64, 99}) mixed.push_back(mixed[(size_t)k]);
  mixed.push_back({});
  for (int k = 0; k < 70; ++k) {   // more than 64 texts that share their first 8 bytes
    Text t = {'s', 'a', 'm', 'e', 'h', 'e', 'a', 'd'};
    t.push_back((uint8_t)(rng() % 3));
    if (k % 2) t.push_back((uint8_t)k);
    mixed.push_back(t);
  }
  if (!check_route(ties, "ties") || !check_route(shared, "shared prefix") || !check_route(mixed, "mixed")) return 1;
  return 0;
}
