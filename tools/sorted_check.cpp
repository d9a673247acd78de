// Host check of the sorted index's searches (mojo_regex_amd/csrc/mrx_sorted_bits.hpp) against std::lower_bound /
// std::upper_bound with std::lexicographical_compare and a brute-force longest prefix, meant for the host sanitizers: no
// kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/sorted_check.cpp -o sorted_check && ./sorted_check
//
// The sorted entries lie packed, at every alignment 0..15, in a buffer of exactly the aligned 16-byte words that hold
// them, and every probe at some alignment in such a buffer of its own, so a read outside the words that the read
// contract of include/mrx.h allows is the sanitizer's to report; what is left of the buffers is poison (zero bytes, 0xFF),
// which a missing mask would turn into a wrong answer.  All three modes run in every form of the search: the plain binary
// search over the bytes, with the key array, and with fence posts above it at the handle's step and at steps of 1, 3 and
// 64 (so that small indexes have several posts).
//   - entries over the alphabet {a, b, \0} with lengths 0..12: duplicates, prefixes, trailing NULs, the empty entry;
//   - entries of 24 bytes whose first difference lies at byte 7, 8, 9, 15, 16, 17, and their cuts at those lengths;
//   - a run of more than 64 entries with equal first 8 bytes, some equal, some a prefix of another;
//   - 300 entries behind one prefix of 100 bytes;
//   - an empty index.
// Probes: every entry, every entry with its last byte changed, dropped, and with \0 appended, every prefix of some, the
// empty text.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the headers' host + device qualifiers)

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_sorted_bits.hpp"

using namespace mrx;

namespace {

using Text = std::vector<uint8_t>;

bool text_less(const Text& a, const Text& b) { return std::lexicographical_compare(a.begin(), a.end(), b.begin(), b.end()); }
bool starts_with(const Text& e, const Text& p) { return e.size() >= p.size() && std::equal(p.begin(), p.end(), e.begin()); }

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

long g_probes = 0;

// the three modes of one probe in one form of the view, against the plain C++ answers
bool check_probe(const SortedView& V, const char* form, const std::vector<Text>& sorted, const Text& probe, int skew) {
  const Placed at(probe, skew, skew % 2 ? 0xFF : 0x00);
  const int64_t want_lo = std::lower_bound(sorted.begin(), sorted.end(), probe, text_less) - sorted.begin();
  const int64_t want_hi = std::upper_bound(sorted.begin(), sorted.end(), probe, text_less) - sorted.begin();
  int64_t plo = want_lo, phi = want_lo, best = -1, best_len = -1;
  bool any = false;
  for (size_t j = 0; j < sorted.size(); ++j) {
    if (starts_with(sorted[j], probe)) {
      if (!any) plo = (int64_t)j;
      any = true;
      phi = (int64_t)j + 1;
    }
    if (starts_with(probe, sorted[j]) && (int64_t)sorted[j].size() > best_len) {
      best = (int64_t)j;
      best_len = (int64_t)sorted[j].size();
    }
  }
  const int64_t want[3][2] = {{want_lo, want_hi}, {plo, phi}, {best, best_len}};
  for (uint32_t mode = 0; mode < 3; ++mode) {
    int64_t lo = -7, hi = -7;
    sorted_search_one(V, mode, at.p, at.L, &lo, &hi);
    ++g_probes;
    if (lo != want[mode][0] || hi != want[mode][1]) {
      printf("FAIL: %s, mode %u, probe of %zu bytes at skew %d over %zu entries: got %lld, %lld, want %lld, %lld\n", form, mode,
             probe.size(), skew, sorted.size(), (long long)lo, (long long)hi, (long long)want[mode][0], (long long)want[mode][1]);
      return false;
    }
  }
  return true;
}

bool check_index(std::vector<Text> entries, const char* what, std::mt19937& rng) {
  std::stable_sort(entries.begin(), entries.end(), text_less);
  const int64_t m = (int64_t)entries.size();
  std::vector<Text> probes = entries;
  for (const Text& e : entries) {
    if (!e.empty()) {
      Text t(e);
      t.back() ^= (uint8_t)(1u << (rng() % 8));
      probes.push_back(t);
      probes.push_back(Text(e.begin(), e.end() - 1));
    }
    Text nul(e);
    nul.push_back(0);
    probes.push_back(nul);
    Text more(e);
    more.push_back((uint8_t)rng());
    more.push_back('b');
    probes.push_back(more);
  }
  for (size_t j = 0; j < entries.size(); j += 5)
    for (size_t k = 0; k <= entries[j].size(); ++k) probes.push_back(Text(entries[j].begin(), entries[j].begin() + k));
  probes.push_back({});
  probes.push_back({0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff});
  if (probes.size() > 3000) {   // (quadratic against the brute force: a sample of the probes is enough)
    std::shuffle(probes.begin() + 1, probes.end(), rng);
    probes.resize(3000);
  }
  for (int skew = 0; skew < 16; ++skew) {
    std::vector<int64_t> offsets(m + 1, 0);
    Text packed;
    for (int64_t j = 0; j < m; ++j) {
      packed.insert(packed.end(), entries[j].begin(), entries[j].end());
      offsets[j + 1] = (int64_t)packed.size();
    }
    const Placed data(packed, skew, skew % 2 ? 0x00 : 0xFF);
    std::vector<uint64_t> keys(m + 1);
    std::vector<uint8_t> valids(m + 1);
    const SortedView plain{data.p, offsets.data(), m, nullptr, nullptr, nullptr, nullptr, 1, 0};
    for (int64_t j = 0; j < m; ++j) {
      int64_t L;
      const uint8_t* e = sorted_entry(plain, j, &L);
      int valid;
      keys[j] = sort_word(e, L, 0, &valid);
      valids[j] = (uint8_t)valid;
    }
    SortedView keyed = plain;
    keyed.keys = keys.data();
    keyed.valids = valids.data();
    for (size_t q = (size_t)skew % 3; q < probes.size(); q += 3) {   // (a third of the probes per alignment, all of them in 3)
      const int ps = (int)((q * 7 + skew) % 16);
      if (!check_probe(plain, "bytes", entries, probes[q], ps) || !check_probe(keyed, "keys", entries, probes[q], ps)) return false;
    }
    for (int64_t step : {sorted_fence_step(m), (int64_t)1, (int64_t)3, (int64_t)64}) {
      if (m == 0 || (m + step - 1) / step > kSortedFence) continue;
      std::vector<uint64_t> fkey;
      std::vector<uint8_t> fvalid;
      for (int64_t j = 0; j < m; j += step) {
        fkey.push_back(keys[j]);
        fvalid.push_back(valids[j]);
      }
      SortedView fenced = keyed;
      fenced.fkey = fkey.data();
      fenced.fvalid = fvalid.data();
      fenced.fstep = step;
      fenced.fcount = (int)fkey.size();
      for (size_t q = (size_t)(skew + step) % 4; q < probes.size(); q += 4)
        if (!check_probe(fenced, "fence", entries, probes[q], (int)((q * 3 + skew) % 16))) return false;
    }
  }
  printf("ok: %s: %lld entries, %zu probes\n", what, (long long)m, probes.size());
  return true;
}

}  // namespace

int main() {
  std::mt19937 rng(20261021);
  // the comparison by itself: sign, depth and truncation on every pair of lengths 0..26 around a first difference
  long compares = 0;
  for (int la = 0; la <= 26; ++la)
    for (int lb = 0; lb <= 26; ++lb)
      for (int c = 0; c <= std::min(la, lb); ++c) {
        Text a((size_t)la), b((size_t)lb);
        for (int k = 0; k < la; ++k) a[(size_t)k] = (k % 5 == 4) ? 0 : (uint8_t)rng();
        for (int k = 0; k < lb; ++k) b[(size_t)k] = k < c ? a[(size_t)k] : (uint8_t)(rng() % 2 ? 0x00 : 0x80);
        if (c < la && c < lb && a[(size_t)c] == b[(size_t)c]) a[(size_t)c] ^= 0x40;
        const Placed pa(a, (la + 3 * c) % 16, 0xFF), pb(b, (lb * 5 + c) % 16, 0x00);
        const int want = text_less(a, b) ? -1 : text_less(b, a) ? 1 : 0;
        const Text cut(a.begin(), a.begin() + std::min(la, lb));
        const int want_cut = text_less(cut, b) ? -1 : text_less(b, cut) ? 1 : 0;
        const int64_t common = c;   // (both texts have c bytes and agree on them; byte c differs or one text ends)
        for (int64_t from = 0; from <= common; from += 8) {
          int64_t depth = -1, depth_cut = -1;
          const int got = sorted_compare_depth(pa.p, la, pb.p, lb, from, &depth);
          const int got_cut = sorted_compare_trunc(pa.p, la, pb.p, lb, from, &depth_cut);
          const int64_t want_depth = want == 0 ? (la / 8) * 8 : (common / 8) * 8;
          if (got != want || got_cut != want_cut || depth != want_depth || depth_cut % 8 || depth_cut > common ||
              sorted_lcp(pa.p, la, pb.p, lb) != common) {
            printf("FAIL: comparison of lengths %d and %d (common prefix %d) from %lld: %d / %d at depth %lld / %lld, want %d / %d at %lld\n",
                   la, lb, c, (long long)from, got, got_cut, (long long)depth, (long long)depth_cut, want, want_cut, (long long)want_depth);
            return 1;
          }
          ++compares;
        }
      }
  printf("ok: %ld comparisons agree with std::lexicographical_compare in sign, depth and common prefix\n", compares);

  std::vector<Text> small;   // {a, b, \0}, lengths 0..12
  for (int k = 0; k < 500; ++k) {
    Text t((size_t)(rng() % 13));
    for (auto& c : t) c = (uint8_t)("ab\0"[rng() % 3]);
    small.push_back(t);
  }
  std::vector<Text> firsts;   // first differences at bytes 7, 8, 9, 15, 16, 17, and the cuts at those lengths
  Text base(24);
  for (auto& c : base) c = (uint8_t)('c' + rng() % 20);
  firsts.push_back(base);
  for (int at : {7, 8, 9, 15, 16, 17}) {
    for (uint8_t v : {(uint8_t)0x00, (uint8_t)0x7f, (uint8_t)0x80, (uint8_t)0xff}) {
      Text t(base);
      t[(size_t)at] = v;
      firsts.push_back(t);
    }
    firsts.push_back(Text(base.begin(), base.begin() + at));
    Text nul(base.begin(), base.begin() + at);
    nul.push_back(0);
    firsts.push_back(nul);
    nul.push_back(0);
    firsts.push_back(nul);
  }
  std::vector<Text> run;   // more than 64 entries with equal first 8 bytes, among others
  for (int k = 0; k < 150; ++k) {
    Text t = {'s', 'a', 'm', 'e', 'h', 'e', 'a', 'd'};
    const int more = (int)(rng() % 5);
    for (int q = 0; q < more; ++q) t.push_back((uint8_t)("xy\0"[rng() % 3]));
    run.push_back(t);
  }
  for (int k = 0; k < 40; ++k) run.push_back(Text{'s', 'a', 'm', 'e', 'h', 'e', 'a', (uint8_t)('a' + k % 8)});
  run.push_back(Text{'s', 'a', 'm', 'e'});
  std::vector<Text> shared;   // 300 entries behind one prefix of 100 bytes
  Text prefix(100);
  for (auto& c : prefix) c = (uint8_t)rng();
  for (int k = 0; k < 300; ++k) {
    Text t(prefix);
    const int more = (int)(rng() % 10);
    for (int q = 0; q < more; ++q) t.push_back((uint8_t)("pq\0\xff"[rng() % 4]));
    shared.push_back(t);
  }
  std::vector<Text> many;   // more entries than fence posts: a step of 3
  for (int k = 0; k < 2500; ++k) {
    Text t((size_t)(rng() % 11));
    for (auto& c : t) c = (uint8_t)('a' + rng() % 3);
    many.push_back(t);
  }
  if (!check_index({}, "empty index", rng) || !check_index(small, "three letters", rng) ||
      !check_index(firsts, "first differences", rng) || !check_index(run, "equal first words", rng) ||
      !check_index(shared, "shared prefix", rng) || !check_index(many, "2500 entries", rng))
    return 1;
  printf("ok: %ld searches agree with std::lower_bound, std::upper_bound and the brute force\n", g_probes);
  return 0;
}
