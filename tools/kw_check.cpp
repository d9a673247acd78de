// Host check of the keyword automaton and its walk (mojo_regex_amd/csrc/mrx_kw_bits.hpp) against a search that knows no
// automaton, meant for the host sanitizers: no kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/kw_check.cpp -o kw_check && ./kw_check
//
// The build and the walk are the ones that mrx_kw_build and the kernels run: kw_build, and kw_host_findall over the
// kernels' pieces at the piece sizes 16, 32, 48 and the rule's.
//   - Every text lies at every alignment 0..15 inside a buffer of exactly the aligned 16-byte words that hold it, so a
//     read outside the words that the read contract of include/mrx.h allows is the sanitizer's to report; an empty text
//     points behind a buffer, where any read is one.  Everything else in the buffer is the alphabet's bytes in turn
//     ('a', 'b', 'c', ...): a walk that took them for text would find other hits.
//   - The outputs have exactly the expected number of rows and a canary row on either side.
//   - Entries over {a, b, c} of 1 to 40 bytes (longer than two of the small pieces), with duplicates, prefixes and
//     suffixes of each other; texts of 0 to 100 bytes; the folded form with mixed case on both sides; every byte value
//     as an entry at once (256 classes, none left for the rest); no entry at all.
//   - The refusals: an empty entry names its index, a table above the limit gives states and classes.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the headers' host + device qualifiers)

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_kw_bits.hpp"

using namespace mrx;

namespace {

struct Placed {
  uint8_t* buf;
  const uint8_t* p;
  Placed(const std::string& bytes, int skew) {
    const size_t words = bytes.empty() ? 1 : (skew + bytes.size() + 15) / 16;
    buf = (uint8_t*)aligned_alloc(16, words * 16);
    for (size_t k = 0; k < words * 16; ++k) buf[k] = (uint8_t)("abcABC"[k % 6]);
    if (!bytes.empty()) memcpy(buf + skew, bytes.data(), bytes.size());
    p = bytes.empty() ? buf + words * 16 : buf + skew;   // an empty text: nothing may be read at all
  }
  ~Placed() { free(buf); }
  Placed(const Placed&) = delete;
};

typedef std::tuple<int, int, int> Hit;   // end, start, entry: sorted as the contract orders a text's hits

uint8_t fold(uint8_t c, bool on) { return on && c >= 'A' && c <= 'Z' ? (uint8_t)(c | 0x20) : c; }

std::vector<Hit> expected(const std::vector<std::string>& entries, const std::string& text, bool ic) {
  std::vector<Hit> hits;
  for (size_t j = 0; j < entries.size(); ++j) {
    bool first = true;   // the lowest index of equal entries stands for them
    for (size_t i = 0; i < j && first; ++i) {
      if (entries[i].size() != entries[j].size()) continue;
      bool same = true;
      for (size_t k = 0; k < entries[j].size() && same; ++k) same = fold(entries[i][k], ic) == fold(entries[j][k], ic);
      first = !same;
    }
    if (!first) continue;
    const std::string& e = entries[j];
    for (size_t s = 0; s + e.size() <= text.size(); ++s) {
      bool at = true;
      for (size_t k = 0; k < e.size() && at; ++k) at = fold(text[s + k], ic) == fold(e[k], ic);
      if (at) hits.emplace_back((int)(s + e.size()), (int)s, (int)j);
    }
  }
  std::sort(hits.begin(), hits.end());
  return hits;
}

long checked = 0, found = 0;

void fail(const char* what, const std::string& text, int skew, int64_t P) {
  printf("%s: text of %zu bytes \"%s\" at alignment %d, pieces of %lld\n", what, text.size(), text.c_str(), skew, (long long)P);
  exit(1);
}

void check_set(const std::vector<std::string>& entries, const std::vector<std::string>& texts, bool ic) {
  std::string data;
  std::vector<int64_t> off(1, 0);
  for (const std::string& e : entries) {
    data += e;
    off.push_back((int64_t)data.size());
  }
  KwAutomaton A;
  std::string err;
  const int rc = kw_build((const uint8_t*)data.data(), off.data(), (int64_t)entries.size(), ic ? MRX_KW_IGNORE_CASE : 0, &A, &err);
  if (rc != MRX_OK) {
    printf("build refused %zu entries: %s\n", entries.size(), err.c_str());
    exit(1);
  }
  for (size_t t = 0; t < texts.size(); ++t) {
    const std::string& text = texts[t];
    const std::vector<Hit> want = expected(entries, text, ic);
    const int64_t sizes[4] = {16, 32, 48, kw_piece_rule(A.lmax, (int64_t)text.size())};
    for (int skew = 0; skew < 16; ++skew) {
      const Placed pl(text, skew);
      const int64_t P = sizes[(skew + t) % 4];
      const int64_t toff[2] = {0, (int64_t)text.size()};
      int64_t prefix[2] = {-1, -1};
      const size_t rows = want.size();
      std::vector<int32_t> ents(rows + 2, -9), spans(2 * (rows + 2), -9);   // a canary row in front and behind
      const int64_t tot = kw_host_findall(A, P, pl.p, toff, 1, prefix, ents.data() + 1, spans.data() + 2, (int64_t)rows);
      if (tot != (int64_t)rows || prefix[0] != 0 || prefix[1] != tot) fail("wrong number of hits", text, skew, P);
      if (ents[0] != -9 || ents[rows + 1] != -9 || spans[0] != -9 || spans[1] != -9 || spans[2 * rows + 2] != -9 ||
          spans[2 * rows + 3] != -9)
        fail("a canary row was written", text, skew, P);
      for (size_t q = 0; q < rows; ++q)
        if (Hit(spans[2 * q + 3], spans[2 * q + 2], ents[q + 1]) != want[q]) fail("wrong hit", text, skew, P);
      ++checked;
      found += (long)rows;
    }
  }
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261020);
  auto run = [&](const char* from, int k) {
    std::string s;
    for (int j = 0; j < k; ++j) s += from[rng() % strlen(from)];
    return s;
  };
  check_set({"a", "aa", "aaa", "aaaa"}, {"aaaaaa", "", "a", "baaab"}, false);
  check_set({"he", "she", "his", "hers"}, {"ushers", "hishershe", "sh", ""}, false);
  check_set({"He", "sHe", "HE", "hers"}, {"usHErs", "HISHERSHE", "sh"}, true);
  check_set({}, {"abc", ""}, false);
  for (int rep = 0; rep < 120; ++rep) {
    const bool ic = rep % 4 == 3;
    const char* al = ic ? "abcABC" : "abc";
    std::vector<std::string> texts, entries;
    for (int t = 0; t < 24; ++t) texts.push_back(run(al, (int)(rng() % 101)));
    const int m = 1 + (int)(rng() % 20);
    while ((int)entries.size() < m) {
      std::string e;
      const int kind = (int)(rng() % 6);
      if (kind == 0 && !entries.empty()) {
        e = entries[rng() % entries.size()];
      } else if (kind == 1 && !entries.empty()) {
        e = entries[rng() % entries.size()];
        e = e.substr(rng() % e.size());
      } else if (kind == 2 && !entries.empty()) {
        e = entries[rng() % entries.size()];
        e = e.substr(0, 1 + rng() % e.size());
      } else if (kind == 3) {
        const std::string& t = texts[rng() % texts.size()];
        if (!t.empty()) e = t.substr(rng() % t.size(), 1 + rng() % 40);
      } else {
        e = run(al, 1 + (int)(rng() % (rng() % 2 ? 4 : 40)));
      }
      if (!e.empty()) entries.push_back(e);
    }
    check_set(entries, texts, ic);
  }
  {   // every byte value is an entry: 256 classes; and the bytes 0x00 and 0xff inside longer entries
    std::vector<std::string> entries;
    for (int c = 0; c < 256; ++c) entries.push_back(std::string(1, (char)c));
    entries.push_back(std::string("\0\xff\0", 3));
    entries.push_back(std::string("\xff\xff", 2));
    std::string all;
    for (int c = 0; c < 256; ++c) all += (char)c;
    check_set(entries, {all, std::string("\0\xff\0\xff\xff\0", 6), std::string(40, '\xff')}, false);
  }
  {   // the refusals
    KwAutomaton A;
    std::string err;
    const int64_t off3[4] = {0, 2, 2, 3};
    if (kw_build((const uint8_t*)"abc", off3, 3, 0, &A, &err) != MRX_E_ARGUMENT || err.find("entry 1 is empty") == std::string::npos) {
      printf("an empty entry was not refused: %s\n", err.c_str());
      return 1;
    }
    const int64_t m = 300, L = 200000;   // 6e7 states x 5 classes x 4 bytes
    std::string big((size_t)(m * L), 'a');
    std::vector<int64_t> off((size_t)m + 1);
    for (int64_t j = 0; j <= m; ++j) off[(size_t)j] = j * L;
    for (int64_t j = 0; j < m; ++j)   // different in their first six bytes
      for (int64_t k = 0, d = j; k < 6; ++k, d /= 3) big[(size_t)(j * L + k)] = "bcd"[d % 3];
    err.clear();
    if (kw_build((const uint8_t*)big.data(), off.data(), m, 0, &A, &err) != MRX_E_UNSUPPORTED ||
        err.find("states x 5 classes") == std::string::npos) {
      printf("a table above the limit was not refused: %s\n", err.c_str());
      return 1;
    }
  }
  printf("kw_check ok: %ld texts placed and walked, %ld hits\n", checked, found);
  return 0;
}
