// Host check of leftmost and sub of a keyword set (mojo_regex_amd/csrc/mrx_kw_sub_bits.hpp) against the loop of the
// definition, meant for the host sanitizers: no kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/kw_sub_check.cpp -o kw_sub_check && ./kw_sub_check
//
// The reversed build, the walk back, the selection, the rows and the block fill are the ones that the handle and the
// kernels run: kw_build_reversed, and kw_sub_host over the kernels' pieces at the piece sizes 16, 32, 48 and the rule's.
//   - Every text lies at every alignment 0..15 at the END of an allocation of exactly the aligned 16-byte words that hold
//     it, so a read outside the words that the read contract of include/mrx.h allows -- the right-hand warm-up leaving
//     the text, above all -- is the sanitizer's to report; an empty text points behind a buffer.  Everything else in the
//     buffer is the alphabet's bytes in turn: a walk that took them for text would find other matches.
//   - The replacements lie in a buffer of their own words only; the output has exactly the expected number of bytes at an
//     alignment that changes with the text's, inside an allocation of exactly that size.
//   - Entries over {a, b, c} of 1 to 40 bytes (longer than two of the small pieces), with duplicates, prefixes and
//     suffixes of each other; texts of 0 to 100 bytes; the folded form; count 0, 1 and 3; one replacement for all and one
//     per entry of 0 to 70 bytes; the headless text `aaaa...` across 257 pieces.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the headers' host + device qualifiers)

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_kw_sub_bits.hpp"

using namespace mrx;

namespace {

// `bytes` at alignment `skew` inside an allocation of exactly the aligned words that hold them
struct Placed {
  uint8_t* buf;
  const uint8_t* p;
  Placed(const std::string& bytes, int skew) {
    const size_t words = bytes.empty() ? 1 : (skew + bytes.size() + 15) / 16;
    buf = (uint8_t*)aligned_alloc(16, words * 16);
    for (size_t k = 0; k < words * 16; ++k) buf[k] = (uint8_t)("abcABC"[k % 6]);
    if (!bytes.empty()) memcpy(buf + skew, bytes.data(), bytes.size());
    p = bytes.empty() ? buf + words * 16 : buf + skew;
  }
  ~Placed() { free(buf); }
  Placed(const Placed&) = delete;
};

typedef std::tuple<int, int, int> Match;   // entry, start, end

uint8_t fold(uint8_t c, bool on) { return on && c >= 'A' && c <= 'Z' ? (uint8_t)(c | 0x20) : c; }

bool occurs(const std::string& e, const std::string& t, size_t s, bool ic) {
  if (s + e.size() > t.size()) return false;
  for (size_t k = 0; k < e.size(); ++k)
    if (fold((uint8_t)t[s + k], ic) != fold((uint8_t)e[k], ic)) return false;
  return true;
}
bool same(const std::string& a, const std::string& b, bool ic) { return a.size() == b.size() && occurs(a, b, 0, ic); }

std::vector<Match> expected(const std::vector<std::string>& entries, const std::string& t, bool ic, int count) {
  std::vector<Match> out;
  size_t pos = 0;
  while (pos < t.size() && !(count && (int)out.size() == count)) {
    int best = -1;
    size_t s = pos;
    for (; s < t.size() && best < 0; ++s)
      for (size_t j = 0; j < entries.size(); ++j)
        if (occurs(entries[j], t, s, ic) && (best < 0 || entries[j].size() > entries[(size_t)best].size())) best = (int)j;
    if (best < 0) break;
    --s;
    for (size_t j = 0; j < (size_t)best; ++j)   // the lowest index of equal entries
      if (same(entries[j], entries[(size_t)best], ic)) {
        best = (int)j;
        break;
      }
    out.emplace_back(best, (int)s, (int)(s + entries[(size_t)best].size()));
    pos = s + entries[(size_t)best].size();
  }
  return out;
}

long checked = 0, found = 0;

void fail(const char* what, const std::string& text, int skew, int64_t P) {
  printf("%s: text of %zu bytes \"%.120s\" at alignment %d, pieces of %lld\n", what, text.size(), text.c_str(), skew, (long long)P);
  exit(1);
}

void check_set(const std::vector<std::string>& entries, const std::vector<std::string>& texts, bool ic,
               const std::vector<std::string>& repls, int only_skew = -1) {
  std::string data, rdata;
  std::vector<int64_t> off(1, 0), roff(1, 0);
  for (const std::string& e : entries) {
    data += e;
    off.push_back((int64_t)data.size());
  }
  for (const std::string& r : repls) {
    rdata += r;
    roff.push_back((int64_t)rdata.size());
  }
  KwAutomaton A;
  std::string err;
  if (kw_build_reversed((const uint8_t*)data.data(), off.data(), (int64_t)entries.size(), ic ? MRX_KW_IGNORE_CASE : 0, &A, &err) != MRX_OK) {
    printf("build refused %zu entries: %s\n", entries.size(), err.c_str());
    exit(1);
  }
  const Placed rp(rdata, 5);
  const KwRepl R{rp.p, roff.data(), (int64_t)repls.size()};
  for (size_t t = 0; t < texts.size(); ++t) {
    const std::string& text = texts[t];
    const int64_t sizes[4] = {16, 32, 48, kw_piece_rule(A.lmax, (int64_t)text.size())};
    for (int skew = 0; skew < 16; ++skew) {
      if (only_skew >= 0 && skew != only_skew) continue;
      const Placed pl(text, skew);   // the allocation ends with the last aligned word that holds a byte of the text
      const int64_t P = sizes[(skew + t) % 4];
      const int count = (skew % 3 == 0) ? 0 : (skew % 3 == 1 ? 1 : 3);
      const std::vector<Match> want = expected(entries, text, ic, count);
      const int64_t toff[2] = {0, (int64_t)text.size()};
      KwSubHostResult res;
      kw_sub_host(A, P, count, pl.p, toff, 1, false, R, nullptr, 0, (int64_t)want.size(), &res);
      if (res.kb[1] != (int64_t)want.size()) fail("wrong number of matches", text, skew, P);
      for (size_t q = 0; q < want.size(); ++q)
        if (Match(res.entries[q], (int)(uint32_t)res.spans[q], (int)(uint32_t)(res.spans[q] >> 32)) != want[q])
          fail("wrong match", text, skew, P);
      std::string out_want;
      int prev = 0;
      for (const Match& m : want) {
        out_want += text.substr((size_t)prev, (size_t)(std::get<1>(m) - prev));
        out_want += repls[repls.size() == 1 ? 0 : (size_t)std::get<0>(m)];
        prev = std::get<2>(m);
      }
      out_want += text.substr((size_t)prev);
      const size_t room = out_want.size() + (size_t)skew;   // exactly the output, at a moving alignment
      uint8_t* out = (uint8_t*)malloc(room ? room : 1) + skew;
      KwSubHostResult sres;
      kw_sub_host(A, P, count, pl.p, toff, 1, true, R, out, (int64_t)out_want.size(), 0, &sres);
      if (sres.bytes != (int64_t)out_want.size() || sres.out_off[1] != sres.bytes || sres.longest != sres.bytes)
        fail("wrong output size", text, skew, P);
      if (memcmp(out, out_want.data(), out_want.size()) != 0) fail("wrong output bytes", text, skew, P);
      free(out - skew);
      ++checked;
      found += (long)want.size();
    }
  }
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261021);
  auto run = [&](const char* from, int k) {
    std::string s;
    for (int j = 0; j < k; ++j) s += from[rng() % strlen(from)];
    return s;
  };
  check_set({"a", "aa", "aaa", "aaaa"}, {"aaaaaa", "", "a", "baaab"}, false, {"<>"});
  check_set({"ab", "abcd", "bc"}, {"abcabcd", "bcabc", ""}, false, {"1", "four", ""});
  check_set({"He", "sHe", "HE", "hers"}, {"usHErs", "HISHERSHE", "sh"}, true, {"h", "s", "H", "long replacement of over 16 bytes"});
  check_set({}, {"abc", ""}, false, {"x"});
  check_set({"a", "aa", "aaa"}, {std::string(4099, 'a')}, false, {"1", "22", "333"}, 0);   // headless: pieces of 16
  for (int rep = 0; rep < 120; ++rep) {
    const bool ic = rep % 4 == 3;
    const char* al = ic ? "abcABC" : (rep % 2 ? "ab" : "abc");
    std::vector<std::string> texts, entries, repls;
    for (int t = 0; t < 12; ++t) texts.push_back(run(al, (int)(rng() % 101)));
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
    if (rep % 2) {
      repls.push_back(run("XYZ", (int)(rng() % 9)));
    } else {
      for (int j = 0; j < m; ++j) repls.push_back(run("XYZ", (int)(rng() % 71)));
    }
    check_set(entries, texts, ic, repls);
  }
  printf("kw_sub_check ok: %ld texts placed, walked back and rewritten, %ld matches\n", checked, found);
  return 0;
}
