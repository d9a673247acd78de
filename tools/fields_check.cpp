// Host check of the fields walk (mojo_regex_amd/csrc/mrx_fields_bits.hpp) against a byte loop that knows no words, no
// groups and no rounds, meant for the host sanitizers: no kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/fields_check.cpp -o fields_check && ./fields_check
//
// The walk is the one the kernel runs: fields_host_text, a group of G lanes over the aligned 16-byte words of a text in
// rounds of G, for G = 1, 2, 4, 16 and 64.
//   - Every text lies at every alignment 0..15 inside a buffer of exactly the aligned 16-byte words that hold it, so a
//     read outside the words that the read contract of include/mrx.h allows is the sanitizer's to report; an empty text
//     points behind a buffer, where any read is one.  Everything else in the buffer is ", \tq": a walk that took it for
//     text would find other fields.
//   - The row is a heap block of exactly f pairs.
//   - Texts over {a, b, ',', ' ', \t, \n, 1} of 0 to 150 bytes and a few of 2 to 5 KiB; both modes, REST, with and without
//     nf (the early stop), generated columns of both signs.  The whitespace mask on all 256 byte values against the six
//     bytes of the contract.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the headers' host + device qualifiers)

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_fields_bits.hpp"

using namespace mrx;

namespace {

struct Placed {
  uint8_t* buf;
  const uint8_t* p;
  Placed(const std::string& bytes, int skew) {
    const size_t words = bytes.empty() ? 1 : (skew + bytes.size() + 15) / 16;
    buf = (uint8_t*)aligned_alloc(16, words * 16);
    for (size_t k = 0; k < words * 16; ++k) buf[k] = (uint8_t)(", \tq"[k % 4]);
    if (!bytes.empty()) memcpy(buf + skew, bytes.data(), bytes.size());
    p = bytes.empty() ? buf + words * 16 : buf + skew;   // an empty text: nothing may be read at all
  }
  ~Placed() { free(buf); }
  Placed(const Placed&) = delete;
};

bool is_ws(uint8_t c) { return (c >= 9 && c <= 13) || c == 32; }

// the parts of t, byte by byte: split(d, maxsplit) / split(None, maxsplit) of Python bytes (maxsplit < 0: no limit)
std::vector<std::pair<int, int>> parts_of(const std::string& t, bool ws, uint8_t d, int maxsplit) {
  std::vector<std::pair<int, int>> out;
  const int L = (int)t.size();
  int i = 0;
  if (!ws) {
    int start = 0;
    for (; i < L; ++i)
      if ((uint8_t)t[i] == d && (maxsplit < 0 || (int)out.size() < maxsplit)) {
        out.push_back({start, i});
        start = i + 1;
      }
    out.push_back({start, L});
    return out;
  }
  while (true) {
    while (i < L && is_ws((uint8_t)t[i])) ++i;
    if (i == L) break;
    if (maxsplit >= 0 && (int)out.size() == maxsplit) {
      out.push_back({i, L});
      break;
    }
    const int start = i;
    while (i < L && !is_ws((uint8_t)t[i])) ++i;
    out.push_back({start, i});
  }
  return out;
}

int failures = 0;

void check(const std::string& t, int skew, int G, uint32_t flags, uint8_t d, const std::vector<int32_t>& cols, bool want_nf) {
  FieldsPlan P;
  const char* msg = fields_plan(flags, d, cols.data(), (int32_t)cols.size(), want_nf, &P);
  if (msg) {
    printf("plan refused: %s\n", msg);
    ++failures;
    return;
  }
  const auto parts = parts_of(t, (flags & MRX_FIELDS_WHITESPACE) != 0, d, (flags & MRX_FIELDS_REST) ? P.cmax - 1 : -1);
  const int nf = (int)parts.size();
  Placed at(t, skew);
  int32_t* row = (int32_t*)malloc(sizeof(int32_t) * 2 * cols.size());
  int32_t got_nf = -7;
  fields_host_text(P, G, at.p, (int64_t)t.size(), row, want_nf ? &got_nf : nullptr);
  bool ok = !want_nf || got_nf == nf;
  for (size_t j = 0; j < cols.size(); ++j) {
    const int64_t q = cols[j] > 0 ? (int64_t)cols[j] - 1 : (int64_t)nf + cols[j];
    const int ws = q >= 0 && q < nf ? parts[(size_t)q].first : -1, we = q >= 0 && q < nf ? parts[(size_t)q].second : -1;
    if (row[2 * j] != ws || row[2 * j + 1] != we) ok = false;
  }
  if (!ok && ++failures <= 10) {
    printf("mismatch: len %zu skew %d G %d flags %u nf %d (want %d) cols", t.size(), skew, G, flags, (int)got_nf, nf);
    for (int32_t c : cols) printf(" %d", (int)c);
    printf("\n");
  }
  free(row);
}

}  // namespace

int main() {
  // the whitespace mask, every byte value at every position of a word
  for (int v = 0; v < 256; ++v)
    for (int k = 0; k < 16; ++k) {
      // (the other bytes: one 'q', one 0xFF and zeros, none of them whitespace)
      const g_u128 word = (g_u128)(uint8_t)v << (8 * k) | ((g_u128)'q' << (8 * ((k + 1) & 15))) | ((g_u128)0xff << (8 * ((k + 2) & 15)));
      const uint32_t m = fields_ws16(word);
      if (m != (is_ws((uint8_t)v) ? 1u << k : 0u)) {
        printf("whitespace mask: byte %d at %d gives %x\n", v, k, m);
        ++failures;
      }
    }
  // the k-th set bit
  for (uint32_t m = 1; m < 0x10000u; m += 7)
    for (int r = 0, k = 0; k < 16; ++k)
      if ((m >> k) & 1u) {
        if (fields_kth(m, r) != k) ++failures;
        ++r;
      }
  std::mt19937 rng(20260101);
  const char alphabet[] = {'a', 'b', ',', ',', ' ', ' ', '\t', '\n', '1'};
  auto text = [&](int len) {
    std::string t((size_t)len, 'a');
    for (auto& c : t) c = alphabet[rng() % sizeof(alphabet)];
    return t;
  };
  auto columns = [&](bool negatives, int nf_hint) {
    std::vector<int32_t> cols(1 + rng() % 5);
    for (auto& c : cols) {
      c = 1 + (int32_t)(rng() % (unsigned)(nf_hint + 3));
      if (negatives && rng() % 2) c = -c;
    }
    return cols;
  };
  const int groups[] = {1, 2, 4, 16, 64};
  int64_t cases = 0;
  for (int rep = 0; rep < 1200; ++rep) {
    const int len = rep < 40 ? rep : rep % 50 == 0 ? 2048 + (int)(rng() % 3072) : (int)(rng() % 151);
    const std::string t = rep % 17 == 3 ? std::string((size_t)len, ',') : rep % 17 == 4 ? std::string((size_t)len, ' ') : text(len);
    const int skew = rep < 64 ? rep % 16 : (int)(rng() % 16);
    for (int G : groups)
      for (uint32_t mode = 0; mode < 2; ++mode) {
        const int hint = len / 3 + 1;
        check(t, skew, G, mode, ',', columns(true, hint), true);
        check(t, skew, G, mode, ',', columns(true, hint), false);
        check(t, skew, G, mode, ',', columns(false, hint), false);                    // the early stop
        check(t, skew, G, mode | MRX_FIELDS_REST, ',', columns(false, hint), true);   // REST stops early with nf too
        check(t, skew, G, mode | MRX_FIELDS_REST, ',', columns(false, 2), false);
        check(t, skew, G, mode, ',', {1}, false);
        check(t, skew, G, mode, ',', {-1, 1000, 2, 1, 2}, true);
        cases += 7;
      }
  }
  // f = 32
  std::vector<int32_t> wide(32);
  for (int j = 0; j < 32; ++j) wide[(size_t)j] = j % 2 ? -(j / 2 + 1) : j / 2 + 1;
  for (int rep = 0; rep < 50; ++rep)
    for (int G : groups) check(text(100 + rep), rep % 16, G, rep % 2, ',', wide, true);
  if (failures) {
    printf("fields_check: %d failures\n", failures);
    return 1;
  }
  printf("fields_check ok: %lld cases\n", (long long)cases);
  return 0;
}
