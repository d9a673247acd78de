// Host check of the quoted-fields walk (mojo_regex_amd/csrc/mrx_fields_bits.hpp) against a byte loop with one bit of
// state that knows no words, no groups, no rounds and no mask parities, meant for the host sanitizers: no kernel, no
// HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/fields_quoted_check.cpp -o fields_quoted_check && ./fields_quoted_check
//
// The walk is the one the kernel runs: fields_host_text with a quote, a group of G lanes over the aligned 16-byte words
// of a text in rounds of G, the group's ballot put together lane by lane, for G = 1, 2, 4, 16 and 64.
//   - Every text lies at every alignment 0..15 inside a buffer of exactly the aligned 16-byte words that hold it, so a
//     read outside the words that the read contract of include/mrx.h allows -- the two bytes that decide a part's outer
//     quotes included -- is the sanitizer's to report; an empty text points behind a buffer, where any read is one.
//     Everything else in the buffer is "\", \"q" over and over, an odd number of quotes in front of the text at most
//     alignments: a walk that took it for text would begin inside.
//   - The row is a heap block of exactly f pairs, the quoted bytes one of exactly f bytes.
//   - Texts over {a, b, ',', ' ', '"', \t, x} of 0 to 150 bytes and a few of 2 to 5 KiB, and rows in the shape that a CSV
//     writer gives; both modes, REST, with and without nf (the early stop), generated columns of both signs.
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

constexpr uint8_t kQuote = '"';

struct Placed {
  uint8_t* buf;
  const uint8_t* p;
  Placed(const std::string& bytes, int skew) {
    const size_t words = bytes.empty() ? 1 : (skew + bytes.size() + 15) / 16;
    buf = (uint8_t*)aligned_alloc(16, words * 16);
    for (size_t k = 0; k < words * 16; ++k) buf[k] = (uint8_t)("\", \"q"[k % 5]);
    if (!bytes.empty()) memcpy(buf + skew, bytes.data(), bytes.size());
    p = bytes.empty() ? buf + words * 16 : buf + skew;   // an empty text: nothing may be read at all
  }
  ~Placed() { free(buf); }
  Placed(const Placed&) = delete;
};

bool is_ws(uint8_t c) { return (c >= 9 && c <= 13) || c == 32; }

// the parts of t, byte by byte, with the state outside / inside; maxsplit < 0: no limit
std::vector<std::pair<int, int>> parts_of(const std::string& t, bool ws, uint8_t d, int maxsplit) {
  const int L = (int)t.size();
  std::vector<char> sep((size_t)L, 0);
  bool inside = false;
  for (int i = 0; i < L; ++i) {
    const uint8_t c = (uint8_t)t[(size_t)i];
    if (c == kQuote) inside = !inside;
    else sep[(size_t)i] = !inside && (ws ? is_ws(c) : c == d);
  }
  std::vector<std::pair<int, int>> out;
  int i = 0;
  if (!ws) {
    int start = 0;
    for (; i < L; ++i)
      if (sep[(size_t)i] && (maxsplit < 0 || (int)out.size() < maxsplit)) {
        out.push_back({start, i});
        start = i + 1;
      }
    out.push_back({start, L});
    return out;
  }
  while (true) {
    while (i < L && sep[(size_t)i]) ++i;
    if (i == L) break;
    if (maxsplit >= 0 && (int)out.size() == maxsplit) {
      out.push_back({i, L});
      break;
    }
    const int start = i;
    while (i < L && !sep[(size_t)i]) ++i;
    out.push_back({start, i});
  }
  return out;
}

int failures = 0;

void check(const std::string& t, int skew, int G, uint32_t flags, uint8_t d, const std::vector<int32_t>& cols, bool want_nf,
           bool want_quoted) {
  FieldsPlan P;
  const char* msg = fields_plan(flags, d, cols.data(), (int32_t)cols.size(), want_nf, &P);
  if (!msg) msg = fields_quote_check(flags, d, kQuote);
  if (msg) {
    printf("plan refused: %s\n", msg);
    ++failures;
    return;
  }
  const auto parts = parts_of(t, (flags & MRX_FIELDS_WHITESPACE) != 0, d, (flags & MRX_FIELDS_REST) ? P.cmax - 1 : -1);
  const int nf = (int)parts.size();
  Placed at(t, skew);
  int32_t* row = (int32_t*)malloc(sizeof(int32_t) * 2 * cols.size());
  uint8_t* quoted = (uint8_t*)malloc(cols.size());
  memset(quoted, 0xEE, cols.size());
  int32_t got_nf = -7;
  fields_host_text(P, G, at.p, (int64_t)t.size(), row, want_nf ? &got_nf : nullptr, kQuote, want_quoted ? quoted : nullptr);
  bool ok = !want_nf || got_nf == nf;
  for (size_t j = 0; j < cols.size(); ++j) {
    const int64_t q = cols[j] > 0 ? (int64_t)cols[j] - 1 : (int64_t)nf + cols[j];
    int ws = -1, we = -1, wq = 0;
    if (q >= 0 && q < nf) {
      ws = parts[(size_t)q].first;
      we = parts[(size_t)q].second;
      if (we - ws >= 2 && (uint8_t)t[(size_t)ws] == kQuote && (uint8_t)t[(size_t)we - 1] == kQuote) ++ws, --we, wq = 1;
    }
    if (row[2 * j] != ws || row[2 * j + 1] != we) ok = false;
    if (quoted[j] != (want_quoted ? wq : 0xEE)) ok = false;
  }
  if (!ok && ++failures <= 10) {
    printf("mismatch: len %zu skew %d G %d flags %u nf %d (want %d) cols", t.size(), skew, G, flags, (int)got_nf, nf);
    for (int32_t c : cols) printf(" %d", (int)c);
    printf("\n");
  }
  free(quoted);
  free(row);
}

}  // namespace

int main() {
  // the prefix-xor and the inside mask against a loop over the bits
  for (uint32_t q = 0; q < 0x10000u; ++q)
    for (uint32_t parity = 0; parity < 2; ++parity) {
      uint32_t want = 0, state = parity;
      for (int k = 0; k < 16; ++k) {
        state ^= (q >> k) & 1u;
        want |= state << k;
      }
      if (fields_inside(q, parity) != want) ++failures;
    }
  // the group's share of a ballot and its parities
  for (int G = 1; G <= 64; G <<= 1)
    for (int t = 0; t < 64 / G; ++t)
      for (uint64_t ballot : {0x0123456789abcdefull, ~0ull, 0x8000000000000001ull, 0xf0f0f0f00f0f0f0full}) {
        const uint64_t bits = fields_group_bits(ballot, t, G);
        uint32_t front = 0;
        for (int l = 0; l < G; ++l) {
          if (fields_parity_front(bits, l) != front) ++failures;
          front ^= (uint32_t)(ballot >> (t * G + l)) & 1u;
        }
        if (fields_parity_all(bits) != front) ++failures;
      }
  std::mt19937 rng(20260101);
  const char alphabet[] = {'a', 'b', ',', ',', ' ', '"', '"', '\t', 'x'};
  auto text = [&](int len) {
    std::string t((size_t)len, 'a');
    for (auto& c : t) c = alphabet[rng() % sizeof(alphabet)];
    return t;
  };
  // rows in a CSV writer's shape: cells over ab," x, quoted when they need it or always, inner quotes doubled
  auto csv_row = [&](bool all) {
    std::string t;
    const int cells = 1 + (int)(rng() % 6);
    for (int c = 0; c < cells; ++c) {
      std::string cell((size_t)(rng() % 7), 'a');
      for (auto& ch : cell) ch = "ab,\" x"[rng() % 6];
      if (c) t += ',';
      if (all || cell.find_first_of(",\"") != std::string::npos || (cells == 1 && cell.empty())) {
        t += '"';
        for (char ch : cell) {
          if (ch == '"') t += '"';
          t += ch;
        }
        t += '"';
      } else {
        t += cell;
      }
    }
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
    const std::string t = rep % 17 == 3   ? std::string((size_t)len, '"')
                          : rep % 17 == 4 ? csv_row(false)
                          : rep % 17 == 5 ? csv_row(true)
                          : rep % 17 == 6 ? "\"" + text(len) + "\""
                                          : text(len);
    const int hint = (int)t.size() / 4 + 1;
    for (int skew = 0; skew < 16; ++skew) {
      if (t.size() > 1024 && skew % 5) continue;   // the long ones at skews 0, 5, 10, 15
      for (int G : groups)
        for (uint32_t mode = 0; mode < 2; ++mode) {
          check(t, skew, G, mode, ',', columns(true, hint), true, true);
          check(t, skew, G, mode, ',', columns(false, hint), false, rep % 2 == 0);                // the early stop
          check(t, skew, G, mode | MRX_FIELDS_REST, ',', columns(false, hint), true, true);       // REST stops early with nf too
          check(t, skew, G, mode, ',', {-1, 1000, 2, 1, 2}, true, false);
          cases += 4;
        }
    }
  }
  // f = 32
  std::vector<int32_t> wide(32);
  for (int j = 0; j < 32; ++j) wide[(size_t)j] = j % 2 ? -(j / 2 + 1) : j / 2 + 1;
  for (int rep = 0; rep < 50; ++rep)
    for (int G : groups) check(text(100 + rep), rep % 16, G, rep % 2, ',', wide, true, true);
  if (failures) {
    printf("fields_quoted_check: %d failures\n", failures);
    return 1;
  }
  printf("fields_quoted_check ok: %lld cases\n", (long long)cases);
  return 0;
}
