// Host check of the translate and strip walks (mojo_regex_amd/csrc/mrx_translate_bits.hpp) against loops that go byte
// by byte and know no blocks and no pieces, meant for the host sanitizers: no kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/translate_check.cpp -o translate_check && ./translate_check
//
// The walks are the ones the kernels run: tr_block per aligned 16-byte block and translate_host over the kernels'
// pieces and passes, at the piece sizes 16, 32, 48 and 1024; tr_map_block per aligned block of the output region; and
// strip_text per text.
//   - Every batch lies at every alignment 0..15 inside a buffer of exactly the aligned 16-byte words that hold it, so a
//     read outside the words that the read contract of include/mrx.h allows is the sanitizer's to report; an empty batch
//     points behind a buffer, where any read is one.  Everything else in the buffer is " \r": members of the sets.
//   - The outputs are heap blocks of exactly the expected sizes, the same-length form's at every alignment too: a write
//     past the bytes is the sanitizer's to report.  With a capacity one short, nothing at all may be written.
//   - Texts over a small alphabet of set members and letters, of 0 to 150 bytes, alone and as batches of 1 to 6 with
//     empty ones among them, and a few long ones: several rounds of the largest piece.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the headers' host + device qualifiers)

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_translate_bits.hpp"

using namespace mrx;

namespace {

struct Placed {
  uint8_t* buf;
  const uint8_t* p;
  Placed(const std::string& bytes, int skew) {
    const size_t words = bytes.empty() ? 1 : (skew + bytes.size() + 15) / 16;
    buf = (uint8_t*)aligned_alloc(16, words * 16);
    for (size_t k = 0; k < words * 16; ++k) buf[k] = (uint8_t)(" \r"[k % 2]);
    if (!bytes.empty()) memcpy(buf + skew, bytes.data(), bytes.size());
    p = bytes.empty() ? buf + words * 16 : buf + skew;   // an empty batch: nothing may be read at all
  }
  ~Placed() { free(buf); }
  Placed(const Placed&) = delete;
};

struct Set {
  uint8_t bits[32];
  explicit Set(const std::string& members) {
    memset(bits, 0, sizeof bits);
    for (unsigned char c : members) bits[c >> 3] |= (uint8_t)(1u << (c & 7));
  }
  bool has(unsigned char c) const { return (bits[c >> 3] >> (c & 7)) & 1; }
  bool empty() const { return !tr_any(bits); }
};

// one call's options: table (empty string: none), delete, squeeze
struct Options {
  std::string table, del, sq;
};

long checked = 0, moved = 0;

void fail(const char* what, const std::vector<std::string>& texts, int skew, int64_t P) {
  printf("%s: %zu texts, the first of %zu bytes, at alignment %d, pieces of %lld\n", what, texts.size(),
         texts.empty() ? (size_t)0 : texts[0].size(), skew, (long long)P);
  exit(1);
}

// exact-size heap blocks, filled with a pattern
template <class T>
struct Block {
  T* p;
  size_t n;
  explicit Block(size_t count) : p((T*)malloc(count ? count * sizeof(T) : 1)), n(count) { memset(p, 0xEE, count * sizeof(T)); }
  ~Block() { free(p); }
  bool untouched() const {
    for (size_t k = 0; k < n * sizeof(T); ++k)
      if (((const uint8_t*)p)[k] != 0xEE) return false;
    return true;
  }
};

std::string translate_one(const std::string& t, const Options& o) {
  const Set del(o.del), sq(o.sq);
  std::string u;
  for (unsigned char c : t) {
    if (del.has(c)) continue;
    const unsigned char m = o.table.empty() ? c : (unsigned char)o.table[c];
    if (!u.empty() && sq.has(m) && (unsigned char)u.back() == m) continue;
    u += (char)m;
  }
  return u;
}

void check_translate(const std::vector<std::string>& texts, const Options& o, int skew, int64_t P) {
  std::string all, want;
  std::vector<int64_t> off(1, 0), woff(1, 0);
  int64_t longest = 0;
  for (const std::string& t : texts) {
    all += t;
    off.push_back((int64_t)all.size());
    const std::string u = translate_one(t, o);
    want += u;
    woff.push_back((int64_t)want.size());
    if ((int64_t)u.size() > longest) longest = (int64_t)u.size();
  }
  const Set del(o.del), sq(o.sq);
  TrPlan plan;
  tr_plan(o.table.empty() ? nullptr : (const uint8_t*)o.table.data(), del.bits, sq.bits, nullptr, &plan);
  const Placed pl(all, skew);
  const int64_t n = (int64_t)texts.size(), bytes = (int64_t)want.size();
  if (del.empty() && sq.empty()) {   // the same-length form, the output at every alignment
    for (int oskew = 0; oskew < 16; oskew += (skew % 3) + 1) {
      // the region begins `oskew` bytes into a heap block (16-byte aligned) that ends with it
      Block<uint8_t> room((size_t)bytes + (size_t)oskew);
      translate_map_host(plan, pl.p, room.p + oskew, bytes);
      if (bytes && memcmp(room.p + oskew, want.data(), (size_t)bytes) != 0) fail("wrong mapped bytes", texts, skew, P);
      for (int k = 0; k < oskew; ++k)
        if (room.p[k] != 0xEE) fail("a byte in front of the region was written", texts, skew, P);
    }
    ++checked;
    moved += (long)bytes;
    return;
  }
  for (int shortage = 0; shortage < 2; ++shortage) {   // the capacity exact, a byte short
    if (shortage == 1 && bytes == 0) continue;
    const int64_t ocap = bytes - shortage;
    Block<int64_t> out_off((size_t)n + 1);
    Block<uint8_t> out((size_t)ocap);
    int64_t tot[2] = {-1, -1};
    translate_host(plan, pl.p, off.data(), n, P, TrHostOut{out_off.p, out.p, ocap, tot});
    if (tot[0] != bytes || tot[1] != longest) fail("wrong totals", texts, skew, P);
    if (memcmp(out_off.p, woff.data(), sizeof(int64_t) * ((size_t)n + 1)) != 0) fail("wrong offsets", texts, skew, P);
    if (shortage == 1) {
      if (!out.untouched()) fail("a byte was written although the bytes do not fit", texts, skew, P);
      continue;
    }
    if (bytes && memcmp(out.p, want.data(), (size_t)bytes) != 0) fail("wrong bytes", texts, skew, P);
  }
  ++checked;
  moved += (long)bytes;
}

void check_strip(const std::vector<std::string>& texts, const std::string& members, uint32_t flags, int skew) {
  std::string all;
  std::vector<int64_t> off(1, 0);
  for (const std::string& t : texts) {
    all += t;
    off.push_back((int64_t)all.size());
  }
  const Set set(members);
  TrPlan plan;
  tr_plan(nullptr, nullptr, nullptr, set.bits, &plan);
  plan.mode = TR_STRIP;
  const Placed pl(all, skew);
  Block<int32_t> rows(2 * texts.size());
  strip_host(plan, pl.p, off.data(), (int64_t)texts.size(), flags, rows.p);
  for (size_t i = 0; i < texts.size(); ++i) {
    const std::string& t = texts[i];
    size_t a = 0, b = t.size();
    if (flags & MRX_STRIP_LEFT)
      while (a < t.size() && set.has((unsigned char)t[a])) ++a;
    if (flags & MRX_STRIP_RIGHT)
      while (b > a && set.has((unsigned char)t[b - 1])) --b;
    if (rows.p[2 * i] != (int32_t)a || rows.p[2 * i + 1] != (int32_t)b) fail("wrong strip row", texts, skew, (int64_t)flags);
  }
  ++checked;
}

void check_batch(const std::vector<std::string>& texts, size_t salt) {
  static const int64_t kPieces[4] = {16, 32, 48, 1024};
  std::string lower(256, '\0'), perm(256, '\0'), tab(256, '\0');
  for (int c = 0; c < 256; ++c) {
    lower[c] = (char)(c >= 'A' && c <= 'Z' ? c + 32 : c);
    perm[c] = (char)((c * 167 + 13) & 255);   // (167 is odd: a permutation)
    tab[c] = (char)(c == '\t' ? ' ' : c);
  }
  const Options options[] = {{"", "", ""},      {lower, "", ""},      {perm, "", ""},        {"", "\r", ""},        {"", "\r ab", ""},
                             {"", " \r\tabQ-", ""}, {"", "", " "},    {"", "", " \t-ab"},    {lower, "ab\r", ""},   {tab, "", " "},
                             {perm, " b", ""},  {perm, "", std::string(1, perm[' ']) + perm['a']}};
  size_t k = 0;
  for (const Options& o : options)
    for (int skew = 0; skew < 16; ++skew, ++k) check_translate(texts, o, skew, kPieces[(skew + k + salt) % 4]);
  static const char* const kSets[] = {" \t\n\v\f\r", " ", "ab", " \r\tabQ-", ""};
  for (const char* members : kSets)
    for (uint32_t flags = 1; flags <= 3; ++flags)
      for (int skew = 0; skew < 16; ++skew) check_strip(texts, members, flags, skew);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261020);
  auto run = [&](const char* from, size_t len, int k) {
    std::string s;
    for (int j = 0; j < k; ++j) {
      const char c = from[rng() % len];
      s.append(1 + rng() % 3, c);   // runs: something to squeeze
    }
    return s.substr(0, (size_t)k);
  };
  // the table of the contract, and the edges of squeeze and strip
  for (const char* t : {"", " ", "  ", "a", "GET /A b", "a\r\n", "a  b   c", "a\t b", "aab", "  42 ", "   ", "\t \t \t\t  X\t"})
    check_batch({t}, 0);
  check_batch({}, 0);
  check_batch({"", "", ""}, 1);
  check_batch({"X   ", "   X", " ", " ", " X", std::string(16, ' '), std::string(17, ' '), " "}, 2);
  {   // runs over a block edge and over a piece edge of every piece size; the other byte at a word's first and last place
    std::string t(70, 'X');
    t[14] = t[15] = t[16] = t[17] = ' ';
    t[31] = t[32] = '\r';
    t[47] = t[48] = t[49] = ' ';
    check_batch({t, t.substr(0, 16), t.substr(0, 32), t.substr(15), std::string(40, ' ')}, 2);
    for (int k = 0; k < 34; ++k) check_strip({std::string((size_t)k, ' ') + "Z" + std::string((size_t)(33 - k), ' ')}, " ", 3, k % 16);
  }
  static const char al[] = {' ', ' ', '\r', '\t', 'a', 'b', 'Q', 'X', '-', 'A', '\n', 'e'};
  for (int rep = 0; rep < 40; ++rep) {
    std::vector<std::string> texts;
    const int n = 1 + (int)(rng() % 6);
    for (int i = 0; i < n; ++i) texts.push_back(rng() % 4 == 0 ? std::string() : run(al, rep % 3 == 0 ? 4 : sizeof al, (int)(rng() % 151)));
    check_batch(texts, (size_t)rep);
    check_batch({texts[0]}, (size_t)rep + 1);
  }
  {   // nothing dropped, everything dropped, and a long text: several rounds of the largest piece
    check_batch({std::string(150, 'X'), std::string(70, ' '), std::string(33, '\r')}, 3);
    const std::string t = run(al, sizeof al, 2500);
    check_batch({t, "", t.substr(0, 1024), t.substr(0, 1025)}, 0);
  }
  printf("translate_check ok: %ld batches placed and walked, %ld bytes\n", checked, moved);
  return 0;
}
