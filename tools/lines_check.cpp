// Host check of the lines walk (mojo_regex_amd/csrc/mrx_lines_bits.hpp) against a split that knows no blocks and no
// pieces, meant for the host sanitizers: no kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/lines_check.cpp -o lines_check && ./lines_check
//
// The walk is the one the kernels run: lines_block per aligned 16-byte block, and lines_host over the kernels' pieces
// and passes, at the piece sizes 16, 32, 48 and 1024.
//   - Every batch lies at every alignment 0..15 inside a buffer of exactly the aligned 16-byte words that hold it, so a
//     read outside the words that the read contract of include/mrx.h allows is the sanitizer's to report; an empty batch
//     points behind a buffer, where any read is one.  Everything else in the buffer is "\n\r\n\r": a walk that took it
//     for text would find other lines.
//   - The outputs are heap blocks of exactly the expected sizes: a write past the lines or the bytes is the sanitizer's
//     to report too.  With a capacity one short, nothing at all may be written behind it.
//   - Texts over {a, b, \n, \r} of 0 to 150 bytes, alone and as batches of 1 to 6 with empty ones among them; every flag
//     combination that the entry points accept, and the separators '\n' and 'a'.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the headers' host + device qualifiers)

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_lines_bits.hpp"

using namespace mrx;

namespace {

struct Placed {
  uint8_t* buf;
  const uint8_t* p;
  Placed(const std::string& bytes, int skew) {
    const size_t words = bytes.empty() ? 1 : (skew + bytes.size() + 15) / 16;
    buf = (uint8_t*)aligned_alloc(16, words * 16);
    for (size_t k = 0; k < words * 16; ++k) buf[k] = (uint8_t)("\n\r\n\r"[k % 4]);
    if (!bytes.empty()) memcpy(buf + skew, bytes.data(), bytes.size());
    p = bytes.empty() ? buf + words * 16 : buf + skew;   // an empty batch: nothing may be read at all
  }
  ~Placed() { free(buf); }
  Placed(const Placed&) = delete;
};

struct Want {
  std::vector<int64_t> prefix, owner, off;
  std::string data;
  int64_t longest = 0, tail = 0;
};

Want expected(const std::vector<std::string>& texts, char sep, uint32_t flags) {
  Want w;
  w.prefix.push_back(0);
  w.off.push_back(0);
  for (size_t i = 0; i < texts.size(); ++i) {
    const std::string& t = texts[i];
    size_t start = 0;
    auto line = [&](std::string l) {
      w.owner.push_back((int64_t)i);
      w.data += l;
      w.off.push_back((int64_t)w.data.size());
      if ((int64_t)l.size() > w.longest) w.longest = (int64_t)l.size();
    };
    for (size_t q = 0; q < t.size(); ++q) {
      if (t[q] != sep) continue;
      std::string l = t.substr(start, q - start);
      if ((flags & MRX_LINES_CRLF) && !l.empty() && l.back() == '\r') l.pop_back();
      if (flags & MRX_LINES_KEEPENDS) l += sep;
      line(l);
      start = q + 1;
    }
    w.tail = (int64_t)(t.size() - start);
    if (!(flags & MRX_LINES_DROP_PARTIAL) && start < t.size()) line(t.substr(start));
    w.prefix.push_back((int64_t)w.owner.size());
  }
  if (texts.empty()) w.tail = 0;
  return w;
}

long checked = 0, found = 0;

void fail(const char* what, const std::vector<std::string>& texts, int skew, int64_t P, uint32_t flags) {
  printf("%s: %zu texts, the first of %zu bytes, at alignment %d, pieces of %lld, flags %u\n", what, texts.size(),
         texts.empty() ? (size_t)0 : texts[0].size(), skew, (long long)P, flags);
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

void check_batch_at(const std::vector<std::string>& texts, char sep, uint32_t flags, int skew, int64_t P) {
  std::string all;
  std::vector<int64_t> off(1, 0);
  for (const std::string& t : texts) {
    all += t;
    off.push_back((int64_t)all.size());
  }
  const Want w = expected(texts, sep, flags);
  const Placed pl(all, skew);
  const int64_t n = (int64_t)texts.size(), lines = (int64_t)w.owner.size(), bytes = (int64_t)w.data.size();
  for (int shortage = 0; shortage < 3; ++shortage) {   // both capacities exact, a line short, a byte short
    if ((shortage == 1 && lines == 0) || (shortage == 2 && bytes == 0)) continue;
    const int64_t pcap = lines - (shortage == 1), ocap = bytes - (shortage == 2);
    Block<int64_t> prefix((size_t)n + 1), owner((size_t)pcap), out_off((size_t)pcap + 1);
    Block<uint8_t> out((size_t)ocap);
    int64_t tot[4] = {-1, -1, -1, -1};
    lines_host(pl.p, off.data(), n, P, (uint8_t)sep, flags, LinesHostOut{prefix.p, owner.p, out_off.p, pcap, out.p, ocap, tot});
    if (tot[0] != lines || tot[1] != bytes || tot[3] != w.tail) fail("wrong totals", texts, skew, P, flags);
    if (memcmp(prefix.p, w.prefix.data(), sizeof(int64_t) * ((size_t)n + 1)) != 0) fail("wrong line prefix", texts, skew, P, flags);
    if (shortage == 1) {
      if (!owner.untouched() || !out_off.untouched() || !out.untouched()) fail("written although the lines do not fit", texts, skew, P, flags);
      continue;
    }
    if (tot[2] != w.longest) fail("wrong longest line", texts, skew, P, flags);
    if (lines && memcmp(owner.p, w.owner.data(), sizeof(int64_t) * (size_t)lines) != 0) fail("wrong owner", texts, skew, P, flags);
    if (memcmp(out_off.p, w.off.data(), sizeof(int64_t) * ((size_t)lines + 1)) != 0) fail("wrong offsets", texts, skew, P, flags);
    if (shortage == 2) {
      if (!out.untouched()) fail("a byte was written although the bytes do not fit", texts, skew, P, flags);
      continue;
    }
    if (bytes && memcmp(out.p, w.data.data(), (size_t)bytes) != 0) fail("wrong bytes", texts, skew, P, flags);
  }
  ++checked;
  found += (long)lines;
}

void check_batch(const std::vector<std::string>& texts, size_t salt) {
  static const uint32_t kFlagSets[6] = {0, MRX_LINES_KEEPENDS, MRX_LINES_CRLF, MRX_LINES_DROP_PARTIAL,
                                        MRX_LINES_KEEPENDS | MRX_LINES_DROP_PARTIAL, MRX_LINES_CRLF | MRX_LINES_DROP_PARTIAL};
  static const int64_t kPieces[4] = {16, 32, 48, 1024};
  for (int f = 0; f < 6; ++f)
    for (int skew = 0; skew < 16; ++skew) {
      check_batch_at(texts, '\n', kFlagSets[f], skew, kPieces[(skew + f + salt) % 4]);
      if (!(kFlagSets[f] & MRX_LINES_CRLF)) check_batch_at(texts, 'a', kFlagSets[f], skew, kPieces[(skew + f + salt + 1) % 4]);
    }
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261020);
  auto run = [&](const char* from, size_t len, int k) {
    std::string s;
    for (int j = 0; j < k; ++j) s += from[rng() % len];
    return s;
  };
  // the table of the contract, and the edges of CRLF
  for (const char* t : {"", "\n", "a", "a\nb", "a\nb\n", "\n\na", "\r", "\r\n", "a\r", "a\r\r\n", "\r\r\n\r", "a\r\nb\r"})
    check_batch({t}, 0);
  check_batch({}, 0);
  check_batch({"", "", ""}, 1);
  {   // a '\r' as the last byte of a block with its '\n' in the next one, and as the last byte of a text with a '\n'
      // behind it that is not text
    std::string t(40, 'b');
    t[15] = '\r';
    t[16] = '\n';
    t[31] = '\r';
    check_batch({t, t.substr(0, 16), t.substr(0, 32), "\n"}, 2);
  }
  for (int rep = 0; rep < 60; ++rep) {
    static const char al[] = {'a', 'b', '\n', '\r', '\n', 'b', 'b', 'b'};
    const size_t spread = rep % 3 == 0 ? 8 : 4;   // (the first four: a line end every other byte)
    std::vector<std::string> texts;
    const int n = 1 + (int)(rng() % 6);
    for (int i = 0; i < n; ++i) texts.push_back(rng() % 4 == 0 ? std::string() : run(al, spread, (int)(rng() % 151)));
    check_batch(texts, (size_t)rep);
    check_batch({texts[0]}, (size_t)rep + 1);
  }
  {   // no separator at all, only separators, and a long text: several rounds of the largest piece
    check_batch({std::string(150, 'b'), std::string(70, '\n'), std::string(33, '\r')}, 3);
    std::string t = run("bbbbbbb\n\r", 9, 2500);
    check_batch({t, "", t.substr(0, 1024), t.substr(0, 1025)}, 0);
  }
  printf("lines_check ok: %ld batches placed and walked, %ld lines\n", checked, found);
  return 0;
}
