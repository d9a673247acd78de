// Host check of format's cell formatter and record assembly (mojo_regex_amd/csrc/mrx_format_bits.hpp: format_cell,
// format_place and format_block, on top of mrx_gather_bits.hpp) against snprintf and a byte-by-byte build of the same
// records, meant for the host sanitizers: no kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/format_check.cpp -o format_check && ./format_check
//
// Cells.  Integers: the edges (powers of ten and of two +- 1, the ends of int64) and random values of every bit length
// under K = 0 .. 20, against "%.*lld" and, for hex, "%.*llx" of the magnitude behind the sign; the precision given to
// snprintf is never 0 (C prints nothing for "%.0d" of 0, format and Python print "0").  FIXED: random bit patterns,
// scaled decimals and dyadic ties under P = 0 .. 9; "%.*f" (glibc rounds the exact binary value, ties to even) is
// compared where the rule answers, and the verdict itself is checked against the number of digits that "%.*f" prints:
// a cell is answered exactly when the value is finite and those digits, without zeros in front, are at most 19.  Every
// cell is also taken in every sub-range that a block boundary can cut it into.
// Records.  Seeded random cases: text columns in a buffer of whole 16-byte words and not a byte more, number columns of
// every kind with rows that print nothing, templates of 0 to 24 segments, and the packed records written at each of the
// 16 output alignments the way k_format_gather writes them; among the cases runs of empty records, a template without
// references, the empty template and few wavefronts so that each runs many rounds.  Everything around the texts, the
// literals and the output is poison (digits, '-', '.'), and the canaries in front of and behind the output must not
// change.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the headers' host + device qualifiers)

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_format_bits.hpp"

using namespace mrx;

namespace {

long cells = 0, answered = 0, refused = 0;

// what snprintf prints for the cell, or "" with *nothing set where format must print nothing
std::string want_cell(int kind, int arg, uint64_t value, bool* nothing) {
  char buf[512];
  *nothing = false;
  if (kind == MRX_COL_INT10) {
    snprintf(buf, sizeof buf, "%.*lld", arg > 1 ? arg : 1, (long long)value);
    return buf;
  }
  if (kind == MRX_COL_INT16) {
    const bool neg = (int64_t)value < 0;
    snprintf(buf, sizeof buf, "%s%.*llx", neg ? "-" : "", arg > 1 ? arg : 1, (unsigned long long)(neg ? 0 - value : value));
    return buf;
  }
  double v;
  memcpy(&v, &value, 8);
  if (!std::isfinite(v)) {
    *nothing = true;
    return "";
  }
  snprintf(buf, sizeof buf, "%.*f", arg, v);
  size_t digits = 0;
  bool lead = true;
  for (const char* p = buf; *p; ++p) {
    if (*p < '0' || *p > '9') continue;
    if (lead && *p == '0') continue;
    lead = false;
    ++digits;
  }
  if (digits > 19) {
    *nothing = true;
    return "";
  }
  return buf;
}

int check_cell(int kind, int arg, uint64_t value) {
  bool nothing;
  const std::string want = want_cell(kind, arg, value, &nothing);
  uint64_t mag = 0;
  int32_t desc = 0;
  const int st = format_cell(kind, arg, value, &mag, &desc);
  ++cells;
  if (nothing) {
    ++refused;
    if (st == MRX_NUM_RANGE) return 0;
    printf("FAIL: kind %d arg %d value %016llx: answered, but it is not below 10^19\n", kind, arg, (unsigned long long)value);
    return 1;
  }
  ++answered;
  uint8_t out[32];
  memset(out, 0xA5, sizeof out);
  if (st != MRX_NUM_OK || format_cell_bytes(mag, desc, out) != (int)want.size() || memcmp(out, want.data(), want.size()) != 0 ||
      out[want.size()] != 0xA5 || want.size() > (size_t)kFmtCellMax) {
    printf("FAIL: kind %d arg %d value %016llx: status %d \"%.*s\", expected \"%s\"\n", kind, arg, (unsigned long long)value, st,
           st == MRX_NUM_OK ? format_desc_len(desc) : 0, (const char*)out, want.c_str());
    return 1;
  }
  // every sub-range at every place in a block
  const int len = (int)want.size();
  for (int off = 0; off < len; ++off)
    for (int take = 1; take <= 16 && off + take <= len; take += (take < 3 || off + take + 1 >= len) ? 1 : 5)
      for (int at = 0; at + take <= 16; at += 1 + (off + at) % 4) {
        const g_u128 acc = format_place(0, mag, desc, off, take, at);
        for (int q = 0; q < 16; ++q) {
          const uint8_t b = (uint8_t)(acc >> (8 * q));
          if (b != (q >= at && q < at + take ? (uint8_t)want[off + q - at] : 0)) {
            printf("FAIL: \"%s\" bytes [%d, %d) placed at %d: byte %d is %02x\n", want.c_str(), off, off + take, at, q, b);
            return 1;
          }
        }
      }
  return 0;
}

int check_cells(std::mt19937_64& rng) {
  std::vector<int64_t> ints = {0, 1, -1, INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1, 255, -255, 99999999, 100000000,
                               9999999999999999ll, 10000000000000000ll};
  for (int k = 0; k < 19; ++k)
    for (int d = -1; d <= 1; ++d) {
      ints.push_back((int64_t)format_pow10(k) + d);
      ints.push_back(-((int64_t)format_pow10(k) + d));
    }
  for (int k = 0; k < 63; ++k)
    for (int d = -1; d <= 1; ++d) {
      ints.push_back(((int64_t)1 << k) + d);
      ints.push_back(-(((int64_t)1 << k) + d));
    }
  for (int rep = 0; rep < 3000; ++rep) ints.push_back((int64_t)((rng() >> (rng() % 64)) * (rng() & 1 ? 1ull : ~0ull)));
  for (int64_t v : ints)
    for (int K = 0; K <= 20; K += (v & 3) == 0 || K < 2 || K > 17 ? 1 : 3)
      if (check_cell(MRX_COL_INT10, K, (uint64_t)v) || check_cell(MRX_COL_INT16, K, (uint64_t)v)) return 1;
  // the SWAR steps on their own: every chunk value at a stride, every 4-digit half exactly
  for (uint32_t v = 0; v < 100000000u; v += v < 20000 ? 1 : 9973) {
    char buf[16];
    snprintf(buf, sizeof buf, "%08u", v);
    const uint64_t got = format_dec8(v);
    if (memcmp(&got, buf, 8) != 0) {
      printf("FAIL: format_dec8(%u)\n", v);
      return 1;
    }
    snprintf(buf, sizeof buf, "%08x", v * 43u);
    const uint64_t hx = format_hex8(v * 43u);
    if (memcmp(&hx, buf, 8) != 0) {
      printf("FAIL: format_hex8(%x)\n", v * 43u);
      return 1;
    }
  }
  std::vector<double> dbl = {0.0, -0.0, 0.5, 1.5, 2.5, -2.5, 0.125, -0.04, 0.05, 1e-9, 5e-10, 5e-324, -5e-324, 2.2250738585072014e-308,
                             9007199254740992.0, 9223372036854775808.0, 18446744073709551616.0, 1e18, 1e19, 1e22, 1e300, NAN,
                             INFINITY, -INFINITY, 0.9999999995, 9.9999999995, 123456.789};
  for (int P = 0; P <= 9; ++P) {
    const double bound = std::pow(10.0, 19 - P);
    for (double v : {bound, std::nextafter(bound, 0.0), std::nextafter(bound, INFINITY), bound - 0.5 / std::pow(10.0, P)}) {
      dbl.push_back(v);
      dbl.push_back(-v);
    }
  }
  for (int k = 1; k <= 12; ++k)
    for (int j = 0; j < 8; ++j) dbl.push_back((2 * j + 1) / std::pow(2.0, k) * (j & 1 ? -1 : 1));
  for (int rep = 0; rep < 40000; ++rep) {
    double v;
    switch (rep % 3) {
      case 0: {
        const uint64_t bits = rng();
        memcpy(&v, &bits, 8);
        break;
      }
      case 1: v = (double)(rng() % 10000000) * std::pow(10.0, (int)(rng() % 25) - 12) * (rng() & 1 ? 1 : -1); break;
      default: v = (double)(2 * (rng() % (1 << 20)) + 1) / std::pow(2.0, 1 + (int)(rng() % 29)); break;
    }
    dbl.push_back(v);
  }
  for (size_t i = 0; i < dbl.size(); ++i) {
    uint64_t bits;
    memcpy(&bits, &dbl[i], 8);
    for (int P = 0; P <= 9; P += i < 200 || i % 5 == 0 ? 1 : 3)
      if (check_cell(MRX_COL_FIXED, P, bits)) return 1;
  }
  return 0;
}

// out[0 .. bytes) as nw wavefronts of k_format_gather assemble it, lane after lane: a sequential loop of this file's own
// with the arithmetic of the device's one walk (gather_blocks in mrx_gather_bits.hpp, device code: it takes its wavefront
// and lane from the launch) around the same fill, format_block
void gather_records(const FormatSrc& S, int64_t bytes, uint8_t* out, int64_t nw) {
  if (bytes <= 0) return;
  const uintptr_t ob = (uintptr_t)out, a0 = ob & ~(uintptr_t)15;
  const int64_t head = (int64_t)(ob - a0), nblk = (head + bytes + 15) >> 4;
  const int64_t per = ((nblk + nw - 1) / nw + 63) & ~(int64_t)63;
  for (int64_t w = 0; w < nw; ++w) {
    const int64_t b_begin = w * per, b_end = b_begin + per < nblk ? b_begin + per : nblk;
    if (b_begin >= b_end) continue;
    const int64_t p_first = b_begin * 16 - head;
    int64_t cur = gather_last_le(S.out_off, 0, S.rows, p_first > 0 ? p_first : 0);
    for (int64_t b0 = b_begin; b0 < b_end; b0 += 64) {
      const int64_t bl = b0 + 63 < b_end ? b0 + 63 : b_end - 1;
      const int64_t pe = bl * 16 - head + 15, pl = pe < bytes ? pe : bytes - 1;
      const int64_t hi = gather_gallop(S.out_off, cur, S.rows, pl);
      for (int64_t b = b0; b <= bl; ++b) {
        const int64_t p0 = b * 16 - head, pos = p0 > 0 ? p0 : 0, endp = p0 + 16 < bytes ? p0 + 16 : bytes;
        const int64_t r = gather_last_le(S.out_off, cur, hi + 1, pos);
        const g_u128 acc = format_block(S, r, hi, p0, pos, endp);
        uint8_t* dst = (uint8_t*)(a0 + (uintptr_t)b * 16);
        if (p0 >= 0 && p0 + 16 <= bytes) {
          gather_store16(dst, acc);
        } else {
          for (int q = p0 < 0 ? (int)-p0 : 0; q < (int)(endp - p0); ++q) dst[q] = (uint8_t)(acc >> (8 * q));
        }
      }
      cur = hi;
    }
  }
}

struct Case {
  int rows, min_segs, max_segs, max_lit, nslots;
  int nothing_pct;   // how many cells print nothing (an empty text, a number without a cell)
  int max_text;
  bool lits;
  const char* name;
};

const char kPoison[] = "0123456789-.";

int run_case(const Case& c, std::mt19937_64& rng, int* checked) {
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  const int ns = c.nslots > 0 ? c.nslots : 1;
  const size_t rows = (size_t)c.rows;
  // the template
  const int nseg = rnd(c.min_segs, c.max_segs);
  std::vector<ExpandSeg> segs;
  std::vector<uint8_t> lits;
  for (int k = 0; k < nseg; ++k) {
    const bool lit = c.lits && (c.nslots == 0 || rng() % 2);
    if (lit && (segs.empty() || segs.back().slot >= 0)) {
      const int len = rnd(1, c.max_lit);
      segs.push_back(ExpandSeg{(int64_t)lits.size(), len, -1, 0});
      for (int q = 0; q < len; ++q) lits.push_back((uint8_t)('A' + rng() % 26));
    } else if (c.nslots > 0) {
      segs.push_back(ExpandSeg{0, 0, rnd(0, c.nslots - 1), 0});
    }
  }
  const size_t lit_bytes = lits.empty() ? 16 : (lits.size() + 15) / 16 * 16;
  uint8_t* dlits = (uint8_t*)aligned_alloc(16, lit_bytes);
  for (size_t k = 0; k < lit_bytes; ++k) dlits[k] = (uint8_t)kPoison[k % 12];
  if (!lits.empty()) memcpy(dlits, lits.data(), lits.size());
  // the columns: a text column's texts lie in one buffer of whole 16-byte words with poison between them
  std::vector<int> kind(ns), arg(ns);
  std::vector<uint64_t> word(rows * ns);
  std::vector<int32_t> desc(rows * ns);
  std::vector<std::string> cell(rows * ns);
  std::vector<uint8_t*> bufs;
  for (int q = 0; q < c.nslots; ++q) {
    kind[q] = rnd(0, 3);
    arg[q] = kind[q] == MRX_COL_FIXED ? rnd(0, 9) : kind[q] == MRX_COL_TEXT ? 0 : rnd(0, 20);
    if (kind[q] == MRX_COL_TEXT) {
      std::vector<int64_t> at(rows);
      std::vector<int> len(rows);
      int64_t end = rnd(0, 15);
      for (size_t r = 0; r < rows; ++r) {
        at[r] = end;
        len[r] = rnd(0, 99) < c.nothing_pct ? 0 : rnd(1, c.max_text);
        end += len[r] + rnd(0, 3);
      }
      const size_t nb = (size_t)(end > 0 ? (end + 15) / 16 * 16 : 16);
      uint8_t* data = (uint8_t*)aligned_alloc(16, nb);
      bufs.push_back(data);
      for (size_t k = 0; k < nb; ++k) data[k] = (uint8_t)kPoison[(7 * k + q) % 12];
      for (size_t r = 0; r < rows; ++r) {
        for (int k = 0; k < len[r]; ++k) data[at[r] + k] = (uint8_t)('a' + rng() % 26);
        // (an empty text may point anywhere, also behind the buffer: nothing is read for it)
        word[(size_t)q * rows + r] = (uint64_t)(uintptr_t)(len[r] ? data + at[r] : data + nb);
        desc[(size_t)q * rows + r] = len[r];
        cell[(size_t)q * rows + r].assign((const char*)data + at[r], (size_t)len[r]);
      }
    } else {
      for (size_t r = 0; r < rows; ++r) {
        uint64_t v = rng() >> (rng() % 64);
        if (rng() & 1) v = 0 - v;
        if (kind[q] == MRX_COL_FIXED) {
          const double d = (double)(int64_t)v / std::pow(10.0, rnd(0, 12));
          memcpy(&v, &d, 8);
        }
        bool nothing;
        std::string want = want_cell(kind[q], arg[q], v, &nothing);
        uint64_t mag = 0xA5A5A5A5A5A5A5A5ull;   // (a fill word: never printed)
        int32_t ds = 0;
        if (rnd(0, 99) < c.nothing_pct) {
          want.clear();
        } else if (format_cell(kind[q], arg[q], v, &mag, &ds) != MRX_NUM_OK) {
          if (!nothing) {
            printf("FAIL: %s: a cell was refused that snprintf prints as %s\n", c.name, want.c_str());
            return 1;
          }
          ds = 0;
        }
        word[(size_t)q * rows + r] = mag;
        desc[(size_t)q * rows + r] = ds;
        cell[(size_t)q * rows + r] = want;
      }
    }
  }
  // the records, byte by byte
  std::vector<int64_t> off{0};
  std::vector<uint8_t> want;
  for (size_t r = 0; r < rows; ++r) {
    for (const ExpandSeg& sg : segs) {
      if (sg.slot < 0) {
        want.insert(want.end(), lits.begin() + sg.lit_off, lits.begin() + sg.lit_off + sg.lit_len);
      } else {
        const std::string& s = cell[(size_t)sg.slot * rows + r];
        want.insert(want.end(), s.begin(), s.end());
      }
    }
    off.push_back((int64_t)want.size());
  }
  const int64_t bytes = off.back();
  const FormatSrc S{dlits, segs.data(), (int32_t)segs.size(), 0, (int64_t)rows, word.data(), desc.data(), off.data()};
  for (int skew = 0; skew < 16; ++skew) {
    const size_t out_bytes = (size_t)((16 + skew + bytes + 16 + 15) / 16 * 16);
    uint8_t* buf = (uint8_t*)aligned_alloc(16, out_bytes);
    for (size_t k = 0; k < out_bytes; ++k) buf[k] = (uint8_t)kPoison[(5 * k + skew) % 12];
    std::vector<uint8_t> before(buf, buf + out_bytes);
    uint8_t* out = buf + 16 + skew;
    gather_records(S, bytes, out, skew % 3 == 0 ? 1 : skew % 3 == 1 ? 3 : 64);
    if (bytes && memcmp(out, want.data(), (size_t)bytes) != 0) {
      printf("FAIL: %s: bytes differ (output skew %d)\n", c.name, skew);
      return 1;
    }
    for (size_t q = 0; q < out_bytes; ++q)
      if ((q < (size_t)(16 + skew) || q >= (size_t)(16 + skew + bytes)) && buf[q] != before[q]) {
        printf("FAIL: %s: canary byte %zu changed (output skew %d)\n", c.name, q, skew);
        return 1;
      }
    free(buf);
    ++*checked;
  }
  free(dlits);
  for (uint8_t* p : bufs) free(p);
  return 0;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261019);
  if (check_cells(rng)) return 1;
  const Case cases[] = {
      {300, 0, 24, 40, 9, 20, 40, true, "random"},
      {2000, 1, 6, 3, 3, 40, 2, true, "short records"},
      {1500, 1, 5, 1, 4, 97, 3, false, "runs of empty records"},
      {60, 6, 12, 300, 5, 10, 700, true, "records longer than 64 blocks"},
      {600, 1, 3, 1, 2, 0, 1, false, "number cells cut by every block boundary"},
      {700, 0, 0, 1, 0, 0, 0, true, "empty template"},
      {200, 1, 1, 300, 0, 0, 0, true, "no references"},
      {5000, 1, 3, 2, 2, 20, 6, true, "many rounds per wavefront"},
  };
  int checked = 0;
  for (int rep = 0; rep < 6; ++rep)
    for (const Case& c : cases)
      if (run_case(c, rng, &checked)) return 1;
  printf("format_check ok: %ld cells (%ld answered, %ld refused) equal snprintf in every sub-range; %d sweeps equal the byte-by-byte records, canaries intact\n",
         cells, answered, refused, checked);
  return 0;
}
