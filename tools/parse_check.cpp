// Host check of the number parser (mojo_regex_amd/csrc/mrx_parse_bits.hpp) against strtoll, strtoull and strtod, meant
// for the host sanitizers: no kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/parse_check.cpp -o parse_check && ./parse_check
//
// Every piece lies at every alignment 0..15 inside a buffer of exactly the aligned 16-byte words that hold it, so a read
// outside the words that the read contract of include/mrx.h allows is the sanitizer's to report; an empty piece points
// behind a buffer, where any read is one.  Everything else in the buffers is digits ('7', or '0' .. '9' in turn),
// which a missing mask would turn into another number.
//   - the grammar of each kind is restated with std::regex, and a piece's status must agree with it;
//   - integers: lengths 0 to 40, decimal and hex, signs, prefixes, leading zeros, the values around 2^63 and 2^64, and
//     random bytes from an alphabet of digits and near misses; the value against strtoll (decimal) and against
//     strtoull of the magnitude with the sign applied (both kinds), their ERANGE against MRX_NUM_RANGE;
//   - pieces of 41 to 130 and more bytes: runs of digits that go on behind an overflow or a full mantissa, some with a
//     late byte outside the grammar;
//   - floats: generated strings (integer part, point, fraction, exponent, each present or not, zeros in front and
//     behind, up to 45 mantissa digits); the d, q rule is restated on the digit string, and every piece it answers
//     must equal strtod in all 64 bits, the sign of zero included.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the headers' host + device qualifiers)

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <regex>
#include <string>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_parse_bits.hpp"

using namespace mrx;

namespace {

// `bytes` at alignment `skew` in a fresh buffer of exactly the aligned words that hold them; the rest is digits
struct Placed {
  uint8_t* buf;
  const uint8_t* p;
  Placed(const std::string& bytes, int skew, int poison) {
    const size_t words = bytes.empty() ? 1 : (skew + bytes.size() + 15) / 16;
    buf = (uint8_t*)aligned_alloc(16, words * 16);
    for (size_t k = 0; k < words * 16; ++k) buf[k] = poison ? (uint8_t)('0' + k % 10) : (uint8_t)'7';
    if (!bytes.empty()) memcpy(buf + skew, bytes.data(), bytes.size());
    p = bytes.empty() ? buf + words * 16 : buf + skew;   // an empty piece: nothing may be read at all
  }
  ~Placed() { free(buf); }
  Placed(const Placed&) = delete;
};

const std::regex kInt10("[+-]?[0-9]+"), kInt16("[+-]?(0[xX])?[0-9a-fA-F]+"),
    kFloat("[+-]?([0-9]+\\.?[0-9]*|\\.[0-9]+)([eE][+-]?[0-9]+)?");

struct Want {
  int status;
  uint64_t bits;
};

bool has_nul(const std::string& t) { return t.find('\0') != std::string::npos; }

Want want_int(const std::string& t, bool hex) {
  if (t.empty()) return {MRX_NUM_EMPTY, 0};
  if (has_nul(t) || !std::regex_match(t, hex ? kInt16 : kInt10)) return {MRX_NUM_MALFORMED, 0};
  size_t at = t[0] == '+' || t[0] == '-';
  const bool neg = t[0] == '-';
  if (hex && t.size() >= at + 3 && t[at] == '0' && (t[at + 1] | 0x20) == 'x') at += 2;   // (0x needs a digit behind it)
  errno = 0;
  const unsigned long long mag = strtoull(t.c_str() + at, nullptr, hex ? 16 : 10);
  const bool over = errno == ERANGE || mag > ((1ull << 63) - (neg ? 0 : 1));
  if (!hex) {   // strtoll reads the decimal grammar as it stands
    errno = 0;
    const long long v = strtoll(t.c_str(), nullptr, 10);
    if ((errno == ERANGE) != over || (!over && (uint64_t)v != (neg ? 0 - mag : mag))) {
      printf("strtoll and strtoull disagree on %s\n", t.c_str());
      exit(1);
    }
  }
  if (over) return {MRX_NUM_RANGE, 0};
  return {MRX_NUM_OK, neg ? 0 - mag : mag};
}

Want want_float(const std::string& t) {
  if (t.empty()) return {MRX_NUM_EMPTY, 0};
  if (has_nul(t) || !std::regex_match(t, kFloat)) return {MRX_NUM_MALFORMED, 0};
  size_t at = t[0] == '+' || t[0] == '-';
  const bool neg = t[0] == '-';
  std::string digits;
  long long frac = 0;
  bool point = false;
  for (; at < t.size() && (t[at] | 0x20) != 'e'; ++at) {
    if (t[at] == '.') {
      point = true;
    } else {
      digits += t[at];
      frac += point;
    }
  }
  long long exp = 0;
  if (at < t.size()) {
    const std::string e = t.substr(at + 1);
    const bool eneg = e[0] == '-';
    for (size_t k = e[0] == '+' || e[0] == '-'; k < e.size(); ++k)
      if (exp < 100000) exp = exp * 10 + (e[k] - '0');
    if (eneg) exp = -exp;
  }
  long long q = exp - frac;
  digits.erase(0, digits.find_first_not_of('0'));   // (npos: all of it)
  while (!digits.empty() && digits.back() == '0') {
    digits.pop_back();
    ++q;
  }
  double v;
  uint64_t bits;
  if (digits.empty()) {
    bits = 0;
  } else {
    if (digits.size() > 16 || q < -22 || q > 22) return {MRX_NUM_RANGE, 0};   // 2^53 has 16 digits
    const unsigned long long d = strtoull(digits.c_str(), nullptr, 10);
    if (d > (1ull << 53)) return {MRX_NUM_RANGE, 0};
    v = strtod(t.c_str() + (t[0] == '+' || t[0] == '-'), nullptr);   // the exact-or-refused rule answers as strtod does
    memcpy(&bits, &v, 8);
  }
  return {MRX_NUM_OK, bits | ((uint64_t)neg << 63)};
}

long checked = 0, answered = 0;

void check(const std::string& t, int kind) {
  const Want w = kind == MRX_NUM_FLOAT ? want_float(t) : want_int(t, kind == MRX_NUM_INT16);
  for (int skew = 0; skew < 16; ++skew) {
    const Placed pl(t, skew, skew & 1);
    uint64_t bits = 0xA5A5A5A5A5A5A5A5ull;
    const int st = parse_piece(pl.p, (int64_t)t.size(), kind, &bits);
    if (st != w.status || (st == MRX_NUM_OK ? bits != w.bits : bits != 0xA5A5A5A5A5A5A5A5ull)) {
      printf("kind %d, alignment %d, piece of %zu bytes \"%s\": status %d value %016llx, expected %d %016llx\n", kind, skew,
             t.size(), t.c_str(), st, (unsigned long long)bits, w.status, (unsigned long long)w.bits);
      exit(1);
    }
  }
  ++checked;
  answered += w.status == MRX_NUM_OK;
}

void check_all_kinds(const std::string& t) {
  for (int kind : {MRX_NUM_INT10, MRX_NUM_INT16, MRX_NUM_FLOAT}) check(t, kind);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20260519);
  auto pick = [&](const char* from) { return from[rng() % strlen(from)]; };
  auto run = [&](const char* from, int k) {
    std::string s;
    for (int j = 0; j < k; ++j) s += pick(from);
    return s;
  };
  // the listed edges
  const char* edges[] = {"", "+", "-", "-0", "+0", "0", "00", "9223372036854775807", "9223372036854775808",
                         "-9223372036854775808", "-9223372036854775809", "18446744073709551615", "18446744073709551616",
                         "0x", "0X", "0X1f", "-0xff", "+0x0", "0x0x1", "00x1", "x1", "0xg", "7fffffffffffffff",
                         "8000000000000000", "-8000000000000000", "-8000000000000001", "ffffffffffffffff",
                         "0xffffffffffffffff", "10000000000000000", ".", "1.", ".5", "+.5", "-.", "1e22", "1e23", "1e-22",
                         "1e-23", "123e-25", "9007199254740992", "9007199254740993", "9007199254740992e22", "1.e5", ".e5",
                         "1e", "1e+", "1e+5", "1E-5", "1.5.2", "1e5e5", "-0.0e999", "0e99999999999999999999",
                         "1e99999999999999999999", "1e-99999999999999999999", "1_0", "inf", "nan", "-inf", " 1", "1 ",
                         "1\n", "0x1p3", "1f", "1d", "--1", "+-1", "1-", "e5", "1.5e", "15e-1", "0.1", "0.000001", "123.456"};
  for (const char* e : edges) check_all_kinds(e);
  check_all_kinds(std::string(100, '0') + "1");
  check_all_kinds(std::string(100, '0') + "1.5e3");
  check_all_kinds("1.5" + std::string(22, '0'));
  check_all_kinds("15" + std::string(22, '0'));
  check_all_kinds("15" + std::string(23, '0'));
  check_all_kinds("1e" + std::string(20, '9'));
  check_all_kinds(std::string("1\0" "2", 3));
  check_all_kinds(std::string("\0", 1));
  // integers: every length 0..40
  for (int len = 0; len <= 40; ++len) {
    for (int rep = 0; rep < 60; ++rep) {
      std::string t;
      switch (rep % 6) {
        case 0: t = run("0123456789", len); break;
        case 1: t = len ? pick("+-") + run("0123456789", len - 1) : ""; break;
        case 2: t = run("0123456789abcdefABCDEF", len); break;
        case 3: t = len > 2 ? std::string(rng() & 1 ? "0x" : "-0X") + run("0123456789abcdefABCDEF", len - 2) : run("0x-", len); break;
        case 4: t = std::string(rng() % (len + 1), '0') + run("0123456789", 19); t.resize(len); break;
        default: t = run("0123456789abcdefxX+-_ .eg", len); break;
      }
      check_all_kinds(t);
    }
  }
  for (int len = 41; len <= 130; ++len)   // long runs of digits behind an overflow, with and without a late byte that spoils them
    for (int rep = 0; rep < 6; ++rep) {
      std::string t = rep & 1 ? run("0123456789", len) : pick("+-1") + run("0123456789", len / 3) + "." + run("0123456789", len);
      if (rep >= 2) t[len - 1 - rng() % 20] = pick("x_e.-f 0");
      if (rep == 5) t += "e-" + run("0123456789", 3);
      check_all_kinds(t);
    }
  for (int len = 15; len <= 22; ++len)   // around 2^63 and 2^64 in both bases
    for (int rep = 0; rep < 400; ++rep) {
      check(pick("+-9") + run("0123456789", len), MRX_NUM_INT10);
      check(pick("+-f") + run("0123456789abcdef", len - 3), MRX_NUM_INT16);
    }
  // floats
  for (int rep = 0; rep < 60000; ++rep) {
    std::string t;
    if (rng() % 4 == 0) t += pick("+-");
    const int shape = (int)(rng() % 8);
    const int ni = shape == 7 ? 0 : (int)(rng() % (rep % 16 == 0 ? 30 : 9)), nf = (int)(rng() % (rep % 16 == 1 ? 30 : 9));
    std::string ip = run("0123456789", ni), fp = run("0123456789", nf);
    if (rng() % 3 == 0) ip = std::string(rng() % 4, '0') + ip;
    if (rng() % 3 == 0) fp += std::string(rng() % 25, '0');
    if (rng() % 5 == 0) ip += std::string(rng() % 25, '0');
    t += ip;
    if (shape != 0) t += "." + fp;
    if (rng() % 2) {
      t += pick("eE");
      if (rng() % 2) t += pick("+-");
      t += rng() % 8 == 0 ? run("0123456789", (int)(rng() % 6)) : std::to_string(rng() % 30);
    }
    if (rng() % 50 == 0 && !t.empty()) t[rng() % t.size()] = pick("_ x.e-+\0");
    check(t, MRX_NUM_FLOAT);
    if (rep % 8 == 0) check_all_kinds(t);
  }
  printf("parse_check ok: %ld pieces at 16 alignments each, %ld answered\n", checked, answered);
  return 0;
}
