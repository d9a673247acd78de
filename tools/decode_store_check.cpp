// decode_store_plan (csrc/mrx_decode_bits.hpp) replayed on the host: the index arithmetic behind k_decode's 16-byte span
// stores, for every combination of the parity of pre0, the parity of the buffer's address, nspan in 0..9 and TILE - 1,
// TILE (both tile sizes), and span_cap from pre0 - 1 to pre0 + nspan + 1.  A stand-alone program, meant to be built with
// the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mojo_regex_amd/csrc \
//       tools/decode_store_check.cpp -o decode_store_check && ./decode_store_check
// The model: memory is a row of 8-byte cells; the buffer begins at cell `a` (its address parity), so span index i is
// cell a + i and a 16-byte store is legal on an even cell only.  The tile holds span k of the wavefront at slot k + odd.
// Exit status 0 and a count of the cases, or the first failure on stderr and 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mrx_decode_bits.hpp"

namespace {

constexpr int32_t kSentinel = -77;
long g_cases = 0;

[[noreturn]] void fail(const char* what, int64_t pre0, int a, int nspan, int64_t cap, int64_t at) {
  std::fprintf(stderr, "decode_store_check: %s (pre0 %lld, address parity %d, nspan %d, span_cap %lld, at %lld)\n", what,
               (long long)pre0, a, nspan, (long long)cap, (long long)at);
  std::exit(1);
}

void check(int64_t pre0, int a, int nspan, int64_t cap, int tile_slots) {
  const mrx::DecodeStorePlan pl = mrx::decode_store_plan(pre0, a, nspan, cap);
  ++g_cases;
  if (pl.odd != (int)((pre0 + a) & 1)) fail("odd is not the parity of the first span's cell", pre0, a, nspan, cap, pl.odd);
  if (pl.head < 0 || pl.head > 1 || pl.tail < 0 || pl.tail > 1 || pl.npairs < 0)
    fail("head and tail are single spans, pairs are counted", pre0, a, nspan, cap, pl.npairs);
  if (pl.head + 2 * pl.npairs + pl.tail != pl.nclip) fail("the parts do not add up to nclip", pre0, a, nspan, cap, pl.nclip);
  // the tile as the kernel fills it: slot k + odd holds span k; every other slot the sentinel
  std::vector<int32_t> tile((size_t)tile_slots, kSentinel);
  for (int k = 0; k < nspan; ++k) {
    if (k + pl.odd >= tile_slots) fail("a span has no slot in the tile", pre0, a, nspan, cap, k);
    tile[(size_t)(k + pl.odd)] = k;
  }
  // memory in span indices: exactly as long as the capacity (at least one cell, so that .data() is an object), every
  // store bounds-checked by hand AND by the sanitizer (the vector has no slack behind span_cap)
  const int64_t len = cap > 0 ? cap : 0;
  std::vector<int32_t> mem((size_t)len, kSentinel);
  std::vector<int> hits((size_t)len, 0);
  auto store1 = [&](int k) {
    const int64_t i = pre0 + k;
    if (i < pre0 || i >= len) fail("an 8-byte store outside [pre0, span_cap)", pre0, a, nspan, cap, i);
    mem[(size_t)i] = tile[(size_t)(k + pl.odd)];
    ++hits[(size_t)i];
  };
  auto store2 = [&](int k) {
    const int64_t i = pre0 + k;
    const int slot = k + pl.odd;
    if ((a + i) & 1) fail("a 16-byte store on an odd cell", pre0, a, nspan, cap, i);
    if (slot & 1) fail("a pair on an odd tile slot", pre0, a, nspan, cap, slot);
    if (i < pre0 || i + 1 >= len) fail("a 16-byte store outside [pre0, span_cap)", pre0, a, nspan, cap, i);
    if (slot + 1 >= tile_slots) fail("a pair read behind the tile", pre0, a, nspan, cap, slot);
    mem[(size_t)i] = tile[(size_t)slot];
    mem[(size_t)i + 1] = tile[(size_t)slot + 1];
    ++hits[(size_t)i];
    ++hits[(size_t)i + 1];
  };
  if (pl.head) store1(0);
  for (int p = 0; p < pl.npairs; ++p) store2(pl.head + 2 * p);
  if (pl.tail) store1(pl.head + 2 * pl.npairs);
  const int64_t end = pre0 + nspan < cap ? pre0 + nspan : cap;   // min(pre0 + nspan, span_cap)
  for (int64_t i = 0; i < len; ++i) {
    const bool inside = i >= pre0 && i < end;
    if (hits[(size_t)i] != (inside ? 1 : 0)) fail(inside ? "a span not written exactly once" : "a write outside the range", pre0, a, nspan, cap, i);
    if (mem[(size_t)i] != (inside ? (int32_t)(i - pre0) : kSentinel)) fail("the wrong span at an index", pre0, a, nspan, cap, i);
  }
  if (pl.nclip != (end > pre0 ? (int)(end - pre0) : 0)) fail("nclip is not the clipped count", pre0, a, nspan, cap, pl.nclip);
}

}  // namespace

int main() {
  for (int tile : {2048, 3072}) {
    std::vector<int> nspans = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, tile - 1, tile};
    for (int64_t pre0 : {int64_t(6), int64_t(7), (int64_t(1) << 31) + 2, (int64_t(1) << 31) + 3})
      for (int a = 0; a < 2; ++a)
        for (int nspan : nspans) {
          if (pre0 > 100 && nspan > 9) continue;   // (the large bases pin the 64-bit arithmetic; memory is modelled from 0)
          for (int64_t cap = pre0 - 1; cap <= pre0 + nspan + 1; ++cap) {
            if (pre0 > 100) {   // no 16 GiB model: the plan alone, against the plan of the same case at a small base
              const mrx::DecodeStorePlan big = mrx::decode_store_plan(pre0, a, nspan, cap);
              const int64_t small = 6 + (pre0 & 1);
              const mrx::DecodeStorePlan ref = mrx::decode_store_plan(small, a, nspan, cap - pre0 + small);
              ++g_cases;
              if (big.odd != ref.odd || big.head != ref.head || big.npairs != ref.npairs || big.tail != ref.tail ||
                  big.nclip != ref.nclip)
                fail("the plan depends on more than the parity of pre0", pre0, a, nspan, cap, 0);
            } else {
              check(pre0, a, nspan, cap, tile + 2);
            }
          }
        }
  }
  std::printf("decode_store_check: %ld cases ok\n", g_cases);
  return 0;
}
