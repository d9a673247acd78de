// 12-byte event records of the streaming findall: texts of at most kRec12MaxLen bytes at an aligned fixed pitch.
// A record is three dwords {F of the even group, F of the odd group, meta} for one PAIR of 16-byte groups (32 text
// bytes, pair p = bytes [32 p, 32 p + 32)).  Everything the 16-byte form keeps in two words fits one:
//   start   0..1023   10 bits   start of the walk alive when the pair begins
//   before  0..1023   10 bits   matches of the text before the pair (no empty matches: at most one per byte)
//   pair    0..32      6 bits   32 = the match that ends at byte 1024
//   lane    0..63      6 bits   the text within its wavefront (top bits, where the 16-byte form has it)
// Shared by the kernels and the host round-trip hook (mrx_testing_rec12_roundtrip), so the packing is pinned without a GPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRX_REC12_HD __host__ __device__ inline
#else
#define MRX_REC12_HD inline
#endif

namespace mrx {

constexpr int kRec12MaxLen = 1024;
constexpr int kRec12StartBits = 10, kRec12BeforeBits = 10, kRec12PairBits = 6, kRec12LaneBits = 6;
constexpr int kRec12BeforeShift = kRec12StartBits;
constexpr int kRec12PairShift = kRec12BeforeShift + kRec12BeforeBits;
constexpr int kRec12LaneShift = kRec12PairShift + kRec12PairBits;
static_assert(kRec12LaneShift + kRec12LaneBits == 32, "the four fields fill one dword");
static_assert(kRec12LaneShift == 26, "lane sits where the 16-byte records have it");
static_assert(kRec12MaxLen - 1 < (1 << kRec12StartBits), "a walk starts at a byte of the text");
static_assert(kRec12MaxLen - 1 < (1 << kRec12BeforeBits), "at most one match per byte, the last one not before itself");
static_assert(kRec12MaxLen / 32 < (1 << kRec12PairBits), "pair of the match that ends at the last byte's end");
static_assert(63 < (1 << kRec12LaneBits), "64 texts per wavefront");

MRX_REC12_HD uint32_t rec12_pack(uint32_t start, uint32_t pair, uint32_t lane, uint32_t before) {
  return start | (before << kRec12BeforeShift) | (pair << kRec12PairShift) | (lane << kRec12LaneShift);
}
MRX_REC12_HD int rec12_start(uint32_t m) { return (int)(m & ((1u << kRec12StartBits) - 1u)); }
MRX_REC12_HD int rec12_before(uint32_t m) { return (int)((m >> kRec12BeforeShift) & ((1u << kRec12BeforeBits) - 1u)); }
MRX_REC12_HD int rec12_pair(uint32_t m) { return (int)((m >> kRec12PairShift) & ((1u << kRec12PairBits) - 1u)); }
MRX_REC12_HD int rec12_lane(uint32_t m) { return (int)(m >> kRec12LaneShift); }

// slots (of 12 bytes) a text can fill: a record per pair that holds a byte of the text or the byte behind it, plus the
// match that ends with the text
MRX_REC12_HD int64_t rec12_row_len(int64_t max_len) { return max_len / 32 + 2; }

}  // namespace mrx
