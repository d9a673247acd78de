// Lines (include/mrx.h, "lines"): a text's bytes cut at one separator byte.  Host and device code: the walk of one aligned
// 16-byte block of a text is what k_lines_count and k_lines_emit run per lane (mrx_lines.hip), and what
// mrx_debug_lines_host and tools/lines_check.cpp run on the CPU, block after block over the same pieces.
//
// Pieces.  A text is cut into pieces of P bytes (a multiple of kLinesRound); a wavefront takes a piece in rounds of
// kLinesRound bytes, a lane the 16 bytes at text position p + 16 * lane of each.  Two passes over the pieces:
//   count   per piece: its separators, its kept bytes (an unterminated tail counted as kept) and the bytes behind its
//           last separator; exclusive scans of the first two
//   text    per text, from the scans at its first piece and at the next text's: its tail (the piece with its last
//           separator is a bisection of the scan), its lines and its output bytes; exclusive scans of those two are the
//           line prefix and every text's first output byte
//   emit    per piece: line index and output position of its first byte from the scans, then per block the line ends
//           (offsets and owners) and the kept bytes
// A line end is a separator, or a text's last byte when it is no separator and tails are kept.  Line j's end writes
// out_offsets[j + 1] and owner[j]: every entry has exactly one writer, whatever runs first.
//
// Reading.  lines_block loads the aligned 16-byte words that hold a byte of its block inside the text and, under CRLF,
// the word of the byte behind a '\r' that is the block's last byte when that byte is text too.  Bytes of those words
// outside the text are masked before anything looks at them.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mrx.h"
#include "mrx_gather_bits.hpp"

namespace mrx {

constexpr int64_t kLinesRound = 1024;   // 64 lanes x 16 bytes
// The piece without a pin (mrx_debug_lines_piece).  The first and the last output block of a piece are shared with its
// neighbours and go out byte by byte; a longer piece has fewer of them and fewer scan entries, a shorter one more
// wavefronts on a short batch (profiles/lines.md).
constexpr int64_t kLinesPiece = 4096;
constexpr uint32_t kLinesFlags = MRX_LINES_KEEPENDS | MRX_LINES_CRLF | MRX_LINES_DROP_PARTIAL;

// first byte and length of text i, 64-bit (a CSR text may have 2^31 bytes or more; a length below 0 counts as 0)
MRX_HD const uint8_t* lines_text(const TextBatch& B, int64_t i, int64_t* L) {
  if (B.offsets) {
    const int64_t a = B.offsets[i], l = B.offsets[i + 1] - a;
    *L = l > 0 ? l : 0;
    return B.data + a;
  }
  const int64_t l = B.lens ? B.lens[i] : B.len;
  *L = l > 0 ? l : 0;
  return B.data + i * B.stride;
}
MRX_HD int64_t lines_pieces_of(int64_t L, int64_t P) { return (L + P - 1) / P; }

// bit k: byte k of w equals b.  Exact: no carry leaves a byte (the high bits are masked out of the sum)
MRX_HD uint32_t lines_eq8(uint64_t w, uint32_t b) {
  const uint64_t low7 = 0x7f7f7f7f7f7f7f7full;
  const uint64_t y = w ^ (0x0101010101010101ull * (uint64_t)(b & 255u));
  const uint64_t z = ~(((y & low7) + low7) | y | low7);   // 0x80 where the byte of y is zero
  return (uint32_t)(((z >> 7) * 0x0102040810204080ull) >> 56);
}
MRX_HD uint32_t lines_eq16(g_u128 x, uint32_t b) { return lines_eq8((uint64_t)x, b) | (lines_eq8((uint64_t)(x >> 64), b) << 8); }
MRX_HD int lines_popc(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(m);
#else
  return __builtin_popcount(m);
#endif
}

// one block: 16-bit masks over its bytes
struct LinesBlock {
  g_u128 bytes;
  uint32_t sep;    // separators
  uint32_t keep;   // bytes that go to the output
  uint32_t ends;   // line ends
};
MRX_HD LinesBlock lines_no_block() { return LinesBlock{0, 0, 0, 0}; }

// The block at text position q0 (a multiple of 16, 0 <= q0 < L) of the text of L bytes at tp.  limit: the first
// position that is not kept whatever it holds (L, or the start of a dropped tail).
MRX_HD LinesBlock lines_block(const uint8_t* tp, int64_t L, int64_t q0, int64_t limit, uint32_t sep, uint32_t flags) {
  LinesBlock b;
  const int v = L - q0 < 16 ? (int)(L - q0) : 16;
  const uint32_t valid = (1u << v) - 1u;
  b.bytes = gather_window(tp + q0, v);
  b.sep = lines_eq16(b.bytes, sep) & valid;
  uint32_t drop = (flags & MRX_LINES_KEEPENDS) ? 0u : b.sep;
  if (flags & MRX_LINES_CRLF) {
    const uint32_t cr = lines_eq16(b.bytes, '\r') & valid;
    uint32_t lf_next = b.sep >> 1;
    if ((cr >> 15) && q0 + 16 < L && ((uint32_t)gather_window(tp + q0 + 16, 1) & 255u) == sep) lf_next |= 0x8000u;
    drop |= cr & lf_next;
  }
  const int64_t room = limit - q0;
  const uint32_t inside = room >= 16 ? 0xffffu : room <= 0 ? 0u : (1u << (int)room) - 1u;
  b.keep = valid & ~drop & inside;
  b.ends = b.sep;
  if (!(flags & MRX_LINES_DROP_PARTIAL) && q0 + v == L && !((b.sep >> (v - 1)) & 1u)) b.ends |= 1u << (v - 1);
  return b;
}
// kept bytes of a block up to and including its byte k: where the line that ends at k ends in the output
MRX_HD int lines_kept_through(const LinesBlock& b, int k) { return lines_popc(b.keep & ((2u << k) - 1u)); }

// a text's tail from the pass over its pieces [a, b) (b > a: the text is not empty): the piece with the last separator
// is the last one whose scan is below the scan at b
MRX_HD int64_t lines_tail(const int64_t* __restrict__ sep_scan, const int64_t* __restrict__ after, int64_t a, int64_t b,
                          int64_t L, int64_t P) {
  if (sep_scan[b] == sep_scan[a]) return L;
  const int64_t p = gather_last_le(sep_scan, a, b, sep_scan[b] - 1);
  const int64_t end = (p - a + 1) * P;
  return after[p] + (L > end ? L - end : 0);
}

// ---- host only: the passes, piece by piece as the kernels take them --------------------------------------------------
struct LinesHostOut {
  int64_t* line_prefix;   // [n + 1]
  int64_t* owner;         // [piece_cap]
  int64_t* out_offsets;   // [piece_cap + 1]
  int64_t piece_cap;
  uint8_t* out_data;
  int64_t out_cap;
  int64_t* totals;        // [4]
};

// Text i is data[off[i], off[i + 1]); the aligned 16-byte words around every text must be readable.  Writes what the
// contract of mrx_lines_dev says is written, under its capacity rules, and nothing else.
inline void lines_host(const uint8_t* data, const int64_t* off, int64_t n, int64_t P, uint32_t sep, uint32_t flags,
                       const LinesHostOut& o) {
  const TextBatch B = csr(data, off);
  const bool drop_tail = (flags & MRX_LINES_DROP_PARTIAL) != 0;
  std::vector<int64_t> first((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    int64_t L;
    (void)lines_text(B, i, &L);
    first[(size_t)i + 1] = first[(size_t)i] + lines_pieces_of(L, P);
  }
  const int64_t np = first[(size_t)n];
  std::vector<int64_t> sep_scan((size_t)np + 1, 0), kept_scan((size_t)np + 1, 0), after((size_t)np + 1, 0);
  for (int64_t i = 0; i < n; ++i) {   // count
    int64_t L;
    const uint8_t* tp = lines_text(B, i, &L);
    for (int64_t p = first[(size_t)i]; p < first[(size_t)i + 1]; ++p) {
      const int64_t p0 = (p - first[(size_t)i]) * P, pend = p0 + P < L ? p0 + P : L;
      int64_t nsep = 0, kept = 0, last = -1;
      for (int64_t q0 = p0; q0 < pend; q0 += 16) {
        const LinesBlock b = lines_block(tp, L, q0, L, sep, flags);
        nsep += lines_popc(b.sep);
        kept += lines_popc(b.keep);
        if (b.sep) last = q0 - p0 + (31 - __builtin_clz(b.sep));
      }
      sep_scan[(size_t)p + 1] = sep_scan[(size_t)p] + nsep;
      kept_scan[(size_t)p + 1] = kept_scan[(size_t)p] + kept;
      after[(size_t)p] = (pend - p0) - (last + 1);
    }
  }
  std::vector<int64_t> tails((size_t)n + 1, 0), base((size_t)n + 1, 0);
  o.line_prefix[0] = 0;
  for (int64_t i = 0; i < n; ++i) {   // text
    int64_t L;
    (void)lines_text(B, i, &L);
    const int64_t a = first[(size_t)i], b = first[(size_t)i + 1];
    const int64_t tail = L > 0 ? lines_tail(sep_scan.data(), after.data(), a, b, L, P) : 0;
    tails[(size_t)i] = tail;
    o.line_prefix[i + 1] = o.line_prefix[i] + (sep_scan[(size_t)b] - sep_scan[(size_t)a]) + (!drop_tail && tail > 0 ? 1 : 0);
    base[(size_t)i + 1] = base[(size_t)i] + (kept_scan[(size_t)b] - kept_scan[(size_t)a]) - (drop_tail ? tail : 0);
  }
  const int64_t lines = o.line_prefix[n], bytes = base[(size_t)n];
  o.totals[0] = lines;
  o.totals[1] = bytes;
  o.totals[2] = 0;
  o.totals[3] = n > 0 ? tails[(size_t)n - 1] : 0;
  if (lines > o.piece_cap) return;
  const bool move = bytes <= o.out_cap;
  o.out_offsets[0] = 0;
  for (int64_t i = 0; i < n; ++i) {   // emit
    int64_t L;
    const uint8_t* tp = lines_text(B, i, &L);
    const int64_t limit = L - (drop_tail ? tails[(size_t)i] : 0);
    for (int64_t p = first[(size_t)i]; p < first[(size_t)i + 1]; ++p) {
      const int64_t p0 = (p - first[(size_t)i]) * P, pend = p0 + P < L ? p0 + P : L;
      int64_t line = o.line_prefix[i] + (sep_scan[(size_t)p] - sep_scan[(size_t)first[(size_t)i]]);
      int64_t pos = base[(size_t)i] + (kept_scan[(size_t)p] - kept_scan[(size_t)first[(size_t)i]]);
      for (int64_t q0 = p0; q0 < pend; q0 += 16) {
        const LinesBlock b = lines_block(tp, L, q0, limit, sep, flags);
        for (uint32_t m = b.ends; m; m &= m - 1) {
          o.out_offsets[line + 1] = pos + lines_kept_through(b, __builtin_ctz(m));
          o.owner[line++] = i;
        }
        for (int k = 0; k < 16; ++k)
          if ((b.keep >> k) & 1u) {
            if (move) o.out_data[pos] = (uint8_t)(b.bytes >> (8 * k));
            ++pos;
          }
      }
    }
  }
  for (int64_t j = 0; j < lines; ++j)
    if (o.out_offsets[j + 1] - o.out_offsets[j] > o.totals[2]) o.totals[2] = o.out_offsets[j + 1] - o.out_offsets[j];
}

}  // namespace mrx
