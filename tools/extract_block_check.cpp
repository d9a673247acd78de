// Host check of the byte movers' block assembly (mojo_regex_amd/csrc/mrx_gather_bits.hpp: window, mask, shift, or-in,
// the aligned 16-byte store) against memcpy, meant for the host sanitizers: no kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/extract_block_check.cpp -o extract_block_check && ./extract_block_check
//
// One text of 200 bytes, pieces of lengths 0, 1, 15, 16, 17, 31, 32, 33 and 47 at each source offset 0..15, written at
// each of the 16 output alignments the way k_extract_gather writes them: every 16-byte block aligned on the output
// address is assembled from the pieces that overlap it; blocks inside the output go out as one 16-byte store, the first
// and the last byte by byte.  Source and output buffers are rounded to 16 bytes, as the read contract of include/mrx.h
// requires (the aligned words around a piece are read).  Canaries in front of and behind the output must not change.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the header's host + device qualifiers)

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_gather_bits.hpp"

using namespace mrx;

namespace {

struct Piece { int64_t src, len; };

// the blocks of out[0 .. bytes) as the kernel's lanes assemble them, one after the other: a sequential loop of this
// file's own around the same block assembly (the device's one walk, gather_blocks in mrx_gather_bits.hpp, is device code:
// it takes its wavefront and lane from the launch)
void blocks_in_turn(const uint8_t* data, const std::vector<Piece>& pieces, const std::vector<int64_t>& off, uint8_t* out,
                   int64_t bytes) {
  const int64_t n = (int64_t)pieces.size();
  const uintptr_t ob = (uintptr_t)out, a0 = ob & ~(uintptr_t)15;
  const int64_t head = (int64_t)(ob - a0), nblk = (head + bytes + 15) >> 4;
  for (int64_t b = 0; b < nblk; ++b) {
    const int64_t p0 = b * 16 - head, endp = p0 + 16 < bytes ? p0 + 16 : bytes;
    int64_t pos = p0 > 0 ? p0 : 0;
    int64_t r = gather_last_le(off.data(), 0, n, pos);
    g_u128 acc = 0;
    while (true) {
      const int64_t s = off[r], e = off[r + 1];
      const int take = (int)((e < endp ? e : endp) - pos);
      acc = gather_place(acc, data + pieces[r].src + (pos - s), take, (int)(pos - p0));
      pos += take;
      if (pos >= endp) break;
      r = gather_last_le(off.data(), r + 1, n, pos);
    }
    uint8_t* dst = (uint8_t*)(a0 + (uintptr_t)b * 16);
    if (p0 >= 0 && p0 + 16 <= bytes) {
      gather_store16(dst, acc);
    } else {
      for (int q = p0 < 0 ? (int)-p0 : 0; q < (int)(endp - p0); ++q) dst[q] = (uint8_t)(acc >> (8 * q));
    }
  }
}

}  // namespace

int main() {
  const int kText = 200, kLens[] = {0, 1, 15, 16, 17, 31, 32, 33, 47};
  // the text at four alignments of its own too (0, 5, 10, 15): a buffer of whole 16-byte words with the text `shift`
  // bytes in
  int checked = 0;
  for (int shift = 0; shift < 16; shift += 5) {
    const size_t src_bytes = (size_t)((shift + kText + 15) / 16 * 16);
    uint8_t* src = (uint8_t*)aligned_alloc(16, src_bytes);
    memset(src, 0x5A, src_bytes);
    for (int k = 0; k < kText; ++k) src[shift + k] = (uint8_t)((37 * k + 11) % 251);
    std::vector<Piece> pieces;
    std::vector<int64_t> off{0};
    std::vector<uint8_t> want;
    for (int s = 0; s < 16; ++s)
      for (int len : kLens) {
        pieces.push_back(Piece{shift + s, len});
        off.push_back(off.back() + len);
        want.insert(want.end(), src + shift + s, src + shift + s + len);
      }
    const int64_t bytes = off.back();
    for (int skew = 0; skew < 16; ++skew) {
      const size_t out_bytes = (size_t)((16 + skew + bytes + 16 + 15) / 16 * 16);
      uint8_t* buf = (uint8_t*)aligned_alloc(16, out_bytes);
      memset(buf, 0xA5, out_bytes);
      uint8_t* out = buf + 16 + skew;
      blocks_in_turn(src, pieces, off, out, bytes);
      if (memcmp(out, want.data(), (size_t)bytes) != 0) {
        printf("FAIL: bytes differ (text shift %d, output skew %d)\n", shift, skew);
        return 1;
      }
      for (size_t q = 0; q < out_bytes; ++q)
        if ((q < (size_t)(16 + skew) || q >= (size_t)(16 + skew + bytes)) && buf[q] != 0xA5) {
          printf("FAIL: canary byte %zu changed (text shift %d, output skew %d)\n", q, shift, skew);
          return 1;
        }
      free(buf);
      ++checked;
    }
    free(src);
  }
  printf("ok: %d sweeps of 144 pieces equal memcpy, canaries intact\n", checked);
  return 0;
}
