// Host check of expand's record assembly (mojo_regex_amd/csrc/mrx_expand_bits.hpp: the segment walk expand_seek and the
// block assembly expand_block, on top of mrx_gather_bits.hpp) against a byte-by-byte build of the same records, meant
// for the host sanitizers: no kernel, no HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/expand_block_check.cpp -o expand_block_check && ./expand_block_check
//
// Seeded random cases: a buffer of texts, rows of up to 9 clamped groups (many of them empty), templates of 0 to 40
// segments with literals of 1 to 300 bytes, and the packed records written at each of the 16 output alignments the way
// k_expand_gather writes them -- wavefronts over contiguous runs of 16-byte blocks, 64 per round, one bisection per
// wavefront, a gallop per round, a bisection per lane between the round's bounds; blocks inside the output go out as
// one 16-byte store, the first and the last byte by byte.  Among the cases: runs of empty records (a template of
// groups only over rows without a byte), records longer than 64 blocks, an empty template, a template without
// references, and few wavefronts so that each runs many rounds.  The text buffer and the literal buffer are whole
// 16-byte words and not a byte more, as the read contract of include/mrx.h allows (the aligned words around a group's
// bytes and around a literal are read), so a read outside them is the sanitizer's to report.  Canaries in front of and
// behind the output must not change.
#include <hip/hip_runtime.h>   // (hipcc compiles this file as HIP: the header's host + device qualifiers)

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../mojo_regex_amd/csrc/mrx_expand_bits.hpp"

using namespace mrx;

namespace {

// out[0 .. bytes) as nw wavefronts of k_expand_gather assemble it, lane after lane: a sequential loop of this file's own
// with the arithmetic of the device's one walk (gather_blocks in mrx_gather_bits.hpp, device code: it takes its wavefront
// and lane from the launch) around the same fill, expand_block
void gather_records(const ExpandSrc& S, int64_t pieces, int64_t bytes, uint8_t* out, int64_t nw) {
  if (bytes <= 0) return;
  const uintptr_t ob = (uintptr_t)out, a0 = ob & ~(uintptr_t)15;
  const int64_t head = (int64_t)(ob - a0), nblk = (head + bytes + 15) >> 4;
  const int64_t per = ((nblk + nw - 1) / nw + 63) & ~(int64_t)63;
  for (int64_t w = 0; w < nw; ++w) {
    const int64_t b_begin = w * per, b_end = b_begin + per < nblk ? b_begin + per : nblk;
    if (b_begin >= b_end) continue;
    const int64_t p_first = b_begin * 16 - head;
    int64_t cur = gather_last_le(S.out_off, 0, pieces, p_first > 0 ? p_first : 0);
    for (int64_t b0 = b_begin; b0 < b_end; b0 += 64) {
      const int64_t bl = b0 + 63 < b_end ? b0 + 63 : b_end - 1;
      const int64_t pe = bl * 16 - head + 15, pl = pe < bytes ? pe : bytes - 1;
      const int64_t hi = gather_gallop(S.out_off, cur, pieces, pl);
      for (int64_t b = b0; b <= bl; ++b) {
        const int64_t p0 = b * 16 - head, pos = p0 > 0 ? p0 : 0, endp = p0 + 16 < bytes ? p0 + 16 : bytes;
        const int64_t r = gather_last_le(S.out_off, cur, hi + 1, pos);
        const g_u128 acc = expand_block(S, r, hi, p0, pos, endp);
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
  int empty_group_pct;   // how many of the groups have no byte
  int max_group;         // longest group
  bool lits;             // literals allowed
  const char* name;
};

int run_case(const Case& c, std::mt19937& rng, int* checked) {
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  // the texts: one buffer of whole 16-byte words, `shift` bytes of it in front of the first text
  const int shift = rnd(0, 15), ntexts = rnd(1, 6);
  std::vector<int64_t> tbase(ntexts), tlen(ntexts);
  int64_t at = shift;
  for (int i = 0; i < ntexts; ++i) {
    tbase[i] = at;
    tlen[i] = rnd(0, 2 * c.max_group + 3);
    at += tlen[i] + rnd(0, 5);
  }
  const size_t data_bytes = (size_t)(at > 0 ? (at + 15) / 16 * 16 : 16);
  uint8_t* data = (uint8_t*)aligned_alloc(16, data_bytes);
  for (size_t k = 0; k < data_bytes; ++k) data[k] = (uint8_t)((37 * k + 11) % 251);
  // the template
  const int nseg = rnd(c.min_segs, c.max_segs);
  std::vector<ExpandSeg> segs;
  std::vector<uint8_t> lits;
  for (int k = 0; k < nseg; ++k) {
    const bool lit = c.lits && (c.nslots == 0 || rng() % 2);
    if (lit && (segs.empty() || segs.back().slot >= 0)) {   // (the parser merges adjacent literals: none here either)
      const int len = rnd(1, c.max_lit);
      segs.push_back(ExpandSeg{(int64_t)lits.size(), len, -1, 0});
      for (int q = 0; q < len; ++q) lits.push_back((uint8_t)(0x80 | (rng() & 0x7F)));
    } else if (c.nslots > 0) {
      segs.push_back(ExpandSeg{0, 0, rnd(0, c.nslots - 1), 0});
    }
  }
  const size_t lit_bytes = lits.empty() ? 16 : (lits.size() + 15) / 16 * 16;
  uint8_t* dlits = (uint8_t*)aligned_alloc(16, lit_bytes);
  memset(dlits, 0x33, lit_bytes);
  if (!lits.empty()) memcpy(dlits, lits.data(), lits.size());
  // the rows: the source entry of each (text position, clamped pairs) and the record built byte by byte
  const int ns = c.nslots > 0 ? c.nslots : 1;
  std::vector<int64_t> base((size_t)c.rows), off{0};
  std::vector<int32_t> pairs((size_t)c.rows * ns * 2);
  std::vector<uint8_t> want;
  for (int r = 0; r < c.rows; ++r) {
    const int i = rnd(0, ntexts - 1);
    base[r] = tbase[i];
    for (int q = 0; q < c.nslots; ++q) {
      int32_t s = rnd(0, (int)tlen[i]), e = s;
      if (rnd(0, 99) >= c.empty_group_pct) e = s + rnd(0, (int)std::min<int64_t>(c.max_group, tlen[i] - s));
      pairs[((size_t)r * ns + q) * 2] = s;
      pairs[((size_t)r * ns + q) * 2 + 1] = e;
    }
    for (const ExpandSeg& sg : segs) {
      if (sg.slot < 0) {
        want.insert(want.end(), lits.begin() + sg.lit_off, lits.begin() + sg.lit_off + sg.lit_len);
      } else {
        const int32_t s = pairs[((size_t)r * ns + sg.slot) * 2], e = pairs[((size_t)r * ns + sg.slot) * 2 + 1];
        want.insert(want.end(), data + base[r] + s, data + base[r] + e);
      }
    }
    off.push_back((int64_t)want.size());
  }
  const int64_t bytes = off.back();
  // the walk on its own: every byte of the first records
  for (int r = 0; r < c.rows && r < 8; ++r)
    for (int64_t q = 0; q < off[r + 1] - off[r]; ++q) {
      int k;
      const int32_t* pr = pairs.data() + (size_t)r * ns * 2;
      const int64_t o = expand_seek(segs.data(), (int)segs.size(), pr, q, &k);
      int64_t before = 0;
      for (int j = 0; j < k; ++j) before += expand_seg_len(segs[j], pr);
      if (k >= (int)segs.size() || before + o != q || o >= expand_seg_len(segs[k], pr)) {
        printf("FAIL: %s: walk of record %d, byte %lld -> segment %d offset %lld\n", c.name, r, (long long)q, k, (long long)o);
        return 1;
      }
    }
  const ExpandSrc S{data, dlits, segs.data(), (int32_t)segs.size(), (int32_t)c.nslots, base.data(), pairs.data(), off.data()};
  for (int skew = 0; skew < 16; ++skew) {
    const size_t out_bytes = (size_t)((16 + skew + bytes + 16 + 15) / 16 * 16);
    uint8_t* buf = (uint8_t*)aligned_alloc(16, out_bytes);
    memset(buf, 0xA5, out_bytes);
    uint8_t* out = buf + 16 + skew;
    gather_records(S, c.rows, bytes, out, skew % 3 == 0 ? 1 : skew % 3 == 1 ? 3 : 64);
    if (bytes && memcmp(out, want.data(), (size_t)bytes) != 0) {
      printf("FAIL: %s: bytes differ (output skew %d)\n", c.name, skew);
      return 1;
    }
    for (size_t q = 0; q < out_bytes; ++q)
      if ((q < (size_t)(16 + skew) || q >= (size_t)(16 + skew + bytes)) && buf[q] != 0xA5) {
        printf("FAIL: %s: canary byte %zu changed (output skew %d)\n", c.name, q, skew);
        return 1;
      }
    free(buf);
    ++*checked;
  }
  free(dlits);
  free(data);
  return 0;
}

}  // namespace

int main() {
  const Case cases[] = {
      {300, 0, 40, 300, 9, 30, 40, true, "random"},
      {2000, 1, 6, 3, 3, 50, 2, true, "short records"},
      {1500, 1, 5, 1, 4, 97, 3, false, "runs of empty records"},
      {40, 6, 12, 300, 5, 10, 700, true, "records longer than 64 blocks"},
      {500, 40, 40, 1, 2, 40, 2, true, "40 segments of 0 to 2 bytes"},
      {700, 0, 0, 1, 0, 0, 0, true, "empty template"},
      {200, 1, 1, 300, 0, 0, 0, true, "no references"},
      {5000, 1, 3, 2, 2, 20, 6, true, "many rounds per wavefront"},
  };
  std::mt19937 rng(20260117);
  int checked = 0;
  for (int rep = 0; rep < 6; ++rep)
    for (const Case& c : cases)
      if (run_case(c, rng, &checked)) return 1;
  printf("ok: %d sweeps equal the byte-by-byte records, canaries intact\n", checked);
  return 0;
}
