// regex.sub on the device (gfx950 / CDNA4), in three routes:
//   k_subs_*   streamable plans with a replacement of one length: the output assembled from findall's spans
//   k_subc_*   \1..\9 on a deterministic chain: the plain search's spans, groups from the leaves' runs
//   k_sub      everything else: sub_text()'s loop (mrx_device.hpp), one lane per text, sizes and then bytes
// The regex kernels underneath (findall, the literal prefilter, the prefix sums) are mrx_kernels.hip's, reached
// through mrx_core.hpp.
#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "mrx_core.hpp"
#include "../../include/mrx_testing.h"
#include "mrx_chain_dev.hpp"
#include "mrx_lookback.hpp"
#include "mrx_wave_bits.hpp"

using namespace mrx;

namespace {
// ---- sub() -------------------------------------------------------------------------
struct SizeSink {
  int64_t n = 0;
  __device__ __forceinline__ void bytes(const uint8_t*, int k) { n += k; }
};
struct WriteSink {
  uint8_t* out;
  int64_t pos, cap;
  __device__ __forceinline__ void bytes(const uint8_t* src, int k) {
    if (pos + k > cap || k < 24) {   // clipped at the buffer's end, or short: byte by byte
      for (int j = 0; j < k; ++j)
        if (pos + j < cap) out[pos + j] = src[j];
      pos += k;
      return;
    }
    // A long piece (the text between two matches): aligned 8-byte stores; the source word for each is put
    // together from the two aligned words that hold its bytes (every word read holds at least one byte of the piece)
    uint8_t* d = out + pos;
    int j = 0;
    while ((uintptr_t)(d + j) & 7) { d[j] = src[j]; ++j; }
    const uintptr_t sa = (uintptr_t)(src + j);
    const uint64_t* sp = (const uint64_t*)(sa & ~(uintptr_t)7);
    const int sh = (int)(sa & 7) * 8;
    if (sh) {
      uint64_t lo = *sp;
      for (; j + 8 <= k; j += 8) {
        const uint64_t hi = *++sp;   // (holds the chunk's last sh / 8 bytes)
        *(uint64_t*)(d + j) = (lo >> sh) | (hi << (64 - sh));
        lo = hi;
      }
    } else {
      for (; j + 8 <= k; j += 8) *(uint64_t*)(d + j) = *sp++;
    }
    for (; j < k; ++j) d[j] = src[j];
    pos += k;
  }
};

// ---- sub() from findall spans (streamable plans) -----------------------------------------
// For plans whose findall runs on the streaming kernel, regex.sub is assembled from the CSR spans:
// the first `count` matches of a text (all when count == 0) are replaced, matches are never empty,
// and the replacement has a fixed length R (literal, or template over fixed-width groups), so
//   out position of replacement m:  rstart(m) = s_m - cum_m + m * R     (cum_m = matched bytes before m)
// k_subs_sizes: one lane per text -> output length and cum_m per span.
__global__ __launch_bounds__(kBlock) void k_subs_sizes(int64_t n, const int64_t* __restrict__ offsets,
                                                       const int64_t* __restrict__ prefix,
                                                       const int32_t* __restrict__ spans, long long count,
                                                       int R, int64_t* __restrict__ sizes,
                                                       int32_t* __restrict__ cum, int64_t span_cap,
                                                       const int32_t* __restrict__ left) {
  // 16 lanes per text: coalesced span loads, prefix sum of the match lengths inside the group
  if (prefix[n] > span_cap) return;   // the findall in front did not have room for its spans: the host retries
  if (left && *left == 0) return;     // cum[] is wanted for the texts k_subs_wave left over: there are none
  constexpr int G = 16;
  const int lane = threadIdx.x & (G - 1);
  const int64_t ngroups = (int64_t)gridDim.x * (blockDim.x / G);
  for (int64_t i = (int64_t)blockIdx.x * (blockDim.x / G) + (threadIdx.x / G); i < n; i += ngroups) {
    const int64_t a = prefix[i];
    int64_t k = prefix[i + 1] - a;
    if (count > 0 && k > count) k = count;
    int carry = 0;
    for (int64_t m0 = 0; m0 < k; m0 += G) {
      const int64_t m = m0 + lane;
      int len = 0;
      if (m < k) {
        const int2 sp = *(const int2*)(spans + 2 * (a + m));
        len = sp.y - sp.x;
      }
      int incl = len;
#pragma unroll
      for (int d = 1; d < G; d <<= 1) {
        const int v = __shfl_up(incl, d, G);
        if (lane >= d) incl += v;
      }
      if (m < k) cum[a + m] = carry + incl - len;
      carry += __shfl(incl, G - 1, G);
    }
    if (lane == 0 && sizes) sizes[i] = (offsets[i + 1] - offsets[i]) - carry + k * (int64_t)R;
  }
}

// k_subs_sizes_flat (count == 0: every match is replaced): output length of every text without a dependent
// round trip per text.  A wavefront owns 64 consecutive texts, whose spans are one contiguous range of the
// CSR; it streams that range 256 spans at a time, keeps the running sum of the match lengths, and lane t
// picks the sum's value at its text's first and one-past-last span as they pass (two cross-lane reads per
// 64 spans).  cum[] -- matched bytes before each match, which only k_subs_emit reads -- is not written here.
__global__ __launch_bounds__(kBlock) void k_subs_sizes_flat(int64_t n, const int64_t* __restrict__ offsets,
                                                            const int64_t* __restrict__ prefix,
                                                            const int32_t* __restrict__ spans, int R,
                                                            int64_t* __restrict__ sizes, int64_t span_cap) {
  if (prefix[n] > span_cap) return;   // as k_subs_sizes
  const int lane = threadIdx.x & 63;
  const int64_t nw = (n + 63) / 64;
  for (int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64; w < nw; w += (int64_t)gridDim.x * (kBlock / 64)) {
    const int64_t i = w * 64 + lane;
    const bool live = i < n;
    const int64_t pa = live ? prefix[i] : 0, pb = live ? prefix[i + 1] : 0;
    const int64_t tbytes = live ? offsets[i + 1] - offsets[i] : 0;
    const int64_t i_last = (w * 64 + 64 < n ? w * 64 + 64 : n);
    const int64_t A = __shfl(pa, 0), B = prefix[i_last];
    int run = 0;                 // matched bytes of spans [A, c), modulo 2^32 (differences are what is used)
    int at_a = 0, at_b = 0;      // the running sum in front of span pa / pb (both 0 while pa == A / pb == A)
    for (int64_t c = A; c < B; c += 256) {
      int len[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t m = c + 64 * j + lane;
        int2 sp = make_int2(0, 0);
        if (m < B) sp = *(const int2*)(spans + 2 * m);
        len[j] = sp.y - sp.x;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t c0 = c + 64 * j;
        const int incl = (int)((uint32_t)run + (uint32_t)group_scan<64, false>(len[j]));   // sum of spans [A, c0 + lane]
        // the sum in front of span x, x in (c0, c0 + 64]: lane x - 1 - c0 holds it
        const int64_t ja = pa - 1 - c0, jb = pb - 1 - c0;
        const int va = __shfl(incl, (int)(ja & 63)), vb = __shfl(incl, (int)(jb & 63));
        if (ja >= 0 && ja < 64) at_a = va;
        if (jb >= 0 && jb < 64) at_b = vb;
        run = __shfl(incl, 63);
      }
    }
    if (live) sizes[i] = tbytes - (int64_t)((uint32_t)at_b - (uint32_t)at_a) + (pb - pa) * (int64_t)R;
  }
}

// k_subs_emit: one wavefront per text, output centric.  Each lane produces one 16-byte block of
// the output (aligned on the output ADDRESS, so full blocks are single coalesced 16-byte stores),
// finds by binary search which replacement precedes its first byte and then walks: replacement
// bytes come from rmap (literal byte, or 0x8000 | offset into the match for a group byte), kept
// bytes from the input through an 8-byte register window.
constexpr int kSubsStage = 128;  // replacements per text staged in LDS (more: read from global)
constexpr int kSubsLanes = 16;   // lanes that share one text in k_subs_emit

// bytes src .. src+15 of a text as two little-endian u64 (bytes past the text are unspecified but
// never fetched from beyond the aligned word that holds the text's last byte)
__device__ __forceinline__ void load16(const uint8_t* base, int len, int src, uint64_t& lo, uint64_t& hi) {
  const uintptr_t addr = (uintptr_t)(base + src);
  const uint64_t* w = (const uint64_t*)(addr & ~(uintptr_t)7);
  const uint64_t* last = (const uint64_t*)(((uintptr_t)(base + len - 1)) & ~(uintptr_t)7);  // len > 0
  const uint64_t w0 = w <= last ? w[0] : 0, w1 = w + 1 <= last ? w[1] : 0, w2 = w + 2 <= last ? w[2] : 0;
  const int sh = (int)(addr & 7) * 8;
  if (sh == 0) { lo = w0; hi = w1; }
  else { lo = (w0 >> sh) | (w1 << (64 - sh)); hi = (w1 >> sh) | (w2 << (64 - sh)); }
}

// G = 16: 16 lanes share a text and its replacements are staged whole (up to kSubsStage, more: read
// from global).  G = kBlock (long texts): a whole workgroup shares a text, and every round -- G output
// blocks = 4 KiB of output -- stages the window of replacements that can touch it (the last one
// starting at or before the round's first byte, and the kSubsWindow - 1 after it).
constexpr int kSubsWindow = 512;
// texts k_subs_wave<G> takes (the rest is k_subs_emit's): frame and output fit the group's LDS tiles
__host__ __device__ inline bool subs_wave_takes(int G, int tlen, int mis, int olen, int head) {
  return tlen + mis <= 32 * G + 16 && olen + head <= 64 * G;
}
template <int G>
__global__ __launch_bounds__(kBlock) void k_subs_emit(int64_t n, const uint8_t* __restrict__ data,
                                                      const int64_t* __restrict__ offsets,
                                                      const int64_t* __restrict__ prefix,
                                                      const int32_t* __restrict__ spans,
                                                      const int32_t* __restrict__ cum, long long count,
                                                      int R, const uint16_t* __restrict__ rmap,
                                                      const int64_t* __restrict__ out_off,
                                                      uint8_t* __restrict__ out, int skip_g,
                                                      const int32_t* __restrict__ left) {
  // `left`: k_subs_wave<skip_g> in front took every text (skip_g != 0), or the host's go-ahead behind the totals
  // (k_subs_gate: the kernel is enqueued before the host has seen them) says no
  if (left && *left == 0) return;
  // kSubsLanes lanes share one text (4 texts per wavefront): a 1 KiB text has ~70 output blocks,
  // which 64 lanes cover in two half-empty rounds; 16 lanes cover them in five full ones, and the
  // four texts' dependent round trips (offsets -> spans -> bytes) overlap.
  constexpr bool WIN = G != kSubsLanes;
  constexpr int STAGE = WIN ? kSubsWindow : kSubsStage;
  static_assert(G == kSubsLanes || G == kBlock, "a group is 16 lanes or the workgroup");
  __shared__ int3 stage_all[kBlock / G][STAGE];  // {rstart, match start, match end}
  extern __shared__ __align__(16) uint8_t subs_dyn[];   // the replacement map (R u16 entries)
  uint16_t* rmap_lds = (uint16_t*)subs_dyn;
  for (int r = threadIdx.x; r < R; r += blockDim.x) rmap_lds[r] = rmap[r];
  __syncthreads();
  auto group_sync = [&]() {
    if (WIN) __syncthreads();
    else {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  };
  const int lane = threadIdx.x & (G - 1);   // lane within the group that owns the text
  int3* stage = stage_all[threadIdx.x / G];
  const int64_t ngroups = (int64_t)gridDim.x * (blockDim.x / G);
  for (int64_t i = (int64_t)blockIdx.x * (blockDim.x / G) + (threadIdx.x / G); i < n; i += ngroups) {
    const int64_t ibase = offsets[i];
    const uint8_t* tptr = data + ibase;
    const int tlen = (int)(offsets[i + 1] - ibase);
    const int64_t a = prefix[i];
    int64_t k64 = prefix[i + 1] - a;
    if (count > 0 && k64 > count) k64 = count;
    const int k = (int)k64;
    const int64_t obase = out_off[i];
    const int olen = (int)(out_off[i + 1] - obase);
    if (olen <= 0) continue;
    if (skip_g && subs_wave_takes(skip_g, tlen, (int)((uintptr_t)tptr & 15), olen, (int)((uintptr_t)(out + obase) & 15)))
      continue;   // k_subs_wave<skip_g> wrote this text
    const int32_t* sp = spans + 2 * a;
    const int32_t* cm = cum + a;
    const bool staged = !WIN && k <= STAGE;
    auto repl_global = [&](int m) {  // {rstart, match start, match end} of replacement m
      const int2 se = *(const int2*)(sp + 2 * m);
      return make_int3(se.x - cm[m] + m * R, se.x, se.y);
    };
    group_sync();
    if (staged) {
      for (int m = lane; m < k; m += G) stage[m] = repl_global(m);
      group_sync();
    }
    int wbase = 0, wcnt = 0;   // WIN: replacements [wbase, wbase + wcnt) are staged
    auto repl_at = [&](int m) {
      if (staged) return stage[m];
      if (WIN && m >= wbase && m < wbase + wcnt) return stage[m - wbase];
      return repl_global(m);
    };
    const int head = (int)((uintptr_t)(out + obase) & 15);  // output starts `head` bytes into its first 16-byte block
    for (int blk = 0; blk * 16 < head + olen; blk += G) {
      if (WIN) {
        group_sync();   // everyone is done with the previous window
        const int w_lo = blk * 16 - head < 0 ? 0 : blk * 16 - head;   // first output position of this round
        int lo = -1, hi = k;
        while (hi - lo > 1) {   // same addresses in every lane: one broadcast load per step
          const int mid = (lo + hi) >> 1;
          if (repl_global(mid).x <= w_lo) lo = mid; else hi = mid;
        }
        wbase = lo < 0 ? 0 : lo;
        wcnt = k - wbase < STAGE ? k - wbase : STAGE;
        for (int m = lane; m < wcnt; m += G) stage[m] = repl_global(wbase + m);
        group_sync();
      }
      const int p_lo = (blk + lane) * 16 - head;   // first output position of my block (may be < 0)
      int p = p_lo < 0 ? 0 : p_lo;
      const int p_hi = p_lo + 16 < olen ? p_lo + 16 : olen;
      if (p >= p_hi) continue;
      // j = last replacement with rstart(j) <= p, or -1
      int lo = -1, hi = k;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (repl_at(mid).x <= p) lo = mid; else hi = mid;
      }
      int j = lo;
      int3 cur = j >= 0 ? repl_at(j) : make_int3(0, 0, 0);
      int nxt = j + 1 < k ? repl_at(j + 1).x : 0x7FFFFFFF;
      uint64_t wlo = 0, whi = 0;   // the 16 output bytes
      // OR `cnt` (1..16) bytes of (vlo, vhi) into the block at byte offset q
      auto put = [&](uint64_t vlo, uint64_t vhi, int q, int cnt) {
        if (cnt < 8) { vlo &= (1ull << (cnt * 8)) - 1; vhi = 0; }
        else if (cnt < 16) { vhi &= (cnt == 8) ? 0ull : ((1ull << ((cnt - 8) * 8)) - 1); }
        if (q == 0) { wlo |= vlo; whi |= vhi; }
        else if (q < 8) { wlo |= vlo << (q * 8); whi |= (vhi << (q * 8)) | (vlo >> (64 - q * 8)); }
        else if (q == 8) { whi |= vlo; }
        else { whi |= vlo << ((q - 8) * 8); }
      };
      while (p < p_hi) {
        while (p == nxt) {   // several replacements can start here when R == 0 and matches touch
          ++j;
          cur = repl_at(j);
          nxt = j + 1 < k ? repl_at(j + 1).x : 0x7FFFFFFF;
        }
        if (j >= 0 && p < cur.x + R) {   // replacement bytes: literal, or group bytes of the match
          int stop = cur.x + R < p_hi ? cur.x + R : p_hi;
          if (nxt < stop) stop = nxt;
          uint64_t mlo, mhi;
          load16(tptr, tlen, cur.y, mlo, mhi);   // the first 16 bytes of the match
          for (; p < stop; ++p) {
            const uint32_t r = rmap_lds[p - cur.x];
            int b = (int)r;
            if (r & 0x8000u) {
              const int o = (int)(r & 0x7FFFu);
              b = o < 16 ? (int)(((o < 8 ? mlo : mhi) >> ((o & 7) * 8)) & 0xFFu) : (int)tptr[cur.y + o];
            }
            put((uint64_t)(uint32_t)b, 0, p - p_lo, 1);
          }
        } else {                          // kept input bytes up to the next replacement: one 16-byte fetch
          const int src = j >= 0 ? p - (cur.x + R) + cur.z : p;
          const int stop = nxt < p_hi ? nxt : p_hi;
          uint64_t vlo, vhi;
          load16(tptr, tlen, src, vlo, vhi);
          put(vlo, vhi, p - p_lo, stop - p);
          p = stop;
        }
      }
      uint8_t* dst = out + (obase + p_lo);
      if (p_lo >= 0 && p_lo + 16 <= olen) {
        *(uint4*)dst = make_uint4((uint32_t)wlo, (uint32_t)(wlo >> 32), (uint32_t)whi, (uint32_t)(whi >> 32));
      } else {  // block shared with a neighbouring text: byte stores only
        for (int q = (p_lo < 0 ? -p_lo : 0); q < p_hi - p_lo; ++q)
          dst[q] = (uint8_t)((q < 8 ? wlo : whi) >> ((q & 7) * 8));
      }
    }
    group_sync();
  }
}

// k_subs_wave<G>: G lanes (a wavefront, half or quarter of one) assemble one text's output in LDS without a
// search and without a per-byte branch.  Text positions are kept in the frame of the 16-byte blocks that
// hold the text (mis = address & 15), the output tile in the frame of the output address (head).
//   matches, one lane each:  the start and end position of every replaced match set a bit in two LDS
//     bitmaps; matched bytes before the match come from a prefix sum over the lanes' match lengths, so the
//     replacement's R bytes go straight to  head + start - matched_before + m R  in the output tile;
//   frame blocks, one lane each:  T = starts ^ ends of the block; "inside a match" at byte t is the parity
//     of the T bits at or below t (matches are non-empty and do not overlap; an end that is the next
//     match's start cancels), carried across lanes by a prefix sum that also gives the kept bytes and the
//     match starts before the block, i.e. where the block's first kept byte goes; the 16 bytes are then
//     placed with predicated byte writes;
//   output blocks, one lane each:  16-byte stores (byte stores where a block is shared with a neighbour).
// Texts whose frame or output exceeds the tiles (32 G + 16 / 64 G bytes) are left to k_subs_emit.
template <int G>
__global__ __launch_bounds__(kBlock) void k_subs_wave(int64_t n, const uint8_t* __restrict__ data,
                                                      const int64_t* __restrict__ offsets,
                                                      const int64_t* __restrict__ prefix,
                                                      const int32_t* __restrict__ spans, long long count,
                                                      int R, const uint16_t* __restrict__ rmap,
                                                      const int64_t* __restrict__ out_off,
                                                      uint8_t* __restrict__ out, int32_t* __restrict__ left,
                                                      const int32_t* __restrict__ go, int dbg) {
  if (*go == 0) return;   // k_subs_gate: the spans or the output do not fit (the host finds out behind this launch)
  constexpr int NG = kBlock / G, F = 32 * G + 16, O = 64 * G, BW = F / 32 + 1;
  static_assert(G == 256 || G == 64 || G == 32 || G == 16, "group = workgroup, wavefront, half or quarter of one");
  constexpr bool BLK = G > 64;   // the workgroup shares one text: barriers instead of wavefront order, prefix
                                 // sums carried across its four wavefronts through LDS
  static_assert(!BLK || G == kBlock, "a group beyond a wavefront is the whole workgroup");
  __shared__ __align__(16) uint8_t text_all[NG][F];
  __shared__ __align__(16) uint8_t out_all[NG][O];
  __shared__ uint32_t sbits_all[NG][BW], ebits_all[NG][BW];
  __shared__ uint32_t spare_all[kBlock];
  __shared__ int xw_all[3][BLK ? kBlock / 64 : 1];   // BLK: per-wavefront totals of the three prefix sums
  extern __shared__ __align__(16) uint8_t subs_dyn[];   // the replacement map (R u16 entries)
  uint16_t* rmap_lds = (uint16_t*)subs_dyn;
  for (int r = threadIdx.x; r < R + 8; r += blockDim.x) rmap_lds[r] = r < R ? rmap[r] : (uint16_t)0;
  __syncthreads();
  auto group_sync = [&]() {
    if (BLK) { __syncthreads(); return; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  // inclusive prefix over the group's lanes and the group's total (xw: one of the three LDS rows; a row is
  // used once per round, and the rounds are separated by the barriers of the other two)
  auto scan_add = [&](int x, int* xw, int& total) {
    if constexpr (!BLK) {
      const int incl = group_scan<BLK ? 64 : G, false>(x);
      total = __shfl(incl, G - 1, G);
      return incl;
    }
    int incl = group_scan<64, false>(x);
    const int wv = threadIdx.x >> 6;
    __syncthreads();   // the row's previous readers are done
    if ((threadIdx.x & 63) == 63) xw[wv] = incl;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < kBlock / 64; ++q) { const int v = xw[q]; tot += v; if (q < wv) before += v; }
    total = tot;
    return incl + before;
  };
  auto scan_xor = [&](int x, int* xw, int& total) {
    if constexpr (!BLK) {
      const int incl = group_scan<BLK ? 64 : G, true>(x);
      total = __shfl(incl, G - 1, G);
      return incl;
    }
    int incl = group_scan<64, true>(x);
    const int wv = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 63) xw[wv] = incl;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < kBlock / 64; ++q) { const int v = xw[q]; tot ^= v; if (q < wv) before ^= v; }
    total = tot;
    return incl ^ before;
  };
  const int lane = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  uint8_t* text = text_all[grp];
  uint8_t* otile = out_all[grp];
  uint32_t* sbits = sbits_all[grp];
  uint32_t* ebits = ebits_all[grp];
  const int64_t ngroups = (int64_t)gridDim.x * NG;
  // Two texts ahead: the descriptor (offsets, prefix, out_off: one round trip); one text ahead: its frame
  // blocks and its first G spans, in registers -- the global round trips of text i + 1 run under the LDS
  // phases of text i.
  struct Desc { int64_t ibase, a, obase; int tlen, k, olen; };
  auto load_desc = [&](int64_t i) {
    Desc d{0, 0, 0, 0, 0, 0};
    if (i < n) {
      d.ibase = offsets[i];
      d.tlen = (int)(offsets[i + 1] - d.ibase);
      d.a = prefix[i];
      int64_t k64 = prefix[i + 1] - d.a;
      if (count > 0 && k64 > count) k64 = count;
      d.k = (int)k64;
      d.obase = out_off[i];
      d.olen = (int)(out_off[i + 1] - d.obase);
    }
    return d;
  };
  uint4 tx[3];
  int2 sp_first;
  auto issue = [&](const Desc& d) {
    const uint8_t* tptr = data + d.ibase;
    const int mis = (int)((uintptr_t)tptr & 15);
    const uint8_t* fptr = tptr - mis;
    int nfb = d.olen > 0 ? (mis + d.tlen + 15) >> 4 : 0;
    if (nfb > 2 * G + 1) nfb = 2 * G + 1;   // a longer text is not this kernel's
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int b = lane + r * G;
      tx[r] = b < nfb ? MRX_LDG((const uint4*)(fptr + 16 * b)) : make_uint4(0, 0, 0, 0);
    }
    sp_first = (d.olen > 0 && lane < d.k) ? *(const int2*)(spans + 2 * (d.a + lane)) : make_int2(0, 0);
  };
  int64_t i = (int64_t)blockIdx.x * NG + grp;
  Desc d0 = load_desc(i), d1 = load_desc(i + ngroups);
  issue(d0);
  for (; i < n; i += ngroups) {
    const Desc d = d0;
    d0 = d1;
    d1 = load_desc(i + 2 * ngroups);
    const uint8_t* tptr = data + d.ibase;
    const int tlen = d.tlen, k = d.k, olen = d.olen;
    const int64_t a = d.a, obase = d.obase;
    const int mis = (int)((uintptr_t)tptr & 15), head = (int)((uintptr_t)(out + obase) & 15);
    if (olen <= 0 || !subs_wave_takes(G, tlen, mis, olen, head)) {
      if (olen > 0 && lane == 0) *left = 1;   // k_subs_emit, launched behind this kernel, looks
      issue(d0);
      continue;
    }
    const int nfb = (mis + tlen + 15) >> 4;
    group_sync();   // the previous text's tiles are free
    for (int w = lane; w < BW; w += G) { sbits[w] = 0; ebits[w] = 0; }
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (lane + r * G < nfb) *(uint4*)(text + 16 * (lane + r * G)) = tx[r];
    const int2 sp_cur = sp_first;
    issue(d0);
    group_sync();
    // ---- matches: boundary bits, replacement bytes
    int carry = 0;
    for (int m0 = 0; m0 < ((dbg & 16) ? 0 : k); m0 += G) {
      const int m = m0 + lane;
      int ms = 0, me = 0;
      if (m < k) {
        const int2 sp = m0 == 0 ? sp_cur : *(const int2*)(spans + 2 * (a + m));
        ms = sp.x; me = sp.y;
      }
      const int len = me - ms;
      int round_total;
      const int incl = scan_add(len, xw_all[0], round_total);
      const int before = carry + incl - len;
      carry += round_total;
      if (m < k) {
        atomicOr(&sbits[(mis + ms) >> 5], 1u << ((mis + ms) & 31));
        atomicOr(&ebits[(mis + me) >> 5], 1u << ((mis + me) & 31));
        uint8_t* dst = otile + (head + ms - before + m * R);
        const uint8_t* msrc = text + mis + ms;
        // four bytes a round: the map entries (one address for every lane) and the match bytes they name are read
        // together -- a byte at a time the loop waits for two dependent LDS reads per replacement byte
        for (int t = 0; t < ((dbg & 1) ? 0 : R); t += 4) {
          uint32_t r[4], v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) r[q] = rmap_lds[t + q];   // (the map is padded with eight zero entries)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = msrc[(r[q] & 0x8000u) ? (r[q] & 0x7FFFu) : 0u];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (t + q < R) dst[t + q] = (r[q] & 0x8000u) ? (uint8_t)v[q] : (uint8_t)r[q];
        }
      }
    }
    group_sync();
    // ---- frame blocks: kept bytes
    int kept_carry = 0, starts_carry = 0, inside_carry = 0;
    for (int b0 = 0; b0 < ((dbg & 8) ? 0 : nfb); b0 += G) {
      const int b = b0 + lane;
      uint32_t S = 0, T = 0, valid = 0;
      uint4 bx = make_uint4(0, 0, 0, 0);
      if (b < nfb) {
        const int sh = (b & 1) * 16;
        S = (sbits[b >> 1] >> sh) & 0xFFFFu;
        T = S ^ ((ebits[b >> 1] >> sh) & 0xFFFFu);
        const int lo = b == 0 ? mis : 0;
        const int hi = mis + tlen - 16 * b < 16 ? mis + tlen - 16 * b : 16;
        valid = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        bx = *(const uint4*)(text + 16 * b);
      }
      uint32_t P = T;   // P bit t = parity of the T bits at or below t
      P ^= P << 1; P ^= P << 2; P ^= P << 4; P ^= P << 8;
      P &= 0xFFFFu;
      const uint32_t keep0 = valid & ~P, keep1 = valid & P;   // kept bytes if the block begins outside / inside a match
      // kept bytes | match starts << 12 | parity << 24, for both entry states the counts differ: scan the
      // parity first (it decides which), then the counts
      const int par = (int)(P >> 15);
      int par_total;
      const int pin = scan_xor(par, xw_all[1], par_total);
      const int inside = inside_carry ^ pin ^ par;   // state on entry to my block
      inside_carry ^= par_total;
      const uint32_t keep = inside ? keep1 : keep0;
      const int cnt = __popc(keep) | (__popc(S) << 16);   // kept bytes (<= 16 G) | match starts
      int tot;
      const int cin = scan_add(cnt, xw_all[2], tot);
      const int ex = cin - cnt;
      int po = head + kept_carry + (ex & 0xFFFF) + (starts_carry + (ex >> 16)) * R;
      kept_carry += tot & 0xFFFF;
      starts_carry += tot >> 16;
      // 16 unconditional byte writes: a byte that is not kept goes to the lane's own spare word (a select costs
      // less than an execution-mask round trip per byte); a wavefront without any kept byte skips them
      if (__builtin_amdgcn_ballot_w64(keep != 0) == 0 || (dbg & 2)) continue;
      const uint32_t wv[4] = {bx.x, bx.y, bx.z, bx.w};
      uint8_t* const spare = (uint8_t*)&spare_all[threadIdx.x];
      const int Rs = S ? R : 0;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        po += (int)((S >> t) & 1u) * Rs;
        const uint32_t kb = (keep >> t) & 1u;
        uint8_t* const wp = kb ? otile + po : spare;
        *wp = (uint8_t)(wv[t >> 2] >> ((t & 3) * 8));
        po += (int)kb;
      }
    }
    group_sync();
    // ---- output blocks
    uint8_t* dst0 = out + obase - head;
    const int nob = (dbg & 4) ? 0 : (head + olen + 15) >> 4;
    for (int b = lane; b < nob; b += G) {
      if (16 * b >= head && 16 * b + 16 <= head + olen) {
        *(uint4*)(dst0 + 16 * b) = *(const uint4*)(otile + 16 * b);
      } else {   // block shared with a neighbouring text
        const int q1 = 16 * b + 16 < head + olen ? 16 * b + 16 : head + olen;
        for (int q = 16 * b < head ? head : 16 * b; q < q1; ++q) dst0[q] = otile[q];
      }
    }
  }
}

enum { SUB_SIZE = 0, SUB_EMIT = 1 };

template <int MODE, int BT = 0>
__global__ __launch_bounds__(kBlock) void k_sub(DevPlan p, const uint8_t* __restrict__ blob,
                                                Layout lay, int64_t n,
                                                const uint8_t* __restrict__ repl, int repl_len,
                                                int use_groups, const ReplSeg* __restrict__ tpl,
                                                int ntpl, long long count,
                                                int64_t* __restrict__ sizes,
                                                const int64_t* __restrict__ out_off,
                                                uint8_t* __restrict__ out, int64_t out_cap) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Ctx c = stage_tables(p, blob, lds);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const Text t = lay.text(i);
    if (MODE == SUB_SIZE) {
      SizeSink s;
      sub_text<BT>(c, t, repl, repl_len, use_groups, tpl, ntpl, count, s);
      sizes[i] = s.n;
    } else {
      WriteSink s{out, out_off[i], out_cap};
      sub_text<BT>(c, t, repl, repl_len, use_groups, tpl, ntpl, count, s);
    }
  }
}

// mrx_debug_subs_group(): lanes per text in k_subs_wave (16 / 32 / 64), 0 = k_subs_emit only, -1 = by text length
std::atomic<int> g_subs_group{env_int("MRX_SUBS_G", -1)};
// regex.sub for streamable plans: streaming findall -> sizes -> prefix sums -> emit (see k_subs_*)
// A replacement that copies a fixed-width group copies text[match start + offset ...] whatever the match looked like
// (_apply_template_fixed, matcher.mojo:1592-1621; the widths come from the pattern text, quantifiers ignored:
// 'x(\\d)?' has its group at offset 1 even when the match is "x").  A match close to the end of its text can thus
// reach behind the text -- upstream reads those bytes unchecked; the oracle's slice and sub_text() stop at the end of
// the text, so the replacement is shorter than R bytes there.  The spans route has one R for every match: it
// looks at the LAST match of each text (the one that reaches furthest) and hands the call back
// (kSubsRetryGeneric) when any reaches behind its text.
__global__ __launch_bounds__(kBlock) void k_subs_reach(int64_t n, const int64_t* __restrict__ offsets,
                                                       const int64_t* __restrict__ prefix, const int32_t* __restrict__ spans,
                                                       int64_t span_cap, int reach, int32_t* __restrict__ over) {
  if (prefix[n] > span_cap) return;   // the spans are incomplete: the caller repeats the findall
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = prefix[i], b = prefix[i + 1];
    if (b > a && (int64_t)spans[2 * (b - 1)] + reach > offsets[i + 1] - offsets[i]) *over = 1;
  }
}
// go = 1 when the assembly may run: every span had room, the output fits, there is output, no group reaches behind its text
__global__ void k_subs_gate(const int64_t* __restrict__ matches, int64_t span_cap, const int64_t* __restrict__ out_bytes,
                            int64_t out_cap, const int32_t* __restrict__ over, int32_t* __restrict__ go) {
  *go = (*matches <= span_cap && *out_bytes <= out_cap && *out_bytes > 0 && !(over && *over)) ? 1 : 0;
}
int sub_from_spans(const mrx_handle* h, const Layout& lay, int64_t n, const std::vector<uint16_t>& rmap,
                   int64_t count, int64_t* out_off, uint8_t* out, int64_t out_cap, int64_t* total_bytes,
                   hipStream_t s, int group_reach = 0, int64_t known_bytes = -1, int64_t known_max = -1) {
  // Two host synchronisations per call: the batch's byte count and longest text (sizes the span buffer
  // and, handed on, spares findall its own look; none when the caller knows them: rows at a fixed pitch), and the
  // two totals -- matches and output bytes -- behind findall, sizes and prefix sums, all enqueued without waiting.
  int64_t in_bytes = known_bytes, max_len = known_max;
  if (known_bytes < 0 || known_max < 0)
    if (int rc0 = csr_stats(lay, n, s, &in_bytes, &max_len)) return rc0;
  if (in_bytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets[n] is negative");
  const int R = (int)rmap.size();
  int64_t* d_prefix = nullptr;
  int32_t* d_spans = nullptr;
  uint16_t* d_rmap = nullptr;
  int32_t* d_cum = nullptr;
  int64_t *d_sizes = nullptr, *d_total = nullptr;
  int32_t* d_left = nullptr;
  int32_t* d_go = nullptr;
  int32_t* d_over = nullptr;
  int32_t over = 0;
  MRX_SCRATCH(d_over, sizeof(int32_t), s);
  if (group_reach > 0) MRX_HIP_TRY(hipMemsetAsync(d_over, 0, sizeof(int32_t), s));
  MRX_SCRATCH(d_prefix, sizeof(int64_t) * (n + 1), s);
  MRX_SCRATCH(d_rmap, sizeof(uint16_t) * (R + 8), s);
  MRX_SCRATCH(d_sizes, sizeof(int64_t) * n, s);
  MRX_SCRATCH(d_total, sizeof(int64_t), s);
  MRX_SCRATCH(d_left, sizeof(int32_t), s);
  MRX_SCRATCH(d_go, sizeof(int32_t), s);
  if (R) MRX_HIP_TRY(hipMemcpyAsync(d_rmap, rmap.data(), sizeof(uint16_t) * R, hipMemcpyHostToDevice, s));
  int64_t cap = in_bytes / 8 + n + 64, nm = 0, tot = 0;
  if (const int64_t seen = h->sub_matches_per_kib.load(std::memory_order_relaxed); seen > 128) {
    const int64_t by_hint = (in_bytes >> 10) * (seen + seen / 8 + 1) + n + 64;   // the last batch's density + 1/8
    if (by_hint > cap) cap = by_hint < in_bytes + n + 64 ? by_hint : in_bytes + n + 64;
  }
  int rc = MRX_OK;
  bool cum_later = false;
  int G = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    MRX_SCRATCH(d_spans, sizeof(int32_t) * 2 * (size_t)cap, s);
    MRX_SCRATCH(d_cum, sizeof(int32_t) * (size_t)(cap + 1), s);
    rc = run_findall(h, lay, n, d_prefix, d_spans, cap, nullptr, s, /*match_next_sequence=*/true, in_bytes, max_len);
    if (rc != MRX_OK) return rc;
    const int64_t avg0 = in_bytes / (n > 0 ? n : 1);
    // lanes per text in k_subs_wave by average text length (1 KiB texts: 32 lanes 1.41 ms, 64 lanes 1.56 ms);
    // 0 = k_subs_emit alone: long replacement templates (one lane writes a replacement), forced, or texts
    // beyond the workgroup form's tiles, which take k_subs_emit<kBlock>
    const bool long_texts = (long_text_mode() == 1 || long_text_mode() == 3 || avg0 > 6144) && long_text_mode() != 2;
    const int force_g = g_subs_group;
    G = force_g >= 0 ? force_g : (avg0 > 2048 ? 256 : avg0 > 1024 ? 64 : avg0 > 224 ? 32 : 16);
    if (R > 1024 || long_texts) G = 0;
    // cum[] (matched bytes before each match) is k_subs_emit's: when k_subs_wave runs in front of it, it is
    // only computed if that kernel leaves texts over (cum_later)
    cum_later = count == 0 && G != 0;
    if (cum_later) {
      const int64_t blocks = ((n + 63) / 64 + (kBlock / 64) - 1) / (kBlock / 64);
      hipLaunchKernelGGL(k_subs_sizes_flat, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kBlock), 0, s,
                         n, lay.offsets, d_prefix, d_spans, R, d_sizes, cap);
    } else {
      const int64_t blocks = (n + (kBlock / 16) - 1) / (kBlock / 16);
      hipLaunchKernelGGL(k_subs_sizes, dim3((unsigned)(blocks < 65536 * 4 ? blocks : 65536 * 4)), dim3(kBlock), 0, s,
                         n, lay.offsets, d_prefix, d_spans, (long long)count, R, d_sizes, d_cum, cap, (const int32_t*)nullptr);
    }
    MRX_HIP_TRY(hipGetLastError());
    rc = device_scan<int64_t>(d_sizes, n, out_off, d_total, s);
    if (rc != MRX_OK) return rc;
    if (group_reach > 0)
      hipLaunchKernelGGL(k_subs_reach, dim3(device_grid(n, kBlock)), dim3(kBlock), 0, s, n, lay.offsets, d_prefix, d_spans, cap,
                         group_reach, d_over);
    // The assembly is enqueued BEHIND a device-side go-ahead and BEFORE the host has seen the totals: the stream does
    // not run dry while they travel (63 us of 1.7 ms on config 4).  When the go-ahead says no, the kernels return at
    // once and the host, which reads the same numbers below, retries or reports.
    hipLaunchKernelGGL(k_subs_gate, dim3(1), dim3(1), 0, s, d_prefix + n, cap, d_total, out_cap,
                       group_reach > 0 ? (const int32_t*)d_over : (const int32_t*)nullptr, d_go);
    if (G == 0 && (long_text_mode() == 1 || long_text_mode() == 3 || in_bytes / n >= 4096) && long_text_mode() != 2) {   // long texts: a workgroup per text
      hipLaunchKernelGGL(k_subs_emit<kBlock>, dim3((unsigned)(n < 4096 ? n : 4096)), dim3(kBlock),
                         (size_t)(2 * R + 16), s, n, lay.data, lay.offsets, d_prefix, d_spans, d_cum, (long long)count, R,
                         d_rmap, out_off, out, 0, (const int32_t*)d_go);
      set_last_kernel("k_subs_emit_long");
    } else {
      // short texts: G lanes assemble a text in LDS (k_subs_wave); what does not fit its tiles is left to
      // k_subs_emit, which returns at once when nothing was left
      MRX_HIP_TRY(hipMemsetAsync(d_left, 0, sizeof(int32_t), s));
#define MRX_SUBS_WAVE(GG)                                                                                        \
  do {                                                                                                           \
    const int64_t blocks = (n + (kBlock / GG) - 1) / (kBlock / GG);                                              \
    hipLaunchKernelGGL(k_subs_wave<GG>, dim3((unsigned)(blocks < grid_cap() ? blocks : grid_cap())), dim3(kBlock), \
                       (size_t)(2 * R + 16), s, n, lay.data, lay.offsets, d_prefix, d_spans, (long long)count, R,   \
                       d_rmap, out_off, out, d_left, (const int32_t*)d_go, env_knobs().subs_debug);              \
  } while (0)
      if (G == 256) MRX_SUBS_WAVE(256);
      else if (G == 64) MRX_SUBS_WAVE(64);
      else if (G == 32) MRX_SUBS_WAVE(32);
      else if (G == 16) MRX_SUBS_WAVE(16);
#undef MRX_SUBS_WAVE
      MRX_HIP_TRY(hipGetLastError());
      const int64_t blocks = (n + (kBlock / kSubsLanes) - 1) / (kBlock / kSubsLanes);
      if (cum_later)
        hipLaunchKernelGGL(k_subs_sizes, dim3((unsigned)(blocks < grid_cap() ? blocks : grid_cap())), dim3(kBlock), 0, s,
                           n, lay.offsets, d_prefix, d_spans, (long long)count, R, (int64_t*)nullptr, d_cum, cap,
                           (const int32_t*)d_left);
      // (behind k_subs_wave: the texts it left over -- none when the go-ahead stopped it; alone: the go-ahead itself)
      hipLaunchKernelGGL(k_subs_emit<kSubsLanes>, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kBlock),
                         (size_t)(2 * R + 16), s, n, lay.data, lay.offsets, d_prefix, d_spans, d_cum, (long long)count, R,
                         d_rmap, out_off, out, G, G ? (const int32_t*)d_left : (const int32_t*)d_go);
      set_last_kernel(G ? "k_subs_wave" : "k_subs_emit");
    }
    MRX_HIP_TRY(hipGetLastError());   // the output bytes are complete when `s` reaches this point, as with every _dev call
    if (group_reach > 0) MRX_HIP_TRY(hipMemcpyAsync(&over, d_over, sizeof over, hipMemcpyDeviceToHost, s));
    MRX_HIP_TRY(hipMemcpyAsync(&nm, d_prefix + n, sizeof nm, hipMemcpyDeviceToHost, s));
    MRX_HIP_TRY(hipMemcpyAsync(&tot, d_total, sizeof tot, hipMemcpyDeviceToHost, s));
    MRX_HIP_TRY(hipStreamSynchronize(s));
    h->sub_matches_per_kib.store(in_bytes >= 1024 ? nm / (in_bytes >> 10) : 0, std::memory_order_relaxed);
    if (nm <= cap) break;
    if (attempt == 1) return internal_fail(MRX_E_NO_DEVICE, "sub: match count changed between two passes");
    // more matches than one per eight bytes: once more with room for all of them.  The second attempt's buffers lie
    // behind the first's, which stay where they are until the call returns (a dense batch sizes its next call's
    // first attempt by sub_matches_per_kib, so this is paid once).
    cap = nm;
  }
  if (over) {
    rc = kSubsRetryGeneric;
  } else {
    if (total_bytes) *total_bytes = tot;
    if (tot > out_cap) rc = internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(tot));
  }
  return rc;
}
}  // namespace

static int g_chain_sub_general = 0;   // mrx_debug_chain_sub_general
// ---- sub() with \1..\9 on a deterministic chain (HostPlan::chain) -----------------------------------------
// The matches are the plain search's spans (run_findall, match_next_sequence); a wavefront takes a text: every byte's
// leaf mask (bit l: leaf l takes the byte) in an LDS tile, a lane per match finds the leaves' boundaries as runs of
// mask bits, four bytes a step; from them the groups and the replacement's length.  k_subc_sizes: output length per
// text and, per match, the bytes the output has gained in front of it; k_subc_emit<TILE>: gaps and replacements into
// an output tile, the tile out in 16-byte stores.  A text or an output beyond 4 KiB: the call is the lane-per-text
// interpreter's (k_sub).
namespace {
template <int TILE>
__global__ __launch_bounds__(kBlock) void k_subc_sizes(ChainDev cd, int64_t n, const uint8_t* __restrict__ data,
                                                       const int64_t* __restrict__ offsets,
                                                       const int64_t* __restrict__ prefix, const int32_t* __restrict__ spans,
                                                       long long count, const uint8_t* __restrict__ g_mask,
                                                       int64_t* __restrict__ sizes, int32_t* __restrict__ dcum,
                                                       int32_t* __restrict__ longest, int64_t span_cap, int dbg) {
  if (prefix[n] > span_cap) return;   // the findall in front did not have room for its spans: the host retries
  constexpr int NB = TILE / 1024 + 1;
  constexpr int ROW = TILE / 16 + 4;
  __shared__ uint16_t bm_all[kBlock / 64][kSubcLeaves * ROW];
  __shared__ uint16_t bnd_all[kBlock / 64][64 * (kSubcLeaves + 1)];
  __shared__ uint8_t mask[256];
  for (int c = threadIdx.x; c < 256; c += blockDim.x) mask[c] = g_mask[c];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint16_t* bm = bm_all[wv];
  uint16_t* bnd = bnd_all[wv] + lane * (kSubcLeaves + 1);
  int worst = 0;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  uint4 tx[NB];
  int2 sp_first;
  auto issue = [&](const SubcDesc& d) {
    const uint8_t* tptr = data + d.ibase;
    const int mis = (int)((uintptr_t)tptr & 15);
    const uint8_t* fptr = tptr - mis;
    const int nfb = d.k > 0 && d.tlen <= TILE ? (mis + d.tlen + 15) >> 4 : 0;
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      const int b = lane + 64 * r;
      tx[r] = b < nfb ? *(const uint4*)(fptr + 16 * b) : make_uint4(0, 0, 0, 0);
    }
    sp_first = lane < d.k ? *(const int2*)(spans + 2 * (d.a + lane)) : make_int2(0, 0);
  };
  int64_t i = (int64_t)blockIdx.x * (kBlock / 64) + wv;
  SubcDesc d0 = subc_desc<false>(i, n, offsets, prefix, nullptr, count), d1 = subc_desc<false>(i + nw, n, offsets, prefix, nullptr, count);
  issue(d0);
  for (; i < n; i += nw) {
    const SubcDesc d = d0;
    d0 = d1;
    d1 = subc_desc<false>(i + 2 * nw, n, offsets, prefix, nullptr, count);
    const int tlen = d.tlen, k = d.k;
    const int64_t a = d.a;
    if (tlen > TILE) {   // (the host has looked at the longest text already: not reached)
      if (lane == 0) sizes[i] = 0;
      worst = 0x7FFFFFFF;
      issue(d0);
      continue;
    }
    const int mis = (int)((uintptr_t)(data + d.ibase) & 15);
    MRX_SUBC_WAVE_SYNC();
    if (k > 0 && !(dbg & 2)) subc_store<NB, ROW, false>(tx, bm, nullptr, mask, cd.need, (mis + tlen + 15) >> 4, lane);
    const int2 sp_cur = sp_first;
    issue(d0);
    MRX_SUBC_WAVE_SYNC();
    int carry = 0;
    for (int m0 = 0; m0 < k; m0 += 64) {
      const int m = m0 + lane;
      int delta = 0;
      if (m < k) {
        const int2 sp = m0 == 0 ? sp_cur : *(const int2*)(spans + 2 * (a + m));
        if (!(dbg & 1)) {
          subc_walk<ROW>(cd, bm, mis, bnd, sp.x, sp.y);
          delta = subc_repl_len(cd, bnd) - (sp.y - sp.x);
        }
      }
      const int incl = group_scan<64, false>(delta);
      if (m < k && !(dbg & 4)) dcum[a + m] = carry + incl - delta;
      carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) sizes[i] = (int64_t)tlen + carry;
    if (tlen + carry > worst) worst = tlen + carry;
  }
  if (lane == 0 && worst > 0) atomicMax(longest, worst);
}
// Every match's replacement differs from the match by the same number of bytes (each leaf of variable width lies in
// exactly one referenced group -- a template that reorders the groups): no walk for the sizes, a lane per text.
__global__ __launch_bounds__(kBlock) void k_subc_sizes_const(int64_t n, const int64_t* __restrict__ offsets,
                                                             const int64_t* __restrict__ prefix, long long count, int delta,
                                                             int64_t* __restrict__ sizes, int32_t* __restrict__ longest,
                                                             int64_t span_cap) {
  if (prefix[n] > span_cap) return;
  int worst = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t tlen = offsets[i + 1] - offsets[i];
    int64_t k = prefix[i + 1] - prefix[i];
    if (count > 0 && k > count) k = count;
    const int64_t olen = tlen + k * delta;
    sizes[i] = olen;
    const int w = tlen > 0x7FFFFFFF || olen > 0x7FFFFFFF ? 0x7FFFFFFF : (int)(tlen > olen ? tlen : olen);
    if (w > worst) worst = w;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(worst, d, 64); if (o > worst) worst = o; }
  if ((threadIdx.x & 63) == 0 && worst > 0) atomicMax(longest, worst);
}
template <int TILE>
__global__ __launch_bounds__(kBlock) void k_subc_emit(ChainDev cd, int64_t n, const uint8_t* __restrict__ data,
                                                      const int64_t* __restrict__ offsets,
                                                      const int64_t* __restrict__ prefix, const int32_t* __restrict__ spans,
                                                      long long count, const uint8_t* __restrict__ g_mask,
                                                      const uint8_t* __restrict__ g_repl, int repl_len,
                                                      const int32_t* __restrict__ dcum, const int64_t* __restrict__ out_off,
                                                      uint8_t* __restrict__ out, int cdelta, int dbg) {
  // dbg (MRX_SUBC_DEBUG, timing only): 8 no gap copies, 32 no replacement bytes, 64 no stores
  // dcum == nullptr: every match gains cdelta bytes (k_subc_sizes_const)
  constexpr int NB = TILE / 1024 + 1;
  constexpr int ROW = TILE / 16 + 4;
  __shared__ uint16_t bm_all[kBlock / 64][kSubcLeaves * ROW];
  __shared__ __align__(16) uint8_t text_all[kBlock / 64][TILE + 32];
  __shared__ __align__(16) uint8_t otile_all[kBlock / 64][TILE + 32];
  __shared__ uint16_t bnd_all[kBlock / 64][64 * (kSubcLeaves + 1)];
  __shared__ uint8_t mask[256];
  __shared__ uint8_t repl[kSubcRepl + 8];
  for (int c = threadIdx.x; c < 256; c += blockDim.x) mask[c] = g_mask[c];
  for (int c = threadIdx.x; c < repl_len; c += blockDim.x) repl[c] = g_repl[c];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint16_t* bm = bm_all[wv];
  uint8_t* tile = text_all[wv];
  uint8_t* otile = otile_all[wv];
  uint16_t* bnd = bnd_all[wv] + lane * (kSubcLeaves + 1);
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  uint4 tx[NB];
  int2 sp_first;
  int dc_first;
  auto takes = [&](const SubcDesc& d) { return d.olen > 0 && d.olen <= TILE && d.tlen <= TILE; };   // (else: not launched)
  auto issue = [&](const SubcDesc& d) {
    const uint8_t* tptr = data + d.ibase;
    const int mis = (int)((uintptr_t)tptr & 15);
    const uint8_t* fptr = tptr - mis;
    const int nfb = takes(d) ? (mis + d.tlen + 15) >> 4 : 0;
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      const int b = lane + 64 * r;
      tx[r] = b < nfb ? *(const uint4*)(fptr + 16 * b) : make_uint4(0, 0, 0, 0);
    }
    const bool have = takes(d) && lane < d.k;
    sp_first = have ? *(const int2*)(spans + 2 * (d.a + lane)) : make_int2(0, 0);
    dc_first = have && dcum ? dcum[d.a + lane] : lane * cdelta;
  };
  int64_t i = (int64_t)blockIdx.x * (kBlock / 64) + wv;
  SubcDesc d0 = subc_desc<true>(i, n, offsets, prefix, out_off, count), d1 = subc_desc<true>(i + nw, n, offsets, prefix, out_off, count);
  issue(d0);
  for (; i < n; i += nw) {
    const SubcDesc d = d0;
    d0 = d1;
    d1 = subc_desc<true>(i + 2 * nw, n, offsets, prefix, out_off, count);
    const int tlen = d.tlen, k = d.k, olen = d.olen;
    const int64_t a = d.a, obase = d.obase;
    if (!takes(d)) { issue(d0); continue; }
    const int mis = (int)((uintptr_t)(data + d.ibase) & 15), head = (int)((uintptr_t)(out + obase) & 15);
    MRX_SUBC_WAVE_SYNC();   // the previous text's tiles are free
    subc_store<NB, ROW, true>(tx, bm, tile, mask, cd.need, (mis + tlen + 15) >> 4, lane);
    const int2 sp_cur = sp_first;
    const int dc_cur = dc_first;
    issue(d0);
    MRX_SUBC_WAVE_SYNC();
    const uint8_t* txt = tile + mis;
    uint8_t* o = otile + head;
    // the whole wavefront copies text[src, src + len) to o[dst ..]
    auto copy_all = [&](int src, int len, int dst) {
      for (int j = lane; j < len; j += 64) o[dst + j] = txt[src + j];
    };
    int prev_end = 0;   // end of the match in front of this round's first
    for (int m0 = 0; m0 < k; m0 += 64) {
      const int m = m0 + lane;
      const bool live = m < k;
      int ms = 0, me = 0, before = 0;
      if (live) {
        const int2 sp = m0 == 0 ? sp_cur : *(const int2*)(spans + 2 * (a + m));
        ms = sp.x; me = sp.y;
        before = m0 == 0 ? dc_cur : dcum ? dcum[a + m] : m * cdelta;
      }
      int pe = __shfl_up(me, 1, 64);
      if (lane == 0) pe = prev_end;
      const int nlive = k - m0 < 64 ? k - m0 : 64;
      prev_end = __shfl(me, nlive - 1, 64);
      // the kept bytes in front of the match: short gaps by the lane, long ones by the wavefront
      const int gap = live ? ms - pe : 0;
      if (gap <= 24 && !(dbg & 8)) subc_copy(o + pe + before, txt + pe, gap);
      uint64_t wide = __ballot(gap > 24);
      while (wide) {
        const int src_lane = __ffsll((unsigned long long)wide) - 1;
        wide &= wide - 1;
        copy_all(__shfl(pe, src_lane, 64), __shfl(gap, src_lane, 64), __shfl(pe + before, src_lane, 64));
      }
      if (live) {
        subc_walk<ROW>(cd, bm, mis, bnd, ms, me);
        uint8_t* dst = o + ms + before;
        if (!(dbg & 32))
#pragma unroll
        for (int q = 0; q < kSubcTpl; ++q) {
          if (q >= cd.ntpl) break;
          const ReplSeg sg = cd.tpl[q];
          if (sg.group_ref) {
            const int gs = bnd[sg.start], gl = (int)bnd[sg.length] - gs;
            subc_copy(dst, txt + gs, gl);
            dst += gl;
          } else {
            subc_copy(dst, repl + sg.start, sg.length);
            dst += sg.length;
          }
        }
      }
    }
    copy_all(prev_end, tlen - prev_end, prev_end + (olen - tlen));   // behind the last replaced match
    MRX_SUBC_WAVE_SYNC();
    // the tile out: whole 16-byte blocks where the block is the text's alone, bytes at the two ends
    uint8_t* oframe = out + obase - head;
    const int nob = (head + olen + 15) >> 4;
    for (int b = lane; b < ((dbg & 64) ? 0 : nob); b += 64) {
      const int lo = 16 * b, hi = lo + 16;
      if (lo >= head && hi <= head + olen) {
        *(uint4*)(oframe + lo) = *(const uint4*)(otile + lo);
      } else {
        const int from = lo > head ? lo : head, to = hi < head + olen ? hi : head + olen;
        for (int j = from; j < to; ++j) oframe[j] = otile[j];
      }
    }
  }
}

int sub_chain_from_spans(const mrx_handle* h, const Layout& lay, int64_t n, const std::string& r,
                         const std::vector<ReplSeg>& tpl, int64_t count, int64_t* out_off, uint8_t* out, int64_t out_cap,
                         int64_t* total_bytes, hipStream_t s, int64_t known_bytes, int64_t known_max) {
  const ChainGroups& cg = h->hp.chain;
  if (cg.nleaf > kSubcLeaves || (int)tpl.size() > kSubcTpl || (int)r.size() > kSubcRepl) return kSubsRetryGeneric;
  int64_t in_bytes = known_bytes, max_len = known_max;
  if (known_bytes < 0 || known_max < 0)
    if (int rc0 = csr_stats(lay, n, s, &in_bytes, &max_len)) return rc0;
  if (in_bytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets[n] is negative");
  if (max_len > 4096) return kSubsRetryGeneric;
  ChainDev cd{};
  cd.nleaf = cg.nleaf; cd.ntpl = (int)tpl.size();
  for (int l = 0; l < kSubcLeaves; ++l) { cd.lmax[l] = cg.lmax[l]; cd.lfix[l] = l < cg.nleaf && cg.lmin[l] == cg.lmax[l] ? cg.lmin[l] : 0; }
  for (int l = 0; l + 1 < cg.nleaf; ++l) if (!cd.lfix[l]) cd.need |= 1 << l;
  cd.ntpl = 0;
  for (const ReplSeg& sg : tpl) {   // a group's segment: the two boundaries it lies between (a group the pattern lacks: nothing)
    if (sg.group_ref > 0) {
      if (sg.group_ref <= 9 && cg.gopen[sg.group_ref] >= 0) cd.tpl[cd.ntpl++] = ReplSeg{1, cg.gopen[sg.group_ref], cg.gclose[sg.group_ref]};
    } else if (sg.length > 0) {
      cd.tpl[cd.ntpl++] = sg;
    }
  }
  uint8_t mask8[256];
  for (int c = 0; c < 256; ++c) mask8[c] = (uint8_t)cg.mask[c];
  // does every match gain the same number of bytes?  (literal bytes + fixed-width leaves counted by the groups that hold
  // them - their own width; a leaf of variable width must lie in exactly one referenced group)
  bool const_delta = true;
  int cdelta = 0;
  {
    int covers[kSubcLeaves] = {0};
    for (int k = 0; k < cd.ntpl; ++k) {
      if (cd.tpl[k].group_ref) for (int l = cd.tpl[k].start; l < cd.tpl[k].length; ++l) ++covers[l];
      else cdelta += cd.tpl[k].length;
    }
    for (int l = 0; l < cg.nleaf; ++l) {
      if (cg.lmin[l] == cg.lmax[l]) cdelta += (covers[l] - 1) * cg.lmin[l];
      else if (covers[l] != 1) const_delta = false;
    }
    if (g_chain_sub_general) const_delta = false;   // (mrx_debug_chain_sub_general: the general form, for A/B runs and tests)
  }
  int64_t *d_prefix = nullptr, *d_sizes = nullptr, *d_total = nullptr;
  int32_t *d_spans = nullptr, *d_dcum = nullptr, *d_longest = nullptr;
  uint8_t *d_mask = nullptr, *d_repl = nullptr;
  MRX_SCRATCH(d_prefix, sizeof(int64_t) * (n + 1), s);
  MRX_SCRATCH(d_sizes, sizeof(int64_t) * n, s);
  // (output total, longest output, match total: three words side by side, one copy to the host)
  MRX_SCRATCH(d_total, 3 * sizeof(int64_t), s);
  d_longest = (int32_t*)(d_total + 1);
  MRX_SCRATCH(d_mask, 256, s);
  MRX_SCRATCH(d_repl, r.size() + 16, s);
  MRX_HIP_TRY(hipMemcpyAsync(d_mask, mask8, 256, hipMemcpyHostToDevice, s));   // (pageable source: copied before the call returns)
  if (!r.empty()) MRX_HIP_TRY(hipMemcpyAsync(d_repl, r.data(), r.size(), hipMemcpyHostToDevice, s));
  MRX_HIP_TRY(hipMemsetAsync(d_total, 0, 3 * sizeof(int64_t), s));
  int64_t cap = in_bytes / 8 + n + 64, nm = 0, tot = 0;
  if (const int64_t seen = h->sub_matches_per_kib.load(std::memory_order_relaxed); seen > 128) {
    const int64_t by_hint = (in_bytes >> 10) * (seen + seen / 8 + 1) + n + 64;
    if (by_hint > cap) cap = by_hint < in_bytes + n + 64 ? by_hint : in_bytes + n + 64;
  }
  int32_t longest = 0;
  const int subc_dbg = env_knobs().subc_debug;   // (ablation runs: wrong results)
  const int64_t blocks = (n + (kBlock / 64) - 1) / (kBlock / 64);
  const unsigned grid = (unsigned)(blocks < grid_cap() ? blocks : grid_cap());
  int rc = MRX_OK;
  // (one host synchronisation: the match total, which sizes the spans; the output total and the longest output, which
  // picks the emit kernel's tile)
  for (int attempt = 0; attempt < 2; ++attempt) {
    MRX_SCRATCH(d_spans, sizeof(int32_t) * 2 * (size_t)cap, s);
    MRX_SCRATCH(d_dcum, sizeof(int32_t) * (size_t)(cap + 1), s);
    rc = run_findall(h, lay, n, d_prefix, d_spans, cap, nullptr, s, /*match_next_sequence=*/true, in_bytes, max_len);
    if (rc != MRX_OK) return rc;
    // (sizes behind the spans without waiting: when the spans did not fit it returns at once)
    if (const_delta)
      hipLaunchKernelGGL(k_subc_sizes_const, dim3(device_grid(n, kBlock)), dim3(kBlock), 0, s, n, lay.offsets, d_prefix,
                         (long long)count, cdelta, d_sizes, d_longest, cap);
    else if (max_len <= 2048)
      hipLaunchKernelGGL(k_subc_sizes<2048>, dim3(grid), dim3(kBlock), 0, s, cd, n, lay.data, lay.offsets, d_prefix, d_spans,
                         (long long)count, d_mask, d_sizes, d_dcum, d_longest, cap, subc_dbg);
    else
      hipLaunchKernelGGL(k_subc_sizes<4096>, dim3(grid), dim3(kBlock), 0, s, cd, n, lay.data, lay.offsets, d_prefix, d_spans,
                         (long long)count, d_mask, d_sizes, d_dcum, d_longest, cap, subc_dbg);
    MRX_HIP_TRY(hipGetLastError());
    rc = device_scan<int64_t>(d_sizes, n, out_off, d_total, s);
    if (rc != MRX_OK) return rc;
    int64_t h3[3] = {0, 0, 0};
    MRX_HIP_TRY(hipMemcpyAsync(d_total + 2, d_prefix + n, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    MRX_HIP_TRY(hipMemcpyAsync(h3, d_total, sizeof h3, hipMemcpyDeviceToHost, s));
    MRX_HIP_TRY(hipStreamSynchronize(s));
    tot = h3[0]; longest = (int32_t)(h3[1] & 0xFFFFFFFF); nm = h3[2];
    h->sub_matches_per_kib.store(in_bytes >= 1024 ? nm / (in_bytes >> 10) : 0, std::memory_order_relaxed);
    if (nm <= cap) break;
    if (attempt == 1) return internal_fail(MRX_E_NO_DEVICE, "sub: match count changed between two passes");
    cap = nm;   // (as in sub_from_spans(): the second attempt's buffers lie behind the first's)
  }
  if (longest > 4096) {
    rc = kSubsRetryGeneric;
  } else {
    if (total_bytes) *total_bytes = tot;
    if (tot > out_cap) {
      rc = internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(tot));
    } else if (tot > 0) {
#define MRX_SUBC_EMIT(TT)                                                                                              \
  hipLaunchKernelGGL(k_subc_emit<TT>, dim3(grid), dim3(kBlock), 0, s, cd, n, lay.data, lay.offsets, d_prefix, d_spans, \
                     (long long)count, d_mask, d_repl, (int)r.size(), const_delta ? (const int32_t*)nullptr : d_dcum, out_off, out, cdelta, subc_dbg)
      if (longest <= 2048 && max_len <= 2048) MRX_SUBC_EMIT(2048);
      else MRX_SUBC_EMIT(4096);
#undef MRX_SUBC_EMIT
      MRX_HIP_TRY(hipGetLastError());
      set_last_kernel("k_subc_emit");
    }
  }
  return rc;
}

__global__ __launch_bounds__(kBlock) void k_pitch_offsets(int64_t n, int64_t stride, int64_t* __restrict__ off) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) off[i] = i * stride;
}
}  // namespace
int mrx::rows_as_csr(const TextBatch& b, int64_t n, void* st, TextBatch* out) {
  int64_t* d_off = nullptr;
  MRX_SCRATCH(d_off, sizeof(int64_t) * (n + 1), (hipStream_t)st);
  hipLaunchKernelGGL(k_pitch_offsets, dim3(device_grid(n + 1, kBlock)), dim3(kBlock), 0, (hipStream_t)st, n, b.stride, d_off);
  MRX_HIP_TRY(hipGetLastError());
  *out = csr(b.data, d_off);
  return MRX_OK;
}
int mrx::group_template_refusal(const mrx_handle* h) {
  if (h->hp.fixed_total >= 0 || h->hp.bt.ok) return MRX_OK;
  return internal_fail(MRX_E_UNSUPPORTED,
                       "sub() with \\1..\\9 on this pattern uses NFAEngine.match_next_with_groups (recursive "
                       "backtracking matcher, nfa.mojo:500-574); its flat-program form does not cover: " +
                           (h->hp.bt.why_not.empty() ? std::string("'.*'") : h->hp.bt.why_not));
}

static int sub_any(const mrx_handle* h, const char* repl, size_t repl_len, int64_t count, const Layout& lay_in,
                   int64_t n, int64_t* out_off, uint8_t* out, int64_t out_cap, int64_t* total_bytes, void* st,
                   int64_t known_bytes = -1, int64_t known_max = -1) {   // (byte count and longest text, when the caller has them)
  const uint8_t* d = lay_in.data;
  const int64_t* off = lay_in.offsets;
  ScratchScope scratch_scope_((hipStream_t)st);
  if (!h) return internal_fail(MRX_E_ARGUMENT, "null handle");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "negative batch size");
  const std::string r(repl ? repl : "", repl_len);
  const bool groups = repl_has_group_refs(r);
  // group references on a pattern outside the fixed-width form: every match comes from
  // NFAEngine.match_next_with_groups (matcher.mojo:1781-1822), not from the search engines
  const bool general_groups = groups && h->hp.fixed_total < 0;
  std::vector<ReplSeg> tpl;
  if (general_groups) {
    if (int rc = group_template_refusal(h)) return rc;
  } else if (int rc = check_search_supported(h)) {
    return rc;
  }
  if (groups) tpl = parse_repl_template(r);
  if (int rc = check_lds(h)) return rc;
  if (int rc = ensure_device(h)) return rc;
  hipStream_t s = (hipStream_t)st;
  // a spans route that hands the call back (kSubsRetryGeneric) has enqueued its work; the lane-per-text form below
  // runs behind it on the same stream and takes over its bytes (not behind mrx_sub_strided_dev's offsets: they stay)
  const ScratchMark before_spans = scratch_mark(s);
  // \1..\9 on a deterministic chain whose matches are the table walk's: spans of the plain search, groups from the
  // leaves' runs (k_subc_sizes / k_subc_emit); batches with a text or an output beyond the tiles stay the interpreter's
  if (general_groups && h->hp.chain.ok && !force_generic() && n > 0 && off && count >= 0 &&
      (h->hp.dev.flags & (PF_STREAM_SEARCH | PF_STEP_SEARCH)) && h->hp.why_no_search.empty()) {
    const int rc = sub_chain_from_spans(h, csr(d, off), n, r, tpl, count, out_off, out, out_cap,
                                        total_bytes, s, known_bytes, known_max);
    if (rc != kSubsRetryGeneric) return rc;
    scratch_reuse_from(s, before_spans);
  }
  // sub() iterates match_next from the previous match end; on the plain route that is exactly the
  // findall sequence, so the spans of the streaming kernel or of the windowed stepper serve it.
  // (Not with a memchr prefilter, which only match_next consults; not for exact literals, whose
  // findall spans overlap while sub's own search loop does not.)
  const uint32_t sfl = h->hp.dev.flags;
  const bool spans_ok = !(sfl & PF_EXACT_LITERAL) &&
                        ((!force_generic() && (sfl & PF_STREAM_SEARCH)) ||
                         (force_generic() < 2 && (sfl & PF_STEP_SEARCH) && !(sfl & PF_PREFILTER)));
  // (group templates of "concat" patterns that are not purely groups: texts of exactly fixed_total bytes take the
  // whole-text shortcut, which only sub_text() has)
  const bool shortcut_differs = groups && h->hp.fixed_concat && !h->hp.fixed_pure;
  if (spans_ok && !general_groups && !shortcut_differs && n > 0 && off) {
    // replacement as a fixed-length byte map
    std::vector<uint16_t> rmap;
    int group_reach = 0;   // how far behind a match's start the template reads
    if (groups) {
      for (const ReplSeg& sg : tpl) {
        if (sg.group_ref > 0 && sg.group_ref <= h->hp.fixed_ngroups) {
          for (int j = 0; j < h->hp.fixed_w[sg.group_ref]; ++j)
            rmap.push_back((uint16_t)(0x8000 | (h->hp.fixed_off[sg.group_ref] + j)));
          group_reach = std::max(group_reach, h->hp.fixed_off[sg.group_ref] + h->hp.fixed_w[sg.group_ref]);
        }
        else
          for (int j = 0; j < sg.length; ++j) rmap.push_back((uint8_t)r[sg.start + j]);
      }
    } else {
      for (unsigned char ch : r) rmap.push_back(ch);
    }
    // (nothing but (\d{N}) groups: every match is fixed_total bytes long and holds all its windows)
    if (h->hp.fixed_pure) group_reach = 0;
    if (rmap.size() <= 4096 && h->hp.fixed_total < 0x7FFF) {
      const int rc = sub_from_spans(h, csr(d, off), n, rmap, count, out_off, out, out_cap,
                                    total_bytes, s, group_reach, known_bytes, known_max);
      if (rc != kSubsRetryGeneric) return rc;   // else: a group reaches behind its text, the lane-per-text form cuts it
      scratch_reuse_from(s, before_spans);
    }
  }
  uint8_t* d_repl = nullptr;
  ReplSeg* d_tpl = nullptr;
  int64_t *d_sizes = nullptr, *d_total = nullptr;
  MRX_SCRATCH(d_repl, r.size() + 16, s);
  MRX_SCRATCH(d_tpl, sizeof(ReplSeg) * (tpl.size() + 1), s);
  MRX_SCRATCH(d_sizes, sizeof(int64_t) * (n > 0 ? n : 1), s);
  MRX_SCRATCH(d_total, sizeof(int64_t), s);
  if (!r.empty()) MRX_HIP_TRY(hipMemcpyAsync(d_repl, r.data(), r.size(), hipMemcpyHostToDevice, s));
  if (!tpl.empty())
    MRX_HIP_TRY(hipMemcpyAsync(d_tpl, tpl.data(), sizeof(ReplSeg) * tpl.size(), hipMemcpyHostToDevice, s));
  Layout lay = lay_in;
  const bool sub_bt = plan_uses_backtracker(h) || general_groups;
  if ((h->hp.dev.flags & PF_BT_SEARCH) || general_groups) {
    const Layout plain = lay;
    if (int rc = bt_prepass(h, plain, n, s, &lay)) return rc;
  }
  if (n > 0) {
    ScanTimer tm(s);
#define MRX_L(B) hipLaunchKernelGGL((k_sub<SUB_SIZE, B>), dim3(device_grid(n, kBlock)), dim3(kBlock), lds_for(h), s,                     \
                                   h->hp.dev, H_BLOB(h), lay, n, d_repl, (int)r.size(), general_groups ? 2 : groups ? 1 : 0, d_tpl, \
                                   (int)tpl.size(), (long long)count, d_sizes, (const int64_t*)nullptr, (uint8_t*)nullptr, (int64_t)0)
    MRX_BT_DISPATCH(bt_kernel_kind(h, sub_bt), MRX_L);
#undef MRX_L
    set_last_kernel("k_sub_size");
    MRX_HIP_TRY(hipGetLastError());
    tm.stop();
  }
  if (int rc = device_scan<int64_t>(d_sizes, n, out_off, d_total, s)) return rc;
  int64_t tot = 0;
  MRX_HIP_TRY(hipMemcpyAsync(&tot, d_total, sizeof tot, hipMemcpyDeviceToHost, s));
  MRX_HIP_TRY(hipStreamSynchronize(s));
  if (total_bytes) *total_bytes = tot;
  int rc = MRX_OK;
  if (tot > out_cap) {
    rc = internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(tot));
  } else if (n > 0 && tot > 0) {
#define MRX_L(B) hipLaunchKernelGGL((k_sub<SUB_EMIT, B>), dim3(device_grid(n, kBlock)), dim3(kBlock), lds_for(h), s,                     \
                                   h->hp.dev, H_BLOB(h), lay, n, d_repl, (int)r.size(), general_groups ? 2 : groups ? 1 : 0, d_tpl, \
                                   (int)tpl.size(), (long long)count, (int64_t*)nullptr, out_off, out, out_cap)
    MRX_BT_DISPATCH(bt_kernel_kind(h, sub_bt), MRX_L);
#undef MRX_L
    MRX_HIP_TRY(hipGetLastError());
  }
  return rc;
}

extern "C" {
int mrx_sub_dev(const mrx_handle* h, const char* repl, size_t repl_len, int64_t count,
                const uint8_t* d, const int64_t* off, int64_t n, int64_t* out_off, uint8_t* out,
                int64_t out_cap, int64_t* total_bytes, void* st) {
  return sub_any(h, repl, repl_len, count, csr(d, off), n, out_off, out, out_cap, total_bytes, st);
}
int mrx_sub_known_dev(const mrx_handle* h, const char* repl, size_t repl_len, int64_t count,
                      const uint8_t* d, const int64_t* off, int64_t n, int64_t end_offset, int64_t max_text_len,
                      int64_t* out_off, uint8_t* out, int64_t out_cap, int64_t* total_bytes, void* st) {
  if (end_offset < 0 || max_text_len < 0) return internal_fail(MRX_E_ARGUMENT, "negative end offset / text length");
  return sub_any(h, repl, repl_len, count, csr(d, off), n, out_off, out, out_cap, total_bytes, st,
                 end_offset, max_text_len);
}
// Texts at a fixed pitch.  Rows without padding (len == stride, no per-text lengths) are a CSR batch whose offsets
// are i * stride: they are written once on the device and the call takes every fast path of mrx_sub_dev; padded
// rows run on the lane-per-text kernels (the spans route assembles its output from CSR offsets).
int mrx_sub_strided_dev(const mrx_handle* h, const char* repl, size_t repl_len, int64_t count,
                        const uint8_t* d, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                        int64_t* out_off, uint8_t* out, int64_t out_cap, int64_t* total_bytes, void* st) {
  // (`len` is ignored when d_lens is given, as in every other strided entry point)
  const TextBatch b = strided(d, stride, d_lens, len);
  if (int rc = check_batch(b, BATCH_PITCH_TERSE)) return rc;
  if (rows_unpadded(b, n)) {
    ScratchScope scope_((hipStream_t)st);
    TextBatch rows;
    if (int rc = rows_as_csr(b, n, st, &rows)) return rc;
    return sub_any(h, repl, repl_len, count, rows, n, out_off, out, out_cap, total_bytes, st, n * stride, stride);
  }
  return sub_any(h, repl, repl_len, count, b, n, out_off, out, out_cap, total_bytes, st);
}
int mrx_sub_batch(const mrx_handle* h, const char* repl, size_t repl_len, int64_t count,
                  const uint8_t* data, const int64_t* off, int64_t n, int64_t* out_offsets,
                  uint8_t* out_data, int64_t out_cap, int64_t* total_bytes) {
  DevBatch b; DevBuf<int64_t> oo; DevBuf<uint8_t> od;
  if (int rc = b.upload(data, off, n)) return rc;
  if (int rc = oo.alloc(n + 1)) return rc;
  if (int rc = od.alloc((size_t)out_cap)) return rc;
  int64_t tot = 0;
  const int rc = mrx_sub_dev(h, repl, repl_len, count, b.data, b.offsets, n, oo.p, od.p, out_cap,
                             &tot, nullptr);
  if (total_bytes) *total_bytes = tot;
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  MRX_HIP_TRY(hipMemcpy(out_offsets, oo.p, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot > 0) MRX_HIP_TRY(hipMemcpy(out_data, od.p, (size_t)tot, hipMemcpyDeviceToHost));
  return rc;
}
void mrx_debug_chain_sub_general(int on) { g_chain_sub_general = on ? 1 : 0; }
void mrx_debug_subs_group(int g) { g_subs_group = (g == 0 || g == 16 || g == 32 || g == 64 || g == 256) ? g : -1; }
}  // extern "C"
