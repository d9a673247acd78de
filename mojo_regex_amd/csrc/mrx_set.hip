// Pattern sets (include/mrx.h, "pattern sets"): search / count / matches of k patterns over one batch.
//
// The reference matches one pattern per call; a caller with k rules makes k calls, and each of them reads the whole
// batch from HBM.  A set runs the members whose single-pattern call would take the streaming kernel's one
// left-to-right walk (check_streamable(), mrx_plan.cpp: PF_STREAMABLE for count, PF_STREAM_SEARCH for search) side
// by side in ONE pass over the texts, k_set_scan: the texts are staged through LDS once and every member takes its
// table step on every byte.  Every other member (prefilter search, anchored automaton, stepper, multi-walk, bitset,
// backtracker, `$`-LazyDFA, `.*`) runs its own single-pattern entry point into scratch, and k_set_scatter writes the
// answer into its column.  Member j's answer for text i is therefore exactly the single-pattern call's.
//
// Set plan (per operation; search and matches share theirs):
//   - a shared member's walk is the entry matrix E of its search automaton (HostPlan::st_entries:
//     E[q][byte] = next << 2 | EMIT << 1 | NEWSTART over the live states, 0 = idle), packed as
//       column slot: at most 4 live states; four members share one u64[256] column table, member m of the group
//         owns bits 16 m .. 16 m + 15, state q the 4-bit field at 16 m + 4 q.  The lane keeps the field's bit
//         offset, so a step is `f = col >> sh & 15; sh = 16 m + (f & 12)`: one ds_read_b64 per byte feeds four walks;
//       class member: more live states (the wide-column and class-table plans): cls u8[256] | trans u16[live][2^cshift]
//         (entry = row of the next state << 2 | EMIT << 1 | NEWSTART, row = state << cshift) | accept u8[live];
//         at most kSetClsEntries entries, otherwise the member keeps its own route.
//   - a pass holds at most 32 members, 8 column groups, 8 class members and kSetTableBudget bytes of tables, so that
//     tables + four 9 KiB text tiles stay within 64 KiB of LDS and the per-lane state (three registers per member for
//     search) within ~170 VGPRs.  Larger sets run several passes; each pass reads the texts again.
//
// Route rule (a pure function of set, operation and batch shape -- nothing is timed): the MEMBER LOOP, for every
// batch shape.  The k-sweep (tools/bench_set.py, profiles/set_scan.md) measured the shared pass slower than the k
// single-pattern calls at every k from 1 to 64, for count, search and matches, pitch and ragged: this kernel is bound
// by instruction issue (every column slot of a group and a uniform branch per group are paid on every byte; search
// with more than two class members runs the spilling <8, 8> instantiation), not by the bytes it saves.  The shared
// pass stays available (mrx_debug_set_route(1)) and tested until a faster kernel earns the rule back.
// Bytes outside a text (the CSR frame: a text is staged from the 16-byte boundary below its first byte, and a
// chunk may reach past its end) are not stepped at all: chunks in which every lane of the wavefront lies inside its
// text run the unmasked loop, the others the masked one (the member states are held), as ST_FIRST's probe does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"
#include "mrx_plan.hpp"

namespace mrx {
namespace {

constexpr int kSetMaxK = 256;
constexpr int kSetPassMembers = 32;
constexpr int kSetMaxCG = 8;                  // column groups (4 members each) per pass
constexpr int kSetMaxCM = 8;                  // class members per pass
constexpr int kSetTableBudget = 20 * 1024;    // LDS bytes of one pass's tables
constexpr int kSetClsEntries = 2048;          // class member: live states x padded classes
constexpr int kSetWaves = 4;
constexpr int kSetChunk = 128;                // bytes of every text staged per step: one cache line
constexpr int kSetPitch = kSetChunk + 16;     // +16: the per-lane 16-byte read-back is bank-conflict free
constexpr int kSetTile = 64 * kSetPitch;      // 9216
constexpr int kSetFrameBytes = 64 * 16;       // per wavefront: base and end address of its 64 texts
typedef uint32_t set_u32x4 __attribute__((ext_vector_type(4)));   // (the non-temporal load takes native vectors)
enum { SET_COUNT = 0, SET_SEARCH = 1, SET_MATCHES = 2 };
const char* const kSetOpName[3] = {"count", "search", "matches"};

std::atomic<int> g_set_route{0};   // mrx_debug_set_route(): 0 rule, 1 shared wherever eligible, 2 own route always

// one pass, by value to the kernel
struct SetPassDev {
  int32_t ncg, ncm, table_bytes, k, words;
  int32_t col_j[kSetMaxCG * 4];     // set member of each column slot (-1: padding)
  int32_t col_fixed[kSetMaxCG * 4]; // > 0: the member's matches are [end - fixed, end) (exact-literal KMP automaton)
  uint32_t col_acc[kSetMaxCG];      // bit 4 m + q: state q of slot m accepts
  int32_t cm_j[kSetMaxCM], cm_fixed[kSetMaxCM], cm_cls[kSetMaxCM], cm_trans[kSetMaxCM], cm_acc[kSetMaxCM],
      cm_shift[kSetMaxCM];
};

// ---------------------------------------------------------------------------------------------------------------
// kernel
// ---------------------------------------------------------------------------------------------------------------
template <int MODE, int NCG, int NCM>
__global__ __launch_bounds__(64 * kSetWaves) void k_set_scan(const SetPassDev P, const uint8_t* __restrict__ blob,
                                                             const TextBatch B, int64_t n,
                                                             int32_t* __restrict__ o0, int32_t* __restrict__ o1,
                                                             uint64_t* __restrict__ bits) {
  constexpr int NS = NCG * 4 + NCM;   // member slots: columns first, then class members
  extern __shared__ __align__(16) uint8_t lds[];
  for (int o = (int)threadIdx.x * 16; o < P.table_bytes; o += 64 * kSetWaves * 16)
    *(uint4*)(lds + o) = *(const uint4*)(blob + o);
  __syncthreads();
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  uint8_t* tile = lds + P.table_bytes + wave * kSetTile;
  uint64_t* fb = (uint64_t*)(lds + P.table_bytes + kSetWaves * kSetTile + wave * kSetFrameBytes);   // [64] base, [64] end
  const uint64_t* cols = (const uint64_t*)lds;
  const int64_t ntask = (n + 63) / 64;
  for (int64_t task = (int64_t)blockIdx.x * kSetWaves + wave; task < ntask; task += (int64_t)gridDim.x * kSetWaves) {
    const int64_t i = task * 64 + lane;
    const bool live = i < n;
    int32_t L = 0;
    const uint64_t ptr = (uint64_t)(uintptr_t)(live ? B.text(i, &L) : B.data);
    const uint64_t base = ptr & ~(uint64_t)15;
    const int skew = live ? (int)(ptr - base) : 0;
    const int flen = live ? skew + L : 0;
    __builtin_amdgcn_wave_barrier();
    fb[lane] = base;
    fb[64 + lane] = live ? ptr + (uint64_t)L : base;   // no word at or past a text's end is loaded
    int nch = (flen + kSetChunk - 1) / kSetChunk;
#pragma unroll
    for (int d = 32; d; d >>= 1) nch = max(nch, __shfl_xor(nch, d));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    uint32_t sh[NCG * 4 > 0 ? NCG * 4 : 1];   // column slots: bit offset of the state's field in the group's column
    uint32_t row[NCM > 0 ? NCM : 1];          // class members: row offset of the state
    int32_t cnt[NS], st[NS], re[NS];          // count / start of the current walk / end of the first match (-1 none)
    uint64_t used = 0, hit = 0;   // per slot (40 slots at most)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const bool u = s < NCG * 4 ? (s < 4 * P.ncg && P.col_j[s] >= 0) : (s - NCG * 4 < P.ncm);
      if (u) used |= 1ull << s;
      cnt[s] = 0;
      st[s] = -1;
      re[s] = u ? -1 : 0;
      if (s < NCG * 4) sh[s < NCG * 4 ? s : 0] = 16 * (s & 3);
      else row[s - NCG * 4 < NCM ? s - NCG * 4 : 0] = 0;
    }
    auto step = [&](uint32_t byte, int p) {
#pragma unroll
      for (int g = 0; g < NCG; ++g) {
        if (g < P.ncg) {
          const uint64_t col = cols[g * 256 + byte];
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const int s = g * 4 + m;
            const uint32_t f = (uint32_t)(col >> sh[s]) & 15u;
            sh[s] = 16u * m + (f & 12u);
            if constexpr (MODE == SET_COUNT) cnt[s] += (f >> 1) & 1u;
            if constexpr (MODE == SET_SEARCH) {
              if ((f & 2u) && re[s] < 0) re[s] = p;
              if ((f & 1u) && re[s] < 0) st[s] = p;
            }
            if constexpr (MODE == SET_MATCHES) hit |= (uint64_t)((f >> 1) & 1u) << s;
          }
        }
      }
#pragma unroll
      for (int c = 0; c < NCM; ++c) {
        if (c < P.ncm) {
          const int s = NCG * 4 + c;
          const uint32_t cl = lds[P.cm_cls[c] + byte];
          const uint32_t e = *(const uint16_t*)(lds + P.cm_trans[c] + 2 * (row[c] + cl));
          row[c] = e >> 2;
          if constexpr (MODE == SET_COUNT) cnt[s] += (e >> 1) & 1u;
          if constexpr (MODE == SET_SEARCH) {
            if ((e & 2u) && re[s] < 0) re[s] = p;
            if ((e & 1u) && re[s] < 0) st[s] = p;
          }
          if constexpr (MODE == SET_MATCHES) hit |= (uint64_t)((e >> 1) & 1u) << s;
        }
      }
    };
    uint4 r[8];
    auto load = [&](int c) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int t = k * 8 + (lane >> 3);
        const uint64_t addr = fb[t] + (uint64_t)c * kSetChunk + 16u * (lane & 7);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (addr < fb[64 + t]) {
          const set_u32x4 x = __builtin_nontemporal_load((const set_u32x4*)(uintptr_t)addr);
          v = make_uint4(x.x, x.y, x.z, x.w);
        }
        r[k] = v;
      }
    };
    if (nch > 0) load(0);
    for (int c = 0; c < nch; ++c) {
#pragma unroll
      for (int k = 0; k < 8; ++k) *(uint4*)(tile + (k * 8 + (lane >> 3)) * kSetPitch + 16 * (lane & 7)) = r[k];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (c + 1 < nch) load(c + 1);
      const int p0 = c * kSetChunk - skew;   // text position of the chunk's first byte
      auto body = [&](auto masked) {
        for (int q = 0; q < kSetChunk / 16; ++q) {
          const uint4 v = *(const uint4*)(tile + lane * kSetPitch + 16 * q);
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int b = 0; b < 16; ++b) {
            const uint32_t byte = (w[b >> 2] >> (8 * (b & 3))) & 0xFFu;
            const int p = p0 + 16 * q + b;
            if constexpr (decltype(masked)::value) {
              if (p >= 0 && p < L) step(byte, p);
            } else {
              step(byte, p);
            }
          }
        }
      };
      if (__all(!live || (skew == 0 && p0 + kSetChunk <= L))) body(std::false_type{});
      else body(std::true_type{});
      __builtin_amdgcn_wave_barrier();   // (the tile is rewritten by the next chunk)
      if constexpr (MODE != SET_COUNT) {
        bool done = !live || (c + 1) * kSetChunk >= flen;
        if constexpr (MODE == SET_SEARCH) {
          bool all = true;
#pragma unroll
          for (int s = 0; s < NS; ++s) all = all && re[s] >= 0;
          done = done || all;
        } else {
          done = done || (hit & used) == used;
        }
        if (__all(done)) break;
      }
    }
    if (!live) continue;
    // end of the text: an accepting walk is a match that ends there
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (!((used >> s) & 1ull)) continue;
      uint32_t acc;
      int j, fixed;
      if (s < NCG * 4) {
        const int g = s >> 2;
        acc = (P.col_acc[g] >> (sh[s < NCG * 4 ? s : 0] >> 2)) & 1u;
        j = P.col_j[s];
        fixed = P.col_fixed[s];
      } else {
        const int c = s - NCG * 4 < NCM ? s - NCG * 4 : 0;
        acc = lds[P.cm_acc[c] + (row[c] >> P.cm_shift[c])];
        j = P.cm_j[c];
        fixed = P.cm_fixed[c];
      }
      const int64_t o = i * P.k + j;
      if constexpr (MODE == SET_COUNT) o0[o] = cnt[s] + (int32_t)acc;
      if constexpr (MODE == SET_SEARCH) {
        if (acc && re[s] < 0) re[s] = L;
        o0[o] = re[s] < 0 ? -1 : fixed > 0 ? re[s] - fixed : st[s];
        o1[o] = re[s];
      }
      if constexpr (MODE == SET_MATCHES) {
        if (((hit >> s) & 1ull) || acc) bits[i * P.words + (j >> 6)] |= 1ull << (j & 63);
      }
    }
  }
}

// own-route member j: its single-pattern answer (scratch, n entries) into column j
__global__ __launch_bounds__(256) void k_set_scatter(int mode, int64_t n, int k, int words, int j,
                                                     const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                     int32_t* __restrict__ o0, int32_t* __restrict__ o1,
                                                     uint64_t* __restrict__ bits) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (mode == SET_MATCHES) {
      if (a[i] >= 0) bits[i * words + (j >> 6)] |= 1ull << (j & 63);
    } else {
      o0[i * k + j] = a[i];
      if (mode == SET_SEARCH) o1[i * k + j] = b[i];
    }
  }
}

// ---- findall of a set (mrx_set_findall_dev): the text-major CSR of every member's findall spans ----------------
// phase 1, behind member j's count into cnt[n]: row_total[i] += cnt[i]; member_total += the member's sum (a wavefront
// reduction, the block's four sums through LDS, then one atomic per block: one atomic per wavefront serialised 16 K
// atomics on one address for 2^20 texts, 0.17 ms a member)
__global__ __launch_bounds__(256) void k_setfa_add(int64_t n, const int32_t* __restrict__ cnt, int64_t* __restrict__ row_total,
                                                   unsigned long long* __restrict__ member_total) {
  __shared__ int64_t part[4];
  int64_t acc = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = cnt[i];
    row_total[i] += c;
    acc += c;
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) acc += __shfl_xor(acc, d);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t sum = part[0] + part[1] + part[2] + part[3];
    if (sum != 0) atomicAdd(member_total, (unsigned long long)sum);
  }
}

// phase 2, behind member j's findall (prefix_j[n + 1], spans_j[m]): one lane per SPAN -- coalesced reads and even work
// whatever the texts hold (a lane per text diverges on dense texts).  Span s belongs to the last text i
// with prefix_j[i] <= s and goes to text_prefix[i] + before[i] + (s - prefix_j[i]), before[i] = the spans of members
// 0..j-1 in text i.  Each wavefront takes one contiguous run of spans, 256 per round (four per lane): it bisects all n
// texts once for its first span, then per round gallops forward from the last round's text to the text of the
// round's last span (uniform, broadcast loads), and each lane bisects only the texts between the two.  (A bisection
// of all n texts per 256 spans was bound by its 20 dependent loads: 0.43 ms a member for 2 * 10^7 spans.)  A findall
// that disagreed with its count can never write outside its text's range.
__global__ __launch_bounds__(256) void k_setfa_place(int64_t n, int j, int64_t m, const int64_t* __restrict__ prefix_j,
                                                     const int32_t* __restrict__ spans_j,
                                                     const int64_t* __restrict__ text_prefix,
                                                     const int64_t* __restrict__ before, int64_t span_cap,
                                                     int32_t* __restrict__ members, int32_t* __restrict__ spans) {
  const int64_t got = prefix_j[n] < m ? prefix_j[n] : m;
  const int lane = (int)threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4, w = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  const int64_t per = ((got + nw - 1) / nw + 255) & ~(int64_t)255;
  const int64_t s_begin = w * per, s_end = s_begin + per < got ? s_begin + per : got;
  if (s_begin >= s_end) return;
  auto last_text = [&](int64_t a, int64_t b, int64_t s) {   // the last i in [a, b) with prefix_j[i] <= s (prefix_j[a] <= s)
    while (b - a > 1) {
      const int64_t mid = (a + b) >> 1;
      if (prefix_j[mid] <= s) a = mid; else b = mid;
    }
    return a;
  };
  int64_t cur = last_text(0, n, s_begin);
  for (int64_t b0 = s_begin; b0 < s_end; b0 += 256) {
    const int64_t last = b0 + 255 < s_end ? b0 + 255 : s_end - 1;
    int64_t hi = cur, step = 1;
    while (hi + step < n && prefix_j[hi + step] <= last) {
      hi += step;
      step <<= 1;
    }
    hi = last_text(hi, hi + step < n ? hi + step : n, last);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t s = b0 + lane + 64 * q;
      if (s > last) continue;
      const int64_t i = last_text(cur, hi + 1, s);
      const int64_t out = text_prefix[i] + before[i] + (s - prefix_j[i]);
      if (out < text_prefix[i + 1] && out < span_cap) {
        *(int2*)(spans + 2 * out) = *(const int2*)(spans_j + 2 * s);
        members[out] = j;
      }
    }
    cur = hi;
  }
}

// behind k_setfa_place: before[i] += member j's spans in text i
__global__ __launch_bounds__(256) void k_setfa_advance(int64_t n, const int64_t* __restrict__ prefix_j,
                                                       int64_t* __restrict__ before) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    before[i] += prefix_j[i + 1] - prefix_j[i];
}

// ---- sub of a set (mrx_set_sub_dev): the set's findall hits -> one selection per text -> output bytes -----------
// One wavefront per text walks it in windows of W positions (0 .. L: an empty hit may sit at L; W = the batch's
// longest text + 1 rounded up to 64, at most kSetSubMaxW).  Per window, the lanes stride over the text's hits
// (contiguous in the set's findall output) and every hit that starts in the window at or after `pos` does
// best[s - w0] = min(best, member << 32 | end): the candidate that the contract's ascending (s, j, e) order puts
// first at that start.  Then 64 positions at a time, one per lane, a ballot of the occupied positions drives the walk
// with wave-uniform values only: next occupied position >= pos (s_ff1), select it, pos = max(e, s + 1) read from that
// lane.  pos, the replacement count and (emit) the input / output cursors carry across windows, so a text of any
// length is served; each window re-reads all of the text's hits, so a text's cost grows as L / W x its hits.
// A text without hits takes neither window nor walk.
// select: the output size and the replacement count of every text.  emit: the same walk, behind the scan of the
// sizes, also assembles the bytes in a per-wavefront LDS ring of kSetSubRing bytes indexed by the output's address:
// every position not inside a selected hit is copied from the input to the offset that the last selected hit at or
// before it leaves, each selected hit writes its member's replacement (a lane alone up to 64 bytes, the whole
// wavefront beyond).  The ring goes to global memory as whole aligned 16-byte words, bytes only at the ends of a
// text's output row (its neighbours' words belong to other wavefronts).  A chunk whose output does not fit the ring
// (long replacements) is written byte by byte.  The walk is repeated rather than stored, so the hits are the only
// per-hit scratch.  Reads stay inside a text, writes inside its output row.
constexpr int kSetSubMaxW = 1536;             // positions per window at most: u64 best[W] per wavefront, 12 KiB
constexpr int kSetSubWaves = 4;
constexpr int kSetSubRing = 2048;             // emit: output ring per wavefront
constexpr int kSetSubFlushAt = 1024;          // ... flushed once this many bytes are pending
constexpr int kSetSubReplLds = 4096;          // the replacement table is staged in LDS up to this many bytes

struct SetSubArgs {   // (the batch's fields, not a TextBatch: with one, k_setsub_emit's scalar register count moved)
  const uint8_t* data;
  const int64_t* offsets;   // CSR, or NULL: fixed pitch
  int64_t stride;
  const int32_t* lens;
  int32_t len;
  int64_t n;
  const int64_t* text_prefix;   // the set's findall: text CSR, member and span of each hit
  const int32_t* members;
  const int32_t* spans;
  const uint8_t* rtab;      // the members' replacements back to back; member j's are [roff[j], roff[j + 1])
  const int64_t* roff;
  int64_t rbytes;
  int64_t count;            // > 0: at most count replacements per text
  int32_t k;
  int32_t W;                // window: a multiple of 64, at most kSetSubMaxW
};

__device__ __forceinline__ int64_t setsub_readlane64(int64_t v, int h) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, h);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), h);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t setsub_shfl64(int64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), src);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ void setsub_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool EMIT>
__device__ void setsub_text(const SetSubArgs& A, int64_t i, uint64_t* best, uint8_t* ring, const uint8_t* R, int lane,
                            int64_t* __restrict__ sizes, int32_t* __restrict__ nsub, const int64_t* __restrict__ out_off,
                            uint8_t* __restrict__ out) {
  int64_t a0;
  int32_t L;
  if (A.offsets) { a0 = A.offsets[i]; L = (int32_t)(A.offsets[i + 1] - a0); }
  else { a0 = i * A.stride; L = A.lens ? A.lens[i] : A.len; }
  const uint8_t* text = A.data + a0;
  const int64_t ha = A.text_prefix[i], hb = A.text_prefix[i + 1];
  if constexpr (!EMIT) {
    if (ha >= hb) {   // no hit: the text is its output
      if (lane == 0) { sizes[i] = L; nsub[i] = 0; }
      return;
    }
  }
  int64_t olen = 0;
  uint64_t ob = 0;           // emit: address of the text's output row
  if constexpr (EMIT) { ob = (uint64_t)(uintptr_t)(out + out_off[i]); olen = out_off[i + 1] - out_off[i]; }
  int64_t pend = 0, oend = 0;   // emit: the output before pend is in global memory, before oend in the ring
  // emit: [pend, upto) of the row from the ring to global memory: bytes up to the first 16-byte boundary, whole words,
  // and (final) the bytes behind the last boundary; else they wait for the next flush
  auto flush = [&](int64_t upto, bool final) {
    setsub_lds_sync();
    const uint64_t a = ob + (uint64_t)pend, b = ob + (uint64_t)upto;
    const uint64_t wa = (a + 15) & ~(uint64_t)15, wb = b & ~(uint64_t)15;
    const uint64_t hend = wa < b ? wa : b;
    for (uint64_t x = a + lane; x < hend; x += 64) *(uint8_t*)(uintptr_t)x = ring[x & (kSetSubRing - 1)];
    for (uint64_t w = wa + 16 * (uint64_t)lane; w + 16 <= wb; w += 1024)
      *(uint4*)(uintptr_t)w = *(const uint4*)(ring + (w & (kSetSubRing - 1)));
    uint64_t np = wb > hend ? wb : hend;
    if (final) {
      for (uint64_t x = np + lane; x < b; x += 64) *(uint8_t*)(uintptr_t)x = ring[x & (kSetSubRing - 1)];
      np = b;
    }
    pend = (int64_t)(np - ob);
    setsub_lds_sync();
  };
  int32_t pos = 0;           // no candidate that starts before pos can be selected
  int64_t reps = 0;
  bool live = ha < hb;       // replacements are still being selected (hits left, count not reached)
  int32_t cur = 0;           // emit: the input before cur is consumed ...
  int64_t ocur = 0;          // ... and fills the output before ocur
  int64_t delta = 0;         // select, per lane: replacement bytes minus matched bytes of its selected hits
  const int32_t W = A.W;
  for (int32_t w0 = 0; w0 <= L; w0 += W) {
    const int32_t wn = min(W, L + 1 - w0);
    const bool walk = live && pos < w0 + wn;
    if constexpr (!EMIT) {
      if (!live) break;
      if (!walk) continue;
    }
    if (walk) {
      const int wc = (wn + 63) & ~63;
      for (int x = lane; x < wc; x += 64) best[x] = ~0ull;
      setsub_lds_sync();
      const int32_t lo = max(w0, pos), hi = w0 + wn;
      for (int64_t q = ha + lane; q < hb; q += 64) {
        const int2 sp = *(const int2*)(A.spans + 2 * q);
        if (sp.x >= lo && sp.x < hi) {
          const int32_t j = A.members[q];
          const int32_t e = min(max(sp.y, sp.x), L);
          if ((uint32_t)j < (uint32_t)A.k)
            atomicMin((unsigned long long*)&best[sp.x - w0], ((unsigned long long)(uint32_t)j << 32) | (uint32_t)e);
        }
      }
      setsub_lds_sync();
    }
    const int32_t c0 = EMIT ? 0 : ((max(pos, w0) - w0) & ~63);
    for (int32_t c = c0; c < wn; c += 64) {
      const int32_t p = w0 + c + lane;
      uint32_t byte = 0;
      if constexpr (EMIT) {
        if (p < L) byte = text[p];
      }
      const int32_t cur_in = cur;
      const int64_t ocur_in = ocur;
      uint64_t sel = 0;
      int32_t e = 0, j = 0;
      int64_t rl = 0, my_o = 0;
      if (walk && live && pos < w0 + c + 64) {
        const uint64_t key = c + lane < wn ? best[c + lane] : ~0ull;
        const bool occupied = key != ~0ull;
        const uint64_t occ = __ballot(occupied);
        e = (int32_t)(uint32_t)key;
        j = occupied ? (int32_t)(key >> 32) : 0;
        if (occupied) rl = A.roff[j + 1] - A.roff[j];
        const int32_t nxt = max(e, p + 1);
        while (true) {
          const int32_t rel = pos - (w0 + c);
          if (rel >= 64) break;
          const uint64_t m = rel <= 0 ? occ : (occ & (~0ull << rel));
          if (!m) break;
          const int h = __builtin_ctzll(m);
          sel |= 1ull << h;
          pos = __builtin_amdgcn_readlane(nxt, h);
          if constexpr (EMIT) {
            const int64_t o = ocur + (int64_t)(w0 + c + h - cur);
            if (lane == h) my_o = o;
            ocur = o + setsub_readlane64(rl, h);
            cur = __builtin_amdgcn_readlane(e, h);
          }
          ++reps;
          if (A.count > 0 && reps >= A.count) { live = false; break; }
        }
      }
      const bool mine = (sel >> lane) & 1ull;
      if constexpr (!EMIT) {
        if (mine) delta += rl - (int64_t)(e - p);
      } else {
        // this chunk writes the output [oend, oend_new): into the ring, or byte by byte when it does not fit
        const int32_t cend = min(w0 + c + 64, L);
        const int64_t oend_new = cur >= cend ? ocur : ocur + (cend - cur);
        bool direct = false;
        if (oend_new - pend > kSetSubRing) {
          flush(oend, false);
          if (oend_new - pend > kSetSubRing) {
            flush(oend, true);
            direct = true;
          }
        }
        auto put = [&](int64_t o, uint8_t v) {
          if (o < olen) {
            const uint64_t x = ob + (uint64_t)o;
            if (direct) *(uint8_t*)(uintptr_t)x = v;
            else ring[x & (kSetSubRing - 1)] = v;
          }
        };
        // the member's replacement at my_o
        const uint8_t* rp = R + (mine ? A.roff[j] : 0);
        if (mine && rl <= 64)
          for (int64_t t = 0; t < rl; ++t) put(my_o + t, rp[t]);
        uint64_t longm = __ballot(mine && rl > 64);
        while (longm) {
          const int h = __builtin_ctzll(longm);
          longm &= longm - 1;
          const int64_t o = setsub_readlane64(my_o, h), n_r = setsub_readlane64(rl, h);
          const int32_t jh = __builtin_amdgcn_readlane(j, h);
          const uint8_t* src = R + A.roff[jh];
          for (int64_t t = lane; t < n_r; t += 64) put(o + t, src[t]);
        }
        // my byte: copied unless a selected hit covers it, behind the last selected hit at or before it
        const uint64_t upto = sel & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
        const int src = upto ? 63 - __builtin_clzll(upto) : lane;
        const int32_t e_src = __shfl(e, src);
        const int64_t o_src = setsub_shfl64(my_o + rl, src);
        const int32_t cs = upto ? e_src : cur_in;
        const int64_t os = upto ? o_src : ocur_in;
        if (p < L && p >= cs) put(os + (p - cs), (uint8_t)byte);
        oend = oend_new;
        if (direct) pend = oend;
        else if (oend - pend >= kSetSubFlushAt) flush(oend, false);
      }
    }
    if (walk) setsub_lds_sync();   // (best[] is rewritten by the next window)
  }
  if constexpr (EMIT) {
    flush(oend < olen ? oend : olen, true);
  } else {
#pragma unroll
    for (int d = 32; d; d >>= 1) delta += setsub_shfl64(delta, lane ^ d);
    if (lane == 0) {
      sizes[i] = (int64_t)L + delta;
      nsub[i] = (int32_t)reps;
    }
  }
}

__device__ __forceinline__ const uint8_t* setsub_stage_repl(const SetSubArgs& A, uint8_t* lds_r) {
  if (A.rbytes > kSetSubReplLds) return A.rtab;
  for (int64_t x = threadIdx.x; x < A.rbytes; x += blockDim.x) lds_r[x] = A.rtab[x];
  __syncthreads();
  return lds_r;
}

// LDS: u64 best[W] per wavefront; emit adds a ring per wavefront and the replacement table (when it fits)
__global__ __launch_bounds__(64 * kSetSubWaves) void k_setsub_select(const SetSubArgs A, int64_t* __restrict__ sizes,
                                                                     int32_t* __restrict__ nsub) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  uint64_t* best = (uint64_t*)lds + wave * A.W;
  for (int64_t i = (int64_t)blockIdx.x * kSetSubWaves + wave; i < A.n; i += (int64_t)gridDim.x * kSetSubWaves)
    setsub_text<false>(A, i, best, nullptr, nullptr, lane, sizes, nsub, nullptr, nullptr);
}

__global__ __launch_bounds__(64 * kSetSubWaves) void k_setsub_emit(const SetSubArgs A, const int64_t* __restrict__ out_off,
                                                                   uint8_t* __restrict__ out) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  uint64_t* best = (uint64_t*)lds + wave * A.W;
  uint8_t* rings = lds + sizeof(uint64_t) * kSetSubWaves * A.W;
  const uint8_t* R = setsub_stage_repl(A, rings + kSetSubWaves * kSetSubRing);
  for (int64_t i = (int64_t)blockIdx.x * kSetSubWaves + wave; i < A.n; i += (int64_t)gridDim.x * kSetSubWaves)
    setsub_text<true>(A, i, best, rings + wave * kSetSubRing, R, lane, nullptr, nullptr, out_off, out);
}

}  // namespace
}  // namespace mrx

using namespace mrx;

// ---------------------------------------------------------------------------------------------------------------
// host: the set plan
// ---------------------------------------------------------------------------------------------------------------
struct mrx_set {
  struct Pass {
    SetPassDev dv{};
    std::vector<uint8_t> blob;    // LDS image, a multiple of 16 bytes
    std::vector<int> members;
  };
  struct Plan {                   // one per operation family: [0] count, [1] search and matches
    std::vector<Pass> passes;
    std::vector<int> pass_of, slot_of;   // per member: pass / slot (-1: own route)
    std::vector<std::string> why_own;    // per member: why it keeps its own route
    std::string refusal;                 // "member j: reason" -- the operation is refused for the set
  };
  std::vector<mrx_handle*> members;
  std::vector<std::string> patterns;
  uint32_t options = 0;
  Plan plan[2];
  std::mutex mu;
  std::map<std::pair<int, int>, uint8_t*> d_blobs;   // (device, plan * 4096 + pass) -> uploaded table image
  ~mrx_set() {
    for (auto& kv : d_blobs) (void)hipFree(kv.second);
    for (mrx_handle* h : members) mrx_free(h);
  }
};

namespace {

// the member's walk as a column slot (u16[256]) or a class member (cls | trans | acc); false: too large for a pass
struct MemberTables {
  bool column = false;
  std::array<uint16_t, 256> col{};
  uint32_t acc_bits = 0;   // column: bit q = state q accepts
  std::array<uint8_t, 256> cls{};
  int cshift = 0;
  std::vector<uint16_t> trans;
  std::vector<uint8_t> acc;
  int fixed = 0;
  size_t bytes() const { return column ? 0 : (size_t)((256 + trans.size() * 2 + acc.size() + 15) & ~size_t(15)); }
};

bool member_tables(const HostPlan& hp, MemberTables& t, std::string& why) {
  const auto& E = hp.st_entries;
  const int nlive = (int)E.size();
  if (nlive == 0 || hp.st_live_acc.size() != E.size()) { why = "no search automaton"; return false; }
  t.fixed = hp.dev.st_fixed_len;
  if (nlive <= 4) {
    t.column = true;
    for (int c = 0; c < 256; ++c)
      for (int q = 0; q < nlive; ++q) t.col[c] |= (uint16_t)((E[q][c] & 0xF) << (4 * q));
    for (int q = 0; q < nlive; ++q)
      if (hp.st_live_acc[q]) t.acc_bits |= 1u << q;
    return true;
  }
  std::map<std::vector<uint16_t>, int> seen;
  int ncls = 0;
  for (int c = 0; c < 256; ++c) {
    std::vector<uint16_t> colv(nlive);
    for (int q = 0; q < nlive; ++q) colv[q] = E[q][c];
    auto it = seen.find(colv);
    if (it == seen.end()) it = seen.emplace(colv, ncls++).first;
    t.cls[c] = (uint8_t)it->second;
  }
  while ((1 << t.cshift) < ncls) ++t.cshift;
  const int ncp = 1 << t.cshift;
  if ((int64_t)nlive * ncp > kSetClsEntries) { why = "search automaton too large for a set pass's LDS tables"; return false; }
  t.trans.assign((size_t)nlive * ncp, 0);
  for (int c = 0; c < 256; ++c)
    for (int q = 0; q < nlive; ++q) {
      const uint16_t e = E[q][c];
      t.trans[(size_t)q * ncp + t.cls[c]] = (uint16_t)((((e >> 2) << t.cshift) << 2) | (e & 3));
    }
  t.acc = hp.st_live_acc;
  return true;
}

void put(std::vector<uint8_t>& b, const void* p, size_t n) {
  const uint8_t* q = (const uint8_t*)p;
  b.insert(b.end(), q, q + n);
}
void pad16(std::vector<uint8_t>& b) { b.resize((b.size() + 15) & ~size_t(15), 0); }

// packs the eligible members of one operation family into passes (in member order)
void build_set_plan(mrx_set& s, int fam) {
  mrx_set::Plan& pl = s.plan[fam];
  const int k = (int)s.members.size();
  pl.pass_of.assign(k, -1);
  pl.slot_of.assign(k, -1);
  pl.why_own.assign(k, std::string());
  std::vector<MemberTables> tabs(k);
  std::vector<int> cols, clsm;
  for (int j = 0; j < k; ++j) {
    const mrx_handle* h = s.members[j];
    const bool streams = fam == 0 ? handle_count_streams(h) : handle_search_streams(h);
    if (!streams) {
      const HostPlan& hp = handle_plan(h);
      pl.why_own[j] = fam == 1 && (hp.dev.flags & PF_STREAMABLE) ? "search is not the streaming walk (prefilter)"
                      : hp.streamable_why_not.empty() ? "not streamable" : hp.streamable_why_not;
      continue;
    }
    if (!member_tables(handle_plan(h), tabs[j], pl.why_own[j])) continue;
    (tabs[j].column ? cols : clsm).push_back(j);
  }
  // passes: column groups first (four members per group), then class members, within the pass budgets
  size_t ci = 0, mi = 0;
  while (ci < cols.size() || mi < clsm.size()) {
    mrx_set::Pass ps;
    SetPassDev& d = ps.dv;
    for (int x = 0; x < kSetMaxCG * 4; ++x) d.col_j[x] = -1;
    for (int x = 0; x < kSetMaxCM; ++x) d.cm_j[x] = -1;
    int members = 0;
    size_t bytes = 0;
    std::vector<std::array<uint64_t, 256>> groups;
    while (ci < cols.size() && members < kSetPassMembers && (int)groups.size() < kSetMaxCG && bytes + 2048 <= (size_t)kSetTableBudget) {
      groups.emplace_back();
      auto& G = groups.back();
      G.fill(0);
      const int g = (int)groups.size() - 1;
      for (int m = 0; m < 4 && ci < cols.size() && members < kSetPassMembers; ++m, ++ci, ++members) {
        const int j = cols[ci];
        for (int c = 0; c < 256; ++c) G[c] |= (uint64_t)tabs[j].col[c] << (16 * m);
        d.col_j[g * 4 + m] = j;
        d.col_fixed[g * 4 + m] = tabs[j].fixed;
        d.col_acc[g] |= tabs[j].acc_bits << (4 * m);
        pl.pass_of[j] = (int)s.plan[fam].passes.size();
        pl.slot_of[j] = g * 4 + m;
        ps.members.push_back(j);
      }
      bytes += 2048;
    }
    d.ncg = (int)groups.size();
    for (auto& G : groups) put(ps.blob, G.data(), 2048);
    while (mi < clsm.size() && members < kSetPassMembers && d.ncm < kSetMaxCM &&
           bytes + tabs[clsm[mi]].bytes() <= (size_t)kSetTableBudget) {
      const int j = clsm[mi++];
      const MemberTables& t = tabs[j];
      const int c = d.ncm++;
      d.cm_j[c] = j;
      d.cm_fixed[c] = t.fixed;
      d.cm_shift[c] = t.cshift;
      d.cm_cls[c] = (int)ps.blob.size();
      put(ps.blob, t.cls.data(), 256);
      d.cm_trans[c] = (int)ps.blob.size();
      put(ps.blob, t.trans.data(), t.trans.size() * 2);
      d.cm_acc[c] = (int)ps.blob.size();
      put(ps.blob, t.acc.data(), t.acc.size());
      pad16(ps.blob);
      bytes = ps.blob.size();
      pl.pass_of[j] = (int)s.plan[fam].passes.size();
      pl.slot_of[j] = kSetMaxCG * 4 + c;
      ps.members.push_back(j);
      ++members;
    }
    pad16(ps.blob);
    d.table_bytes = (int)ps.blob.size();
    d.k = k;
    d.words = (k + 63) / 64;
    pl.passes.push_back(std::move(ps));
  }
}

// CPU walk of one pass's packed tables over one text (mrx_testing_set_run): the kernel's arithmetic, byte by byte
void set_pass_run_host(const mrx_set::Pass& ps, int mode, const uint8_t* text, int len, int32_t* out) {
  const SetPassDev& d = ps.dv;
  const uint8_t* lds = ps.blob.data();
  auto finish = [&](int j, uint32_t acc, int32_t cnt, int32_t st, int32_t re, bool hit, int fixed) {
    if (mode == SET_COUNT) out[j] = cnt + (int32_t)acc;
    if (mode == SET_SEARCH) {
      if (acc && re < 0) re = len;
      out[2 * j] = re < 0 ? -1 : fixed > 0 ? re - fixed : st;
      out[2 * j + 1] = re;
    }
    if (mode == SET_MATCHES) out[j] = (hit || acc) ? 1 : 0;
  };
  for (int s = 0; s < d.ncg * 4; ++s) {
    if (d.col_j[s] < 0) continue;
    const int g = s >> 2, m = s & 3;
    uint32_t sh = 16u * m;
    int32_t cnt = 0, st = -1, re = -1;
    bool hit = false;
    for (int p = 0; p < len; ++p) {
      uint64_t col;
      memcpy(&col, lds + (size_t)(g * 256 + text[p]) * 8, 8);
      const uint32_t f = (uint32_t)(col >> sh) & 15u;
      sh = 16u * m + (f & 12u);
      cnt += (f >> 1) & 1u;
      hit = hit || (f & 2u);
      if ((f & 2u) && re < 0) re = p;
      if ((f & 1u) && re < 0) st = p;
    }
    finish(d.col_j[s], (d.col_acc[g] >> (sh >> 2)) & 1u, cnt, st, re, hit, d.col_fixed[s]);
  }
  for (int c = 0; c < d.ncm; ++c) {
    uint32_t row = 0;
    int32_t cnt = 0, st = -1, re = -1;
    bool hit = false;
    for (int p = 0; p < len; ++p) {
      const uint32_t cl = lds[d.cm_cls[c] + text[p]];
      uint16_t e;
      memcpy(&e, lds + d.cm_trans[c] + 2 * (row + cl), 2);
      row = e >> 2;
      cnt += (e >> 1) & 1u;
      hit = hit || (e & 2u);
      if ((e & 2u) && re < 0) re = p;
      if ((e & 1u) && re < 0) st = p;
    }
    finish(d.cm_j[c], lds[d.cm_acc[c] + (row >> d.cm_shift[c])], cnt, st, re, hit, d.cm_fixed[c]);
  }
}

// the route rule: shared pass for this batch shape?  Never by default (see the head of this file).
bool set_shared_route(const TextBatch& /*b*/, int64_t /*n*/) {
  return g_set_route.load(std::memory_order_relaxed) == 1;
}

hipError_t set_upload(mrx_set* s, int fam, int pi, int dev, const uint8_t** out) {
  std::lock_guard<std::mutex> g(s->mu);
  auto key = std::make_pair(dev, fam * 4096 + pi);
  auto it = s->d_blobs.find(key);
  if (it != s->d_blobs.end()) { *out = it->second; return hipSuccess; }
  const auto& b = s->plan[fam].passes[pi].blob;
  uint8_t* p = nullptr;
  hipError_t e = hipMalloc((void**)&p, std::max<size_t>(b.size(), 16));
  if (e != hipSuccess) return e;
  e = hipMemcpy(p, b.data(), b.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(p); return e; }
  s->d_blobs[key] = p;
  *out = p;
  return hipSuccess;
}

// blocks of `per` items each, at least one and at most 4096 (the kernels stride over what is left)
unsigned set_grid(int64_t items, int per = 256) {
  const int64_t g = (items + per - 1) / per;
  return (unsigned)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}

// "member j: reason" if a member's count / search would be refused: asked before anything is enqueued
std::string set_refusal(const mrx_set* s) {
  for (size_t j = 0; j < s->members.size(); ++j) {
    const std::string why = handle_refusal(s->members[j]);
    if (!why.empty()) return "member " + std::to_string(j) + ": " + why;
  }
  return std::string();
}

template <int MODE>
void launch_pass(const SetPassDev& d, const uint8_t* blob, const TextBatch& b, int64_t n, int32_t* o0, int32_t* o1,
                 uint64_t* bits, hipStream_t s) {
  const dim3 grid(set_grid((n + 63) / 64, kSetWaves)), block(64 * kSetWaves);
  const size_t lds = (size_t)d.table_bytes + kSetWaves * (kSetTile + kSetFrameBytes);
  if (d.ncg <= 2 && d.ncm <= 2)
    hipLaunchKernelGGL((k_set_scan<MODE, 2, 2>), grid, block, lds, s, d, blob, b, n, o0, o1, bits);
  else
    hipLaunchKernelGGL((k_set_scan<MODE, kSetMaxCG, kSetMaxCM>), grid, block, lds, s, d, blob, b, n, o0, o1, bits);
}

// known_total / known_max: a CSR batch's bounds where the caller has them (< 0: not; set filter), for the members' search
int set_run(const mrx_set* sc, int mode, const TextBatch& tb, int64_t n, int32_t* o0, int32_t* o1, uint64_t* bits,
            void* st, int64_t known_total = -1, int64_t known_max = -1) {
  if (!sc) return internal_fail(MRX_E_ARGUMENT, "null set");
  mrx_set* s = const_cast<mrx_set*>(sc);
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (int rc = check_batch(tb, BATCH_PITCH)) return rc;
  if (n > 0 && (!tb.data || (mode == SET_MATCHES ? !bits : (!o0 || (mode == SET_SEARCH && !o1)))))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  const int fam = mode == SET_COUNT ? 0 : 1;
  const mrx_set::Plan& pl = s->plan[fam];
  const int k = (int)s->members.size();
  const std::string refused = set_refusal(s);
  if (!refused.empty()) return internal_fail(MRX_E_UNSUPPORTED, refused);
  int dev = 0;
  MRX_HIP_TRY(hipGetDevice(&dev));
  if (n == 0) return MRX_OK;
  hipStream_t hs = (hipStream_t)st;
  const bool shared = set_shared_route(tb, n);
  const int words = (k + 63) / 64;
  ScratchScope scope_(st);
  if (mode == SET_MATCHES) MRX_HIP_TRY(hipMemsetAsync(bits, 0, sizeof(uint64_t) * (size_t)n * words, hs));
  int32_t* a = nullptr;
  int32_t* b = nullptr;
  for (int j = 0; j < k; ++j) {
    if (shared && pl.pass_of[j] >= 0) continue;
    if (!a) {
      a = (int32_t*)scratch_get(sizeof(int32_t) * 2 * (size_t)n, st);
      if (!a) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
      b = a + n;
    }
    const mrx_handle* h = s->members[j];
    int rc;
    if (mode == SET_COUNT)
      rc = tb.offsets ? mrx_count_dev(h, tb.data, tb.offsets, n, a, st)
                      : mrx_count_strided_dev(h, tb.data, tb.stride, tb.lens, tb.len, n, a, st);
    else
      rc = member_search(h, tb, n, a, b, st, known_total, known_max);
    if (rc != MRX_OK) return internal_fail(rc, "member " + std::to_string(j) + ": " + mrx_last_error());
    hipLaunchKernelGGL(k_set_scatter, dim3(set_grid(n)), dim3(256), 0, hs, mode, n, k, words, j, a, b, o0, o1, bits);
    MRX_HIP_TRY(hipGetLastError());
  }
  if (shared && !pl.passes.empty()) {
    void* tm = scan_timer_begin(st);
    for (int pi = 0; pi < (int)pl.passes.size(); ++pi) {
      const uint8_t* d_blob = nullptr;
      MRX_HIP_TRY(set_upload(s, fam, pi, dev, &d_blob));
      const SetPassDev& d = pl.passes[pi].dv;
      if (mode == SET_COUNT) launch_pass<SET_COUNT>(d, d_blob, tb, n, o0, o1, bits, hs);
      else if (mode == SET_SEARCH) launch_pass<SET_SEARCH>(d, d_blob, tb, n, o0, o1, bits, hs);
      else launch_pass<SET_MATCHES>(d, d_blob, tb, n, o0, o1, bits, hs);
      MRX_HIP_TRY(hipGetLastError());
    }
    scan_timer_end(tm);
    set_last_kernel("k_set_scan");
  } else {
    set_last_kernel("k_set_member_loop");
  }
  return MRX_OK;
}

// Two phases: every member's count sizes each text's row and each member's total (one stream
// synchronisation); then every member with a match runs its findall into scratch of exactly its total, and
// k_setfa_place moves the spans into the text-major output.  Scratch: O(n) words plus the densest member's spans,
// whatever k is (the arena is rewound behind each member's call).  The phases are separate calls so that a caller
// (set sub) can allocate the hits' buffers once their total is known; both run inside the caller's scratch scope.
struct SetFaRun {
  int64_t kt = -1, km = -1;      // the CSR batch's byte count and longest text, once for every member
  int64_t* before = nullptr;     // [n] spans of the members placed so far, per text
  int64_t* pre_j = nullptr;      // [n + 1] one member's findall CSR
  std::vector<int64_t> h_mt;     // [k] member totals, [k] the total
  int64_t total() const { return h_mt.back(); }
};

// phase 1: counts -> d_text_prefix[n + 1] and the member totals (one synchronisation); n > 0
int set_findall_count(const mrx_set* sc, const TextBatch& b, int64_t n, int64_t known_total, int64_t known_max,
                      int64_t* d_text_prefix, SetFaRun& r, void* st) {
  const int k = (int)sc->members.size();
  hipStream_t hs = (hipStream_t)st;
  if (b.offsets) {
    if (known_total >= 0 && known_max >= 0) { r.kt = known_total; r.km = known_max; }
    else if (int rc = batch_bounds(b.offsets, n, st, &r.kt, &r.km)) return rc;
  }
  int32_t* cnt = (int32_t*)scratch_get(sizeof(int32_t) * (size_t)n, st);
  int64_t* row = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, st);
  r.before = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, st);
  r.pre_j = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(n + 1), st);
  int64_t* mt = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(k + 1), st);   // [k] member totals, [k] the total
  if (!cnt || !row || !r.before || !r.pre_j || !mt) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  MRX_HIP_TRY(hipMemsetAsync(row, 0, sizeof(int64_t) * (size_t)n, hs));
  MRX_HIP_TRY(hipMemsetAsync(mt, 0, sizeof(int64_t) * (size_t)(k + 1), hs));
  const ScratchMark mark = scratch_mark(st);
  for (int j = 0; j < k; ++j) {
    const int rc = member_count(sc->members[j], b, n, cnt, st, r.kt, r.km);
    if (rc != MRX_OK) return internal_fail(rc, "member " + std::to_string(j) + ": " + mrx_last_error());
    hipLaunchKernelGGL(k_setfa_add, dim3(std::min(set_grid(n), 1024u)), dim3(256), 0, hs, n, cnt, row,
                       (unsigned long long*)(mt + j));
    MRX_HIP_TRY(hipGetLastError());
    scratch_rewind(st, mark);
  }
  if (int rc = exclusive_scan(row, n, d_text_prefix, mt + k, st)) return rc;
  r.h_mt.assign((size_t)k + 1, 0);
  MRX_HIP_TRY(hipMemcpyAsync(r.h_mt.data(), mt, sizeof(int64_t) * (size_t)(k + 1), hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));
  return MRX_OK;
}

// phase 2: the spans of the members that match, into d_members / d_spans (capacity span_cap >= r.total())
int set_findall_place(const mrx_set* sc, const TextBatch& b, int64_t n, const SetFaRun& r, const int64_t* d_text_prefix,
                      int32_t* d_members, int32_t* d_spans, int64_t span_cap, void* st) {
  const int k = (int)sc->members.size();
  hipStream_t hs = (hipStream_t)st;
  const int64_t densest = *std::max_element(r.h_mt.begin(), r.h_mt.begin() + k);
  int32_t* sp_j = (int32_t*)scratch_get(sizeof(int32_t) * 2 * (size_t)densest, st);
  if (!sp_j) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  MRX_HIP_TRY(hipMemsetAsync(r.before, 0, sizeof(int64_t) * (size_t)n, hs));
  const ScratchMark mark2 = scratch_mark(st);
  for (int j = 0; j < k; ++j) {
    const int64_t m = r.h_mt[j];
    if (m == 0) continue;
    const int rc = member_findall(sc->members[j], b, n, r.pre_j, sp_j, m, st, r.kt, r.km);
    if (rc == MRX_E_CAPACITY)
      return internal_fail(MRX_E_NO_DEVICE, "internal error: member " + std::to_string(j) + ": findall disagrees with count");
    if (rc != MRX_OK) return internal_fail(rc, "member " + std::to_string(j) + ": " + mrx_last_error());
    hipLaunchKernelGGL(k_setfa_place, dim3(set_grid(m)), dim3(256), 0, hs, n, j, m, r.pre_j, sp_j, d_text_prefix, r.before,
                       span_cap, d_members, d_spans);
    hipLaunchKernelGGL(k_setfa_advance, dim3(set_grid(n)), dim3(256), 0, hs, n, r.pre_j, r.before);
    MRX_HIP_TRY(hipGetLastError());
    scratch_rewind(st, mark2);
  }
  return MRX_OK;
}

int set_findall(const mrx_set* sc, const TextBatch& b, int64_t n, int64_t known_total, int64_t known_max,
                int64_t* d_text_prefix, int32_t* d_members, int32_t* d_spans, int64_t span_cap, int64_t* total, void* st) {
  if (!sc) return internal_fail(MRX_E_ARGUMENT, "null set");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (span_cap < 0) return internal_fail(MRX_E_ARGUMENT, "span_cap must be >= 0");
  if (int rc = check_batch(b, BATCH_PITCH)) return rc;
  if (!d_text_prefix || (n > 0 && span_cap > 0 && (!d_members || !d_spans)))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  if ((uintptr_t)d_spans & 7) return internal_fail(MRX_E_ARGUMENT, "d_spans must be 8-byte aligned");
  const std::string refused = set_refusal(sc);
  if (!refused.empty()) return internal_fail(MRX_E_UNSUPPORTED, refused);
  int dev = 0;
  MRX_HIP_TRY(hipGetDevice(&dev));
  hipStream_t hs = (hipStream_t)st;
  if (total) *total = 0;
  if (n == 0) {
    MRX_HIP_TRY(hipMemsetAsync(d_text_prefix, 0, sizeof(int64_t), hs));
    return MRX_OK;
  }
  ScratchScope scope_(st);
  SetFaRun r;
  if (int rc = set_findall_count(sc, b, n, known_total, known_max, d_text_prefix, r, st)) return rc;
  const int64_t tot = r.total();
  if (total) *total = tot;
  if (tot > span_cap)
    return internal_fail(MRX_E_CAPACITY, "span buffer too small: need " + std::to_string(tot));
  set_last_kernel("k_set_findall");
  if (tot == 0) return MRX_OK;
  if (int rc = set_findall_place(sc, b, n, r, d_text_prefix, d_members, d_spans, span_cap, st)) return rc;
  set_last_kernel("k_set_findall");
  return MRX_OK;
}

// sub of a set: the set's findall into scratch (12 bytes per hit), k_setsub_select -> sizes and
// replacement counts, the device scan -> output offsets, one synchronisation for the output size, k_setsub_emit.
// Scratch: the hits, O(n) words and, while the members' findall runs, the densest member's spans.
int set_sub(const mrx_set* sc, const char* const* repls, const size_t* repl_lens, int64_t count, const TextBatch& b,
            int64_t n, int64_t known_total, int64_t known_max, int64_t* d_out_off, uint8_t* d_out, int64_t out_cap,
            int32_t* d_nsub, int64_t* total_bytes, void* st) {
  if (!sc) return internal_fail(MRX_E_ARGUMENT, "null set");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (count < 0) return internal_fail(MRX_E_ARGUMENT, "count must be >= 0");
  if (out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "out_cap must be >= 0");
  if (int rc = check_batch(b, BATCH_PITCH)) return rc;
  const int k = (int)sc->members.size();
  if (!repl_lens || !d_out_off || (out_cap > 0 && !d_out))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  std::vector<int64_t> roff((size_t)k + 1, 0);
  for (int j = 0; j < k; ++j) {
    if (repl_lens[j] > 0 && (!repls || !repls[j]))
      return internal_fail(MRX_E_ARGUMENT, "member " + std::to_string(j) + ": null replacement of nonzero length");
    roff[j + 1] = roff[j] + (int64_t)repl_lens[j];
  }
  // refusals before anything is enqueued: group references, then the members' own
  for (int j = 0; j < k; ++j)
    if (repl_lens[j] > 0 && repl_has_group_refs(std::string(repls[j], repl_lens[j])))
      return internal_fail(MRX_E_UNSUPPORTED,
                           "member " + std::to_string(j) + ": group references are not supported in a set's sub");
  const std::string refused = set_refusal(sc);
  if (!refused.empty()) return internal_fail(MRX_E_UNSUPPORTED, refused);
  int dev = 0;
  MRX_HIP_TRY(hipGetDevice(&dev));
  hipStream_t hs = (hipStream_t)st;
  if (total_bytes) *total_bytes = 0;
  if (n == 0) {
    MRX_HIP_TRY(hipMemsetAsync(d_out_off, 0, sizeof(int64_t), hs));
    set_last_kernel("k_set_sub");
    return MRX_OK;
  }
  ScratchScope scope_(st);
  // the set's findall, into scratch
  int64_t* text_prefix = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(n + 1), st);
  if (!text_prefix) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  SetFaRun r;
  if (int rc = set_findall_count(sc, b, n, known_total, known_max, text_prefix, r, st)) return rc;
  const int64_t hits = r.total();
  int32_t* members = (int32_t*)scratch_get(sizeof(int32_t) * (size_t)std::max<int64_t>(hits, 1), st);
  int32_t* spans = (int32_t*)scratch_get(sizeof(int32_t) * 2 * (size_t)std::max<int64_t>(hits, 1), st);
  int64_t* sizes = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, st);
  int64_t* d_total = (int64_t*)scratch_get(sizeof(int64_t), st);
  int64_t* d_roff = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(k + 1), st);
  uint8_t* d_rtab = (uint8_t*)scratch_get((size_t)roff[k] + 16, st);
  int32_t* nsub = d_nsub ? d_nsub : (int32_t*)scratch_get(sizeof(int32_t) * (size_t)n, st);
  if (!members || !spans || !sizes || !d_total || !d_roff || !d_rtab || !nsub)
    return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  if (hits > 0)
    if (int rc = set_findall_place(sc, b, n, r, text_prefix, members, spans, hits, st)) return rc;
  std::vector<uint8_t> rtab((size_t)roff[k] + 1);
  for (int j = 0; j < k; ++j)
    if (repl_lens[j]) memcpy(rtab.data() + roff[j], repls[j], repl_lens[j]);
  MRX_HIP_TRY(hipMemcpyAsync(d_roff, roff.data(), sizeof(int64_t) * (size_t)(k + 1), hipMemcpyHostToDevice, hs));
  if (roff[k]) MRX_HIP_TRY(hipMemcpyAsync(d_rtab, rtab.data(), (size_t)roff[k], hipMemcpyHostToDevice, hs));
  // the window: the longest text + 1 positions, rounded up to 64, at most kSetSubMaxW
  const int64_t longest = b.offsets ? r.km : b.pitch_longest();
  const int32_t W = (int32_t)std::min<int64_t>(kSetSubMaxW, std::max<int64_t>(64, (longest + 1 + 63) & ~int64_t(63)));
  SetSubArgs A{b.data, b.offsets, b.stride, b.lens, b.len, n, text_prefix, members, spans, d_rtab, d_roff, roff[k], count, k, W};
  const dim3 g(set_grid(n, kSetSubWaves));
  const size_t lds_best = sizeof(uint64_t) * kSetSubWaves * (size_t)W;
  const size_t lds_ring = (size_t)kSetSubWaves * kSetSubRing;
  const size_t lds_repl = roff[k] <= kSetSubReplLds ? (size_t)((roff[k] + 15) & ~int64_t(15)) : 0;
  hipLaunchKernelGGL(k_setsub_select, g, dim3(64 * kSetSubWaves), lds_best, hs, A, sizes, nsub);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(sizes, n, d_out_off, d_total, st)) return rc;
  int64_t tot = 0;
  MRX_HIP_TRY(hipMemcpyAsync(&tot, d_total, sizeof tot, hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));
  if (total_bytes) *total_bytes = tot;
  set_last_kernel("k_set_sub");
  if (tot > out_cap) return internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(tot));
  if (tot > 0) {
    hipLaunchKernelGGL(k_setsub_emit, g, dim3(64 * kSetSubWaves), lds_best + lds_ring + lds_repl, hs, A, d_out_off,
                       d_out);
    MRX_HIP_TRY(hipGetLastError());
  }
  return MRX_OK;
}

}  // namespace

extern "C" {

int mrx_set_compile(const char* const* patterns, const size_t* lens, int32_t k, uint32_t options, mrx_set** out) {
  if (!out) return internal_fail(MRX_E_ARGUMENT, "null argument");
  *out = nullptr;
  if (k < 1 || k > kSetMaxK) return internal_fail(MRX_E_ARGUMENT, "set size must be in [1, 256]");
  if (!patterns || !lens) return internal_fail(MRX_E_ARGUMENT, "null argument");
  mrx_set* s = new mrx_set();
  s->options = options;
  for (int j = 0; j < k; ++j) {
    mrx_handle* h = nullptr;
    const int rc = mrx_compile_ex(patterns[j], lens[j], options, &h);
    if (rc != MRX_OK) {
      const std::string msg = mrx_last_error();
      delete s;
      return internal_fail(rc, "member " + std::to_string(j) + ": " + msg);
    }
    s->members.push_back(h);
    s->patterns.emplace_back(patterns[j] ? std::string(patterns[j], lens[j]) : std::string());
  }
  try {
    build_set_plan(*s, 0);
    build_set_plan(*s, 1);
  } catch (const std::exception& e) {
    delete s;
    return internal_fail(MRX_E_UNSUPPORTED, e.what());
  }
  *out = s;
  return MRX_OK;
}

void mrx_set_free(mrx_set* s) { delete s; }

int32_t mrx_set_size(const mrx_set* s) { return s ? (int32_t)s->members.size() : 0; }

size_t mrx_set_describe(const mrx_set* s, char* buf, size_t cap) {
  std::ostringstream o;
  if (s) {
    o << "set k=" << s->members.size() << " count_passes=" << s->plan[0].passes.size()
      << " search_passes=" << s->plan[1].passes.size() << "\n";
    for (size_t j = 0; j < s->members.size(); ++j) {
      o << "member " << j << ":";
      for (int op = 0; op < 3; ++op) {
        const mrx_set::Plan& pl = s->plan[op == 0 ? 0 : 1];
        o << " " << kSetOpName[op] << "=";
        if (pl.pass_of[j] >= 0) {
          const int sl = pl.slot_of[j];
          o << "shared(pass " << pl.passes.size() << "/" << pl.pass_of[j] << ", ";
          if (sl < kSetMaxCG * 4) o << "column " << sl / 4 << "." << sl % 4 << ")";
          else o << "class " << sl - kSetMaxCG * 4 << ")";
        } else {
          o << "own";
        }
      }
      const std::string& w0 = s->plan[0].why_own[j];
      const std::string& w1 = s->plan[1].why_own[j];
      if (!w0.empty()) o << " count_own_why=\"" << w0 << "\"";
      if (!w1.empty()) o << " search_own_why=\"" << w1 << "\"";
      o << "\n";
    }
  }
  const std::string t = o.str();
  if (buf && cap) {
    const size_t m = std::min(cap - 1, t.size());
    memcpy(buf, t.data(), m);
    buf[m] = 0;
  }
  return t.size();
}

int mrx_set_search_dev(const mrx_set* s, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int32_t* d_start,
                       int32_t* d_end, void* stream) {
  const TextBatch b = csr(d_data, d_offsets);
  if (int rc = check_batch(b, BATCH_CSR)) return rc;
  return set_run(s, SET_SEARCH, b, n, d_start, d_end, nullptr, stream);
}
int mrx_set_search_strided_dev(const mrx_set* s, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                               int32_t len, int64_t n, int32_t* d_start, int32_t* d_end, void* stream) {
  return set_run(s, SET_SEARCH, strided(d_data, stride, d_lens, len), n, d_start, d_end, nullptr, stream);
}
int mrx_set_count_dev(const mrx_set* s, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int32_t* d_counts,
                      void* stream) {
  const TextBatch b = csr(d_data, d_offsets);
  if (int rc = check_batch(b, BATCH_CSR)) return rc;
  return set_run(s, SET_COUNT, b, n, d_counts, nullptr, nullptr, stream);
}
int mrx_set_count_strided_dev(const mrx_set* s, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                              int32_t len, int64_t n, int32_t* d_counts, void* stream) {
  return set_run(s, SET_COUNT, strided(d_data, stride, d_lens, len), n, d_counts, nullptr, nullptr, stream);
}
int mrx_set_matches_dev(const mrx_set* s, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, uint64_t* d_bits,
                        void* stream) {
  const TextBatch b = csr(d_data, d_offsets);
  if (int rc = check_batch(b, BATCH_CSR)) return rc;
  return set_run(s, SET_MATCHES, b, n, nullptr, nullptr, d_bits, stream);
}
int mrx_set_matches_strided_dev(const mrx_set* s, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                                int32_t len, int64_t n, uint64_t* d_bits, void* stream) {
  return set_run(s, SET_MATCHES, strided(d_data, stride, d_lens, len), n, nullptr, nullptr, d_bits, stream);
}

int mrx_set_findall_dev(const mrx_set* s, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        int64_t* d_text_prefix, int32_t* d_members, int32_t* d_spans, int64_t span_cap, int64_t* total,
                        void* stream) {
  const TextBatch b = csr(d_data, d_offsets);
  if (int rc = check_batch(b, BATCH_CSR)) return rc;
  return set_findall(s, b, n, -1, -1, d_text_prefix, d_members, d_spans, span_cap, total, stream);
}
int mrx_set_findall_known_dev(const mrx_set* s, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                              int64_t end_offset, int64_t max_text_len, int64_t* d_text_prefix, int32_t* d_members,
                              int32_t* d_spans, int64_t span_cap, int64_t* total, void* stream) {
  const TextBatch b = csr(d_data, d_offsets);
  if (int rc = check_batch(b, BATCH_CSR)) return rc;
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return set_findall(s, b, n, end_offset, max_text_len, d_text_prefix, d_members, d_spans, span_cap, total, stream);
}
int mrx_set_findall_strided_dev(const mrx_set* s, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                                int32_t len, int64_t n, int64_t* d_text_prefix, int32_t* d_members, int32_t* d_spans,
                                int64_t span_cap, int64_t* total, void* stream) {
  return set_findall(s, strided(d_data, stride, d_lens, len), n, -1, -1, d_text_prefix, d_members, d_spans, span_cap,
                     total, stream);
}
int mrx_set_findall_batch(const mrx_set* s, const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* text_prefix,
                          int32_t* members, int32_t* spans, int64_t span_cap, int64_t* total) {
  if (!s || n < 0 || !offsets || !text_prefix || (span_cap > 0 && (!members || !spans)))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (span_cap < 0) return internal_fail(MRX_E_ARGUMENT, "span_cap must be >= 0");
  // refusals before any device work, as the _dev entry points
  const std::string refused = set_refusal(s);
  if (!refused.empty()) return internal_fail(MRX_E_UNSUPPORTED, refused);
  DevBatch b; DevBuf<int64_t> pre; DevBuf<int32_t> mem, sp;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = pre.alloc((size_t)n + 1)) return rc;
  if (int rc = mem.alloc((size_t)span_cap)) return rc;
  if (int rc = sp.alloc(2 * (size_t)std::max<int64_t>(span_cap, 1))) return rc;
  int64_t tot = 0;
  const int rc = mrx_set_findall_known_dev(s, b.data, b.offsets, n, b.nbytes, b.longest, pre.p, mem.p, sp.p, span_cap,
                                           &tot, nullptr);
  if (total) *total = tot;
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  MRX_HIP_TRY(hipMemcpy(text_prefix, pre.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot > 0) {
    MRX_HIP_TRY(hipMemcpy(members, mem.p, sizeof(int32_t) * (size_t)tot, hipMemcpyDeviceToHost));
    MRX_HIP_TRY(hipMemcpy(spans, sp.p, sizeof(int32_t) * 2 * (size_t)tot, hipMemcpyDeviceToHost));
  }
  return rc;
}

int mrx_set_sub_dev(const mrx_set* s, const char* const* repls, const size_t* repl_lens, int64_t count,
                    const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_out_offsets, uint8_t* d_out_data,
                    int64_t out_cap, int32_t* d_nsub, int64_t* total_bytes, void* stream) {
  const TextBatch b = csr(d_data, d_offsets);
  if (int rc = check_batch(b, BATCH_CSR)) return rc;
  return set_sub(s, repls, repl_lens, count, b, n, -1, -1, d_out_offsets, d_out_data, out_cap, d_nsub, total_bytes, stream);
}
int mrx_set_sub_known_dev(const mrx_set* s, const char* const* repls, const size_t* repl_lens, int64_t count,
                          const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset,
                          int64_t max_text_len, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                          int32_t* d_nsub, int64_t* total_bytes, void* stream) {
  const TextBatch b = csr(d_data, d_offsets);
  if (int rc = check_batch(b, BATCH_CSR)) return rc;
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return set_sub(s, repls, repl_lens, count, b, n, end_offset, max_text_len, d_out_offsets, d_out_data, out_cap, d_nsub,
                 total_bytes, stream);
}
int mrx_set_sub_strided_dev(const mrx_set* s, const char* const* repls, const size_t* repl_lens, int64_t count,
                            const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                            int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int32_t* d_nsub,
                            int64_t* total_bytes, void* stream) {
  return set_sub(s, repls, repl_lens, count, strided(d_data, stride, d_lens, len), n, -1, -1, d_out_offsets, d_out_data,
                 out_cap, d_nsub, total_bytes, stream);
}
int mrx_set_sub_batch(const mrx_set* s, const char* const* repls, const size_t* repl_lens, int64_t count,
                      const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* out_offsets, uint8_t* out_data,
                      int64_t out_cap, int32_t* nsub, int64_t* total_bytes) {
  if (!s || n < 0 || !offsets || !out_offsets || !repl_lens || (out_cap > 0 && !out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (count < 0 || out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "count and out_cap must be >= 0");
  // argument errors and refusals before any device work, as the _dev entry points
  for (size_t j = 0; j < s->members.size(); ++j)
    if (repl_lens[j] > 0 && (!repls || !repls[j]))
      return internal_fail(MRX_E_ARGUMENT, "member " + std::to_string(j) + ": null replacement of nonzero length");
  for (size_t j = 0; j < s->members.size(); ++j)
    if (repl_lens[j] > 0 && repl_has_group_refs(std::string(repls[j], repl_lens[j])))
      return internal_fail(MRX_E_UNSUPPORTED,
                           "member " + std::to_string(j) + ": group references are not supported in a set's sub");
  const std::string refused = set_refusal(s);
  if (!refused.empty()) return internal_fail(MRX_E_UNSUPPORTED, refused);
  DevBatch b; DevBuf<int64_t> oo; DevBuf<uint8_t> od; DevBuf<int32_t> ns;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = oo.alloc((size_t)n + 1)) return rc;
  if (int rc = od.alloc((size_t)out_cap)) return rc;
  if (nsub)
    if (int rc = ns.alloc((size_t)n)) return rc;
  int64_t tot = 0;
  const int rc = mrx_set_sub_known_dev(s, repls, repl_lens, count, b.data, b.offsets, n, b.nbytes, b.longest, oo.p, od.p,
                                       out_cap, ns.p, &tot, nullptr);
  if (total_bytes) *total_bytes = tot;
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  MRX_HIP_TRY(hipMemcpy(out_offsets, oo.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost));
  if (nsub && n > 0) MRX_HIP_TRY(hipMemcpy(nsub, ns.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot > 0) MRX_HIP_TRY(hipMemcpy(out_data, od.p, (size_t)tot, hipMemcpyDeviceToHost));
  return rc;
}

}  // extern "C"
namespace mrx {
std::string set_members_refusal(const mrx_set* s) { return set_refusal(s); }
int set_matches(const mrx_set* s, const TextBatch& b, int64_t n, uint64_t* d_bits, void* stream, int64_t known_total,
                int64_t known_max) {
  return set_run(s, SET_MATCHES, b, n, nullptr, nullptr, d_bits, stream, known_total, known_max);
}
}  // namespace mrx
extern "C" {

void mrx_debug_set_route(int mode) { g_set_route = (mode == 1 || mode == 2) ? mode : 0; }

int mrx_testing_set_run(const mrx_set* s, int op, const uint8_t* text, int len, int32_t* out) {
  if (!s || op < 0 || op > 2 || len < 0 || (!text && len) || !out) return internal_fail(MRX_E_ARGUMENT, "bad argument");
  const int k = (int)s->members.size();
  const int per = op == SET_SEARCH ? 2 : 1;
  for (int x = 0; x < per * k; ++x) out[x] = -2;
  const mrx_set::Plan& pl = s->plan[op == SET_COUNT ? 0 : 1];
  for (const auto& ps : pl.passes) set_pass_run_host(ps, op, text, len, out);
  return MRX_OK;
}

}  // extern "C"
