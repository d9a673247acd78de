// Distinct (include/mrx.h, "distinct"): the unique texts of a batch, numbered by first occurrence, with their counts, the
// group of every text and the values as a new packed CSR batch on the device.  Nothing is sorted.
//
// Route, all scratch under one ScratchScope:
//   k_distinct_hash     64-bit hash of every text (mrx_distinct_bits.hpp): a lane per text of at most kDistinctLaneMax
//                       bytes, 16 lanes for a longer one (the hash is a sum over 16-byte blocks, so the lanes stripe
//                       the blocks and add their parts with four shuffles)
//   k_distinct_insert   open-addressing table of 64-bit slots, a power of two >= 2 n, zeroed by hipMemsetAsync.  A
//                       slot is (high 32 hash bits << 32) | (representative's index + 1), written once by atomicCAS
//                       and never again.  A text walks from its home slot: an empty slot it tries to take (the CAS's
//                       return value is the truth: on failure it holds the winner's word), a slot with its own tag it
//                       compares bytewise with -- that text's bytes are INPUT, complete before the call -- and equal
//                       ends the walk.  No lane ever waits for another lane's store; no spin, no fence, no flag.
//                       Lanes of a wavefront that hold the same text are thinned out first: one of them walks.
//                       Equal texts walk the same slots and slots are write-once, so they all end at the one slot that
//                       the first of them to arrive took: one representative per group, whichever it is.
//   k_distinct_first    atomicMin(first_at[rep], i), atomicAdd(count_at[rep], 1); lanes of a wavefront that share a
//                       representative are combined first, then the wavefronts of a workgroup in LDS (one pair of
//                       atomics per 4096 equal texts)
//   k_distinct_flags    keep[i] = (first_at[rep_of[i]] == i), klen[i] = the kept length
//   exclusive_scan      twice, as filter: ranks (total -> d_totals[0]) and byte positions (total -> d_totals[1])
//   k_distinct_finish   group_of[i] = rank[first_at[rep_of[i]]]; for kept i first[rank], counts[rank], out_offsets[rank]
//   filter's gather     with kept_idx = first (mrx_filter.hip, filter_gather_kept: its kernels, its route rule)
// Which text represents a group depends on the race; first_at (a minimum) and count_at (a sum of ones) do not, and
// every output is a function of those two and of the input.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_distinct_bits.hpp"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"

namespace mrx {
namespace {

constexpr int kDistinctBlock = 256;
constexpr unsigned kDistinctMaxGrid = 2048;   // 8 workgroups per CU; the kernels stride over what is left
constexpr int kDistinctLanes = 16;            // lanes that share a long text in k_distinct_hash
constexpr int kDistinctLaneMax = 64;          // a text of at most this many bytes (four blocks) is hashed by one lane

std::atomic<uint64_t> g_distinct_mask{~0ull};   // mrx_debug_distinct_hash_mask()
std::atomic<int> g_distinct_grid{0};            // mrx_debug_distinct_grid(): workgroups at most (0 = no cap)

// A wavefront takes 64 consecutive texts a round, a lane each.  A text of at most kDistinctLaneMax bytes is hashed by
// its lane alone.  The longer ones are then taken one after the other by the 16 lanes of their quarter of the
// wavefront: the lanes stripe the text's blocks and add their parts with four shuffles (the hash is a sum over the
// blocks).  One kernel for every shape: pieces of ten bytes keep all lanes busy, and no long text is left to one lane.
__global__ __launch_bounds__(kDistinctBlock) void k_distinct_hash(const TextBatch B, int64_t n, uint64_t mask,
                                                                  uint64_t* __restrict__ hash) {
  constexpr int G = kDistinctLanes;
  const int lane = (int)threadIdx.x & 63, sub = lane % G, quarter = lane - sub;
  const int64_t nw = (int64_t)gridDim.x * (kDistinctBlock / 64);
  const int64_t w = (int64_t)blockIdx.x * (kDistinctBlock / 64) + ((int)threadIdx.x >> 6);
  for (int64_t base = w * 64; base < n; base += nw * 64) {   // (base is the same in all lanes of the wavefront)
    const int64_t i = base + lane;
    int32_t L = 0;
    const uint8_t* tp = i < n ? B.text(i, &L) : nullptr;
    const bool wide = L > kDistinctLaneMax;
    if (i < n && !wide) hash[i] = distinct_finish(distinct_partial(tp, L, 0, 1), L) & mask;
    unsigned todo = (unsigned)(__ballot(wide) >> quarter) & 0xffffu;   // the long texts of this lane's quarter
    while (todo) {   // (the same in the G lanes of a quarter: they are all here, and leave together)
      const int64_t j = base + quarter + (__ffs(todo) - 1);
      todo &= todo - 1;
      int32_t Lj;
      const uint8_t* pj = B.text(j, &Lj);
      uint64_t sum = distinct_partial(pj, Lj, sub, G);
      for (int d = G / 2; d > 0; d >>= 1) sum += (uint64_t)__shfl_xor((unsigned long long)sum, d, G);
      if (sub == 0) hash[j] = distinct_finish(sum, Lj) & mask;
    }
  }
}

// A wavefront takes 64 consecutive texts a round.  Real inputs are skewed, and a slot that thousands of lanes read at
// once is served one lane at a time, so the lanes of a wavefront are thinned out first: the lowest lane still to do
// leads, the lanes with its hash compare their bytes with ITS text (input, like a representative's: nobody waits for
// anybody) and, where equal, follow it.  Only the leaders walk the table; a follower takes its leader's answer.
__global__ __launch_bounds__(kDistinctBlock) void k_distinct_insert(const TextBatch B, int64_t n,
                                                                    const uint64_t* __restrict__ hash,
                                                                    unsigned long long* table, uint64_t slots,
                                                                    int32_t* __restrict__ rep_of, int32_t* err) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (kDistinctBlock / 64);
  const int64_t w = (int64_t)blockIdx.x * (kDistinctBlock / 64) + ((int)threadIdx.x >> 6);
  for (int64_t base = w * 64; base < n; base += nw * 64) {   // (base is the same in all lanes of the wavefront)
    const int64_t i = base + lane;
    const bool active = i < n;
    const uint64_t h = active ? hash[i] : 0;
    int32_t L = 0;
    const uint8_t* tp = active ? B.text(i, &L) : nullptr;
    int follow = lane;
    bool todo = active;
    while (true) {
      const unsigned long long left = __ballot(todo);
      if (left == 0) break;
      const int leader = __ffsll((long long)left) - 1;
      const uint64_t hl = (uint64_t)__shfl((unsigned long long)h, leader);
      if (lane == leader) {
        todo = false;
      } else if (todo && h == hl) {
        int32_t Ll;
        const uint8_t* lp = B.text(base + leader, &Ll);
        if (Ll == L && distinct_equal(tp, lp, L)) {
          follow = leader;
          todo = false;
        }
      }
    }
    int32_t rep = -1;
    if (active && follow == lane) {
      const uint64_t tag = h >> 32;
      const unsigned long long mine = (tag << 32) | (uint64_t)(i + 1);
      for (uint64_t probe = 0; probe < slots; ++probe) {
        unsigned long long* slot = table + ((h + probe) & (slots - 1));
        unsigned long long cur = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
          cur = atomicCAS(slot, 0ull, mine);
          if (cur == 0) {   // taken: this text stands for its group
            rep = (int32_t)i;
            break;
          }
        }
        if ((cur >> 32) != tag) continue;
        const int64_t r = (int64_t)(cur & 0xffffffffull) - 1;
        int32_t Lr;
        const uint8_t* rp = B.text(r, &Lr);
        if (Lr == L && distinct_equal(tp, rp, L)) {
          rep = (int32_t)r;
          break;
        }
      }
      if (rep < 0) {   // (a table at load <= 1/2 always has an empty slot: unreachable)
        *err = 1;
        rep = (int32_t)i;
      }
    }
    rep = __shfl(rep, follow);
    if (active) rep_of[i] = rep;
  }
}

// atomicMin(first_at[rep], i) and atomicAdd(count_at[rep], 1) for every text, with as few atomics on one address as
// the skew of real inputs asks for (a hot address takes them one at a time).  A workgroup takes kDistinctChunk
// consecutive texts at a time.  In each wavefront the lanes that share a representative are combined by ballots: the
// lowest of them leads, its index is their minimum and the ballot's population their count.  The leaders add to a
// direct-mapped table in LDS (kDistinctSlots entries: representative, lowest index, count; an index fits 32 bits),
// or, where another representative holds the entry, to memory.  The table is flushed with one pair of atomics per
// entry: 2^24 equal texts cost 4096 pairs on the one address, not 2^24.
constexpr int kDistinctChunk = 4096;
constexpr int kDistinctSlots = 1024;
__global__ __launch_bounds__(kDistinctBlock) void k_distinct_first(int64_t n, const int32_t* __restrict__ rep_of,
                                                                   unsigned long long* first_at,
                                                                   unsigned long long* count_at) {
  __shared__ unsigned s_tag[kDistinctSlots];   // representative + 1; 0 = free
  __shared__ unsigned s_low[kDistinctSlots];
  __shared__ unsigned s_cnt[kDistinctSlots];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int64_t c0 = (int64_t)blockIdx.x * kDistinctChunk; c0 < n; c0 += (int64_t)gridDim.x * kDistinctChunk) {
    for (int q = (int)threadIdx.x; q < kDistinctSlots; q += kDistinctBlock) {
      s_tag[q] = 0;
      s_low[q] = 0xffffffffu;
      s_cnt[q] = 0;
    }
    __syncthreads();
    const int64_t c1 = c0 + kDistinctChunk < n ? c0 + kDistinctChunk : n;
    for (int64_t base = c0 + wave * 64; base < c1; base += kDistinctBlock) {   // (the same in all lanes of a wavefront)
      const int64_t i = base + lane;
      const int32_t r = i < c1 ? rep_of[i] : -1;
      bool todo = i < c1, lead = false;
      unsigned group = 0;
      while (true) {
        const unsigned long long left = __ballot(todo);
        if (left == 0) break;
        const int leader = __ffsll((long long)left) - 1;
        const int32_t lr = __shfl(r, leader);
        const unsigned long long same = __ballot(todo && r == lr);
        if (lane == leader) {
          lead = true;
          group = (unsigned)__popcll(same);
        }
        todo = todo && r != lr;
      }
      if (lead) {
        const unsigned q = (unsigned)r & (kDistinctSlots - 1), t = (unsigned)r + 1;
        const unsigned prev = atomicCAS(&s_tag[q], 0u, t);
        if (prev == 0 || prev == t) {
          atomicMin(&s_low[q], (unsigned)i);
          atomicAdd(&s_cnt[q], group);
        } else {
          atomicMin(first_at + r, (unsigned long long)i);
          atomicAdd(count_at + r, (unsigned long long)group);
        }
      }
    }
    __syncthreads();
    for (int q = (int)threadIdx.x; q < kDistinctSlots; q += kDistinctBlock) {
      if (s_tag[q]) {
        atomicMin(first_at + (s_tag[q] - 1), (unsigned long long)s_low[q]);
        atomicAdd(count_at + (s_tag[q] - 1), (unsigned long long)s_cnt[q]);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kDistinctBlock) void k_distinct_flags(const TextBatch B, int64_t n,
                                                                   const int32_t* __restrict__ rep_of,
                                                                   const unsigned long long* __restrict__ first_at,
                                                                   int64_t* __restrict__ klen, int64_t* __restrict__ keep) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const bool kp = (int64_t)first_at[rep_of[i]] == i;
    int32_t L = 0;
    (void)B.text(i, &L);
    klen[i] = kp ? (int64_t)L : 0;
    keep[i] = kp ? 1 : 0;
  }
}

// rank[n + 1], pos[n + 1]: the exclusive scans of keep and klen.  Entry n closes the values' CSR.
struct DistinctOut {
  int64_t* group_of;
  int64_t* first;
  int64_t* counts;
  int64_t* out_off;
  int64_t* totals;
};
__global__ __launch_bounds__(kDistinctBlock) void k_distinct_finish(int64_t n, const int32_t* __restrict__ rep_of,
                                                                    const unsigned long long* __restrict__ first_at,
                                                                    const unsigned long long* __restrict__ count_at,
                                                                    const int64_t* __restrict__ rank,
                                                                    const int64_t* __restrict__ pos,
                                                                    const int32_t* __restrict__ err, const DistinctOut O) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i == n) {
      O.out_off[rank[n]] = pos[n];
      if (*err) O.totals[0] = O.totals[1] = -1;   // the probe ran out: no gather, and the caller is told
      continue;
    }
    const int32_t rep = rep_of[i];
    const int64_t f = (int64_t)first_at[rep];
    const int64_t g = rank[f];
    O.group_of[i] = g;
    if (f == i) {
      O.first[g] = i;
      O.counts[g] = (int64_t)count_at[rep];
      O.out_off[g] = pos[i];
    }
  }
}

}  // namespace

// ---- shared with dictionaries (mrx_lookup.hip) through mrx_internal.hpp --------------------------------------------
uint64_t distinct_hash_mask() { return g_distinct_mask.load(std::memory_order_relaxed); }

unsigned distinct_grid(int64_t items, int64_t per) {
  return grid_for(items, per, kDistinctMaxGrid, g_distinct_grid.load(std::memory_order_relaxed));
}

int distinct_groups(const TextBatch& b, int64_t n, uint64_t mask, const DistinctGroups& g, void* stream) {
  hipStream_t hs = (hipStream_t)stream;
  const dim3 blk(kDistinctBlock);
  const dim3 per_text(distinct_grid(n, kDistinctBlock));
  hipLaunchKernelGGL(k_distinct_hash, per_text, blk, 0, hs, b, n, mask, g.hash);
  MRX_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_distinct_insert, per_text, blk, 0, hs, b, n, g.hash, g.table, g.slots, g.rep_of, g.err);
  MRX_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_distinct_first, dim3(distinct_grid(n, kDistinctChunk)), blk, 0, hs, n, g.rep_of, g.first_at, g.count_at);
  MRX_HIP_TRY(hipGetLastError());
  return MRX_OK;
}

namespace {

struct DistinctArgs : PackedDest {   // d_rows: d_first
  int64_t* d_group_of;
  int64_t* d_counts;
};

// argument errors: nothing has touched the device when one of them returns
int distinct_check(const TextBatch& b, BatchForm form, int64_t n, const DistinctArgs& a) {
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (a.out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "out_cap must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (!a.d_out_offsets || !a.d_totals || (n > 0 && (!a.d_group_of || !a.d_rows || !a.d_counts)) ||
      (a.out_cap > 0 && !a.d_out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n >= ((int64_t)1 << 31)) return internal_fail(MRX_E_ARGUMENT, "n must be below 2^31: a table slot keeps a text's index in 32 bits");
  return MRX_OK;
}

int distinct_run(const TextBatch& b, BatchForm form, int64_t n, int64_t known_max, const DistinctArgs& a) {
  if (int rc = distinct_check(b, form, n, a)) return rc;
  hipStream_t hs = (hipStream_t)a.stream;
  if (n == 0) return packed_empty(a);
  ScratchScope scope_(a.stream);
  uint64_t slots = 2;
  while (slots < 2 * (uint64_t)n) slots <<= 1;
  const size_t words = (size_t)n;
  uint64_t* hash = (uint64_t*)scratch_get(sizeof(uint64_t) * words, a.stream);
  unsigned long long* table = (unsigned long long*)scratch_get(sizeof(uint64_t) * (size_t)slots, a.stream);
  unsigned long long* first_at = (unsigned long long*)scratch_get(sizeof(uint64_t) * words, a.stream);
  unsigned long long* count_at = (unsigned long long*)scratch_get(sizeof(uint64_t) * words, a.stream);
  int64_t* klen = (int64_t*)scratch_get(sizeof(int64_t) * words, a.stream);
  int64_t* keep = (int64_t*)scratch_get(sizeof(int64_t) * words, a.stream);
  int64_t* pos = (int64_t*)scratch_get(sizeof(int64_t) * (words + 1), a.stream);
  int64_t* rank = (int64_t*)scratch_get(sizeof(int64_t) * (words + 1), a.stream);
  int32_t* rep_of = (int32_t*)scratch_get(sizeof(int32_t) * words, a.stream);
  int32_t* err = (int32_t*)scratch_get(sizeof(int32_t), a.stream);
  if (!hash || !table || !first_at || !count_at || !klen || !keep || !pos || !rank || !rep_of || !err)
    return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  MRX_HIP_TRY(hipMemsetAsync(table, 0, sizeof(uint64_t) * (size_t)slots, hs));
  MRX_HIP_TRY(hipMemsetAsync(first_at, 0xFF, sizeof(uint64_t) * words, hs));   // the largest value: atomicMin's start
  MRX_HIP_TRY(hipMemsetAsync(count_at, 0, sizeof(uint64_t) * words, hs));
  MRX_HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), hs));
  const dim3 blk(kDistinctBlock);
  const dim3 per_text(distinct_grid(n, kDistinctBlock));
  if (int rc = distinct_groups(b, n, distinct_hash_mask(), DistinctGroups{hash, table, slots, rep_of, first_at, count_at, err}, a.stream))
    return rc;
  hipLaunchKernelGGL(k_distinct_flags, per_text, blk, 0, hs, b, n, rep_of, first_at, klen, keep);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(klen, n, pos, a.d_totals + 1, a.stream)) return rc;
  if (int rc = exclusive_scan(keep, n, rank, a.d_totals, a.stream)) return rc;
  hipLaunchKernelGGL(k_distinct_finish, dim3(distinct_grid(n + 1, kDistinctBlock)), blk, 0, hs, n, rep_of, first_at, count_at, rank,
                     pos, err, DistinctOut{a.d_group_of, a.d_rows, a.d_counts, a.d_out_offsets, a.d_totals});
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = filter_gather_kept(b, n, known_max, a.d_rows, a.d_out_offsets, a.d_totals, a.d_out_data, a.out_cap, a.stream))
    return rc;
  return packed_verdict(a, -1, "distinct: a probe of the table ran out");
}

int distinct_known(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset, int64_t max_text_len,
                   const DistinctArgs& a) {
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return distinct_run(csr(d_data, d_offsets), BATCH_CSR, n, max_text_len, a);
}

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_distinct_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_group_of, int64_t* d_first,
                     int64_t* d_counts, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                     int64_t* totals, void* stream) {
  return distinct_run(csr(d_data, d_offsets), BATCH_CSR, n, -1,
                      DistinctArgs{{d_first, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, d_group_of, d_counts});
}
int mrx_distinct_known_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset,
                           int64_t max_text_len, int64_t* d_group_of, int64_t* d_first, int64_t* d_counts,
                           int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                           int64_t* totals, void* stream) {
  return distinct_known(d_data, d_offsets, n, end_offset, max_text_len,
                        DistinctArgs{{d_first, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, d_group_of, d_counts});
}
int mrx_distinct_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                             int64_t* d_group_of, int64_t* d_first, int64_t* d_counts, int64_t* d_out_offsets,
                             uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  return distinct_run(strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1,
                      DistinctArgs{{d_first, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, d_group_of, d_counts});
}

// host buffers: argument errors before any device work, as the _dev entry points
int mrx_distinct_batch(const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* group_of, int64_t* first,
                       int64_t* counts, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals) {
  if (n < 0 || out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "n and out_cap must be >= 0");
  if (!offsets || !out_offsets || (n > 0 && (!group_of || !first || !counts)) || (out_cap > 0 && !out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n >= ((int64_t)1 << 31)) return internal_fail(MRX_E_ARGUMENT, "n must be below 2^31: a table slot keeps a text's index in 32 bits");
  DevBatch b; DevBuf<int64_t> go, fi, co, oo, dt; DevBuf<uint8_t> od;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = go.alloc((size_t)n)) return rc;
  if (int rc = fi.alloc((size_t)n)) return rc;
  if (int rc = co.alloc((size_t)n)) return rc;
  if (int rc = oo.alloc((size_t)n + 1)) return rc;
  if (int rc = dt.alloc(2)) return rc;
  if (int rc = od.alloc((size_t)out_cap)) return rc;
  int64_t tot[2] = {0, 0};
  const int rc = distinct_known(b.data, b.offsets, n, b.nbytes, b.longest,
                                DistinctArgs{{fi.p, oo.p, od.p, out_cap, dt.p, tot, nullptr}, go.p, co.p});
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  if (totals) { totals[0] = tot[0]; totals[1] = tot[1]; }
  if (n > 0) MRX_HIP_TRY(hipMemcpy(group_of, go.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (tot[0] > 0) {
    MRX_HIP_TRY(hipMemcpy(first, fi.p, sizeof(int64_t) * (size_t)tot[0], hipMemcpyDeviceToHost));
    MRX_HIP_TRY(hipMemcpy(counts, co.p, sizeof(int64_t) * (size_t)tot[0], hipMemcpyDeviceToHost));
  }
  MRX_HIP_TRY(hipMemcpy(out_offsets, oo.p, sizeof(int64_t) * (size_t)(tot[0] + 1), hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot[1] > 0) MRX_HIP_TRY(hipMemcpy(out_data, od.p, (size_t)tot[1], hipMemcpyDeviceToHost));
  return rc;
}

void mrx_debug_distinct_hash_mask(uint64_t mask) { g_distinct_mask = mask; }
void mrx_debug_distinct_grid(int workgroups) { g_distinct_grid = workgroups > 0 ? workgroups : 0; }

}  // extern "C"
