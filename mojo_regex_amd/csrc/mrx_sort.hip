// Sort and take (include/mrx.h, "sort" and "take"): the stable ascending order of a batch's texts as a permutation with
// their dense ranks, and a new packed batch made of the texts at given indices.
//
// Sort's route is a most-significant-first refinement in steps of 8 bytes.  The state is, for every
// position of the order that is not final yet (an ACTIVE position, kept as a compacted ascending list), the text that
// stands there for now and the GROUP it belongs to: a run of positions whose texts agree on their first d bytes.  A
// round at depth d:
//   k_sort_keys     the big-endian word of bytes [d, d + 8) of every active text, zero padded, and valid = how many of
//                   them exist (mrx_sort_bits.hpp); the round's key is (group, word, valid)
//   k_sort_hist / exclusive_scan / k_sort_scatter
//                   one stable least-significant-digit radix pass of 8 bits each over that key: valid, the word's bytes
//                   that any text can have (the host knows the longest text of most batches), the bytes of the dense
//                   group number that the round's group count needs (none in round 0).  A wavefront owns a tile of
//                   kSortTile elements in both kernels; the counts lie [digit][tile], so their exclusive scan is every
//                   tile's first output slot of every digit.  The scatter walks its tile 64 elements at a time: eight
//                   ballots give a lane the lanes that hold its digit, its rank is their number below it, and the
//                   lowest of them moves the wavefront's own running offset in LDS.  Nothing orders wavefronts against
//                   each other and there is no atomic on memory.
//   k_sort_bounds   a slot starts a new group where its key differs from its predecessor's; exclusive_scan numbers the
//                   groups, k_sort_heads scatters their first slots (the heads give the sizes)
//   k_sort_small    what is final now is written to d_order: a group of one; a group with valid < 8, or at a depth
//                   behind which the host knows that no text goes on (equal texts, in ascending index order because
//                   every pass is stable); and a group of at most 64 members, which a
//                   lane per member finishes by comparing its text from byte d + 8 on with every other member
//                   (sort_compare) and counting those that are smaller, or equal and earlier.  Each such position also
//                   gets its "first of a distinct value" flag.  The members of every other group are flagged to stay.
//   exclusive_scan / k_sort_compact   the next round's active list and dense group numbers
// The host reads one word a round, {active positions, active groups}, and goes on at d + 8 while any is left.  One
// more scan over the distinct-value flags gives d_rank through d_order, and d_totals.
// Every output position is written once, by the one lane that the (deterministic) key order assigns to it.
//
// Take: k_take_lengths validates every index and writes its text's length, exclusive_scan turns the lengths into
// d_out_offsets and the byte count, k_take_totals closes d_totals ({-1, -1} behind an invalid index) and filter's byte
// movers (mrx_filter.hip, filter_gather_kept) move the bytes with d_index as their kept_idx.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <utility>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"
#include "mrx_sort_bits.hpp"

namespace mrx {
namespace {

constexpr int kSortBlock = 256;
constexpr int kSortWaves = kSortBlock / 64;
constexpr int kSortTile = 2048;             // elements of a radix pass that one wavefront counts and scatters
constexpr unsigned kSortMaxGrid = 2048;     // 8 workgroups per CU; the kernels stride over what is left
constexpr int kSortSmallMax = 64;           // a group of at most this many members is finished by comparisons

std::atomic<int> g_sort_small{kSortSmallMax};   // mrx_debug_sort_small()
std::atomic<int> g_sort_grid{0};                // mrx_debug_sort_grid(): workgroups at most (0 = no cap)
thread_local int g_sort_rounds = 0;             // mrx_debug_sort_rounds(): of the calling thread's last sort

// a round's elements, one per active position, in slot order: the key's two words and the text
struct SortKeys {
  uint64_t* word;
  uint64_t* gv;     // group << 8 | valid
  uint32_t* idx;
};

__global__ __launch_bounds__(kSortBlock) void k_sort_keys(const TextBatch B, int64_t m, int64_t d, int first, const SortKeys K) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = first ? j : (int64_t)K.idx[j];
    int32_t L = 0;
    const uint8_t* p = B.text(t, &L);
    int valid;
    K.word[j] = sort_word(p, L, d, &valid);
    K.gv[j] = (first ? 0 : K.gv[j]) | (uint64_t)valid;   // (k_sort_compact left group << 8)
    if (first) K.idx[j] = (uint32_t)j;
  }
}

// Wavefront `wave` of a workgroup takes tile 4 tg + wave of tile group tg; all four run the same number of rounds, so
// the barriers are uniform.  counts[digit * ntiles + tile].
__global__ __launch_bounds__(kSortBlock) void k_sort_hist(const SortKeys K, int64_t m, int pass, int64_t ntiles,
                                                          int64_t* __restrict__ counts) {
  __shared__ unsigned s_cnt[kSortWaves][256];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int64_t tg = blockIdx.x; tg * kSortWaves < ntiles; tg += gridDim.x) {
    const int64_t tile = tg * kSortWaves + wave;
    for (int q = lane; q < 256; q += 64) s_cnt[wave][q] = 0;
    __syncthreads();
    if (tile < ntiles) {
      const int64_t t0 = tile * kSortTile, t1 = t0 + kSortTile < m ? t0 + kSortTile : m;
      for (int64_t j = t0 + lane; j < t1; j += 64) atomicAdd(&s_cnt[wave][sort_digit(K.word[j], K.gv[j], pass)], 1u);
    }
    __syncthreads();
    if (tile < ntiles)
      for (int q = lane; q < 256; q += 64) counts[(int64_t)q * ntiles + tile] = (int64_t)s_cnt[wave][q];
    __syncthreads();
  }
}

// first[digit * ntiles + tile]: the exclusive scan of the counts, the first output slot of that tile's elements with
// that digit.  Elements with one digit keep their order: inside a round of 64 by the lane, between rounds by the
// running offset, between tiles by the scan.
__global__ __launch_bounds__(kSortBlock) void k_sort_scatter(const SortKeys K, const SortKeys O, int64_t m, int pass,
                                                             int64_t ntiles, const int64_t* __restrict__ first) {
  __shared__ unsigned s_off[kSortWaves][256];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int64_t tg = blockIdx.x; tg * kSortWaves < ntiles; tg += gridDim.x) {
    const int64_t tile = tg * kSortWaves + wave;
    if (tile < ntiles)
      for (int q = lane; q < 256; q += 64) s_off[wave][q] = (unsigned)first[(int64_t)q * ntiles + tile];
    __syncthreads();
    const int64_t t0 = tile * kSortTile, t1 = tile < ntiles ? (t0 + kSortTile < m ? t0 + kSortTile : m) : t0;
    const int rounds = kSortTile / 64;   // (the same in every wavefront: the barriers below are uniform)
    for (int r = 0; r < rounds; ++r) {
      const int64_t j = t0 + (int64_t)r * 64 + lane;
      const bool act = j < t1;
      uint64_t word = 0, gv = 0;
      uint32_t idx = 0;
      if (act) {
        word = K.word[j];
        gv = K.gv[j];
        idx = K.idx[j];
      }
      const unsigned dg = act ? sort_digit(word, gv, pass) : 0u;
      unsigned long long same = __ballot(act);
      for (int b = 0; b < 8; ++b) {
        const bool bit = (dg >> b) & 1u;
        const unsigned long long has = __ballot(bit);
        same &= bit ? has : ~has;
      }
      const int below = __popcll(same & ((1ull << lane) - 1ull));
      unsigned at = 0;
      if (act) at = s_off[wave][dg] + (unsigned)below;
      __syncthreads();   // every lane has read its digit's offset
      if (act && below == 0) s_off[wave][dg] += (unsigned)__popcll(same);
      __syncthreads();   // ... and the next round reads the moved ones
      if (act) {
        O.word[at] = word;
        O.gv[at] = gv;
        O.idx[at] = idx;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kSortBlock) void k_sort_bounds(const SortKeys K, int64_t m, int64_t* __restrict__ flags) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x)
    flags[j] = (j == 0 || K.word[j] != K.word[j - 1] || K.gv[j] != K.gv[j - 1]) ? 1 : 0;
}

// before[m + 1]: the exclusive scan of the flags, so a flagged slot's value is its group's number and before[m] the
// number of groups.  head[groups + 1]: the first slot of every group, closed by m.
__global__ __launch_bounds__(kSortBlock) void k_sort_heads(int64_t m, const int64_t* __restrict__ flags,
                                                           const int64_t* __restrict__ before, uint32_t* __restrict__ head) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= m; j += (int64_t)gridDim.x * blockDim.x)
    if (j == m || flags[j]) head[before[j]] = (uint32_t)j;
}

// pos[m]: the output position of every slot (nullptr in round 0: the slot itself).  The positions of a group are
// consecutive, so a member's position is the head's plus its distance from the head.  `state` holds the bounds' flags
// on entry and, on return, what k_sort_compact needs: 1 for a slot that stays active, with bit 32 set at the head of
// its group.
__global__ __launch_bounds__(kSortBlock) void k_sort_small(const TextBatch B, int64_t m, int64_t d, int small_max,
                                                           int last_word, const SortKeys K, const uint32_t* __restrict__ pos,
                                                           const int64_t* __restrict__ before,
                                                           const uint32_t* __restrict__ head, int64_t* state,
                                                           int64_t* __restrict__ order, int64_t* __restrict__ newval) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = before[j] + state[j] - 1;
    const int64_t h = (int64_t)head[g], size = (int64_t)head[g + 1] - h;
    const int64_t p0 = pos ? (int64_t)pos[h] : h;
    const int valid = (int)(K.gv[j] & 0xff);
    const int64_t t = (int64_t)K.idx[j];
    int64_t stay = 0;
    // alone, or one of `size` equal texts that the stable passes left in index order: their last word is this one,
    // because it is not full or because no text of the batch is longer than d + 8 bytes (last_word)
    if (size == 1 || valid < 8 || last_word) {
      order[p0 + (j - h)] = t;
      newval[p0 + (j - h)] = j == h ? 1 : 0;
    } else if (size <= (int64_t)small_max) {
      int32_t L = 0;
      const uint8_t* tp = B.text(t, &L);
      int64_t smaller = 0;
      bool repeated = false;   // an equal member stands earlier
      for (int64_t q = h; q < h + size; ++q) {
        if (q == j) continue;
        int32_t Lq = 0;
        const uint8_t* qp = B.text((int64_t)K.idx[q], &Lq);
        const int c = sort_compare(qp, Lq, tp, L, d + 8);
        if (c < 0 || (c == 0 && q < j)) ++smaller;
        if (c == 0 && q < j) repeated = true;
      }
      order[p0 + smaller] = t;
      newval[p0 + smaller] = repeated ? 0 : 1;
    } else {
      stay = 1 | ((int64_t)(j == h) << 32);
    }
    state[j] = stay;
  }
}

// packed[m + 1]: the exclusive scan of state.  Its low half is a staying slot's new slot, its high half the number of
// staying groups that begin before the slot.
__global__ __launch_bounds__(kSortBlock) void k_sort_compact(int64_t m, const int64_t* __restrict__ state,
                                                             const int64_t* __restrict__ packed, const SortKeys K,
                                                             const uint32_t* __restrict__ pos, const SortKeys O,
                                                             uint32_t* __restrict__ pos_next) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = state[j];
    if (!(s & 1)) continue;
    const int64_t r = packed[j] & 0xffffffffll;
    const int64_t group = (packed[j] >> 32) + (s >> 32) - 1;
    O.idx[r] = K.idx[j];
    O.gv[r] = (uint64_t)group << 8;
    pos_next[r] = pos ? pos[j] : (uint32_t)j;
  }
}

// before[n + 1]: the exclusive scan of newval over the positions
__global__ __launch_bounds__(kSortBlock) void k_sort_rank(int64_t n, const int64_t* __restrict__ order,
                                                          const int64_t* __restrict__ newval,
                                                          const int64_t* __restrict__ before, int64_t* __restrict__ rank) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x)
    rank[order[p]] = before[p] + newval[p] - 1;
}

__global__ __launch_bounds__(kSortBlock) void k_take_lengths(const TextBatch B, int64_t n, const int64_t* __restrict__ index,
                                                             int64_t k, int64_t* __restrict__ klen, int32_t* err) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < k; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = index[j];
    int32_t L = 0;
    if (i < 0 || i >= n)
      *err = 1;
    else
      (void)B.text(i, &L);
    klen[j] = (int64_t)L;
  }
}

// the scan has written the byte count to totals[1]
__global__ void k_take_totals(int64_t k, const int32_t* __restrict__ err, int64_t* __restrict__ totals) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (*err)
      totals[0] = totals[1] = -1;   // an index outside [0, n): no gather, and the caller is told
    else
      totals[0] = k;
  }
}

unsigned sort_grid(int64_t items, int64_t per) {
  return grid_for(items, per, kSortMaxGrid, g_sort_grid.load(std::memory_order_relaxed));
}

// argument errors: nothing has touched the device when one of them returns
int sort_check(const TextBatch& b, BatchForm form, int64_t n, const int64_t* d_order) {
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (n > 0 && !d_order) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n >= ((int64_t)1 << 31)) return internal_fail(MRX_E_ARGUMENT, "n must be below 2^31: a round keeps a text's index in 32 bits");
  return MRX_OK;
}

// known_max: the longest text where the host knows it (< 0: not known)
int sort_run(const TextBatch& b, BatchForm form, int64_t n, int64_t known_max, int64_t* d_order, int64_t* d_rank,
             int64_t* d_totals, void* stream) {
  if (int rc = sort_check(b, form, n, d_order)) return rc;
  hipStream_t hs = (hipStream_t)stream;
  set_last_kernel("k_sort_small");
  g_sort_rounds = 0;
  if (n == 0) {
    if (d_totals) MRX_HIP_TRY(hipMemsetAsync(d_totals, 0, sizeof(int64_t), hs));
    return MRX_OK;
  }
  ScratchScope scope_(stream);
  const size_t words = (size_t)n;
  const int64_t max_tiles = (n + kSortTile - 1) / kSortTile;
  SortKeys cur, oth;
  cur.word = (uint64_t*)scratch_get(sizeof(uint64_t) * words, stream);
  cur.gv = (uint64_t*)scratch_get(sizeof(uint64_t) * words, stream);
  cur.idx = (uint32_t*)scratch_get(sizeof(uint32_t) * words, stream);
  oth.word = (uint64_t*)scratch_get(sizeof(uint64_t) * words, stream);
  oth.gv = (uint64_t*)scratch_get(sizeof(uint64_t) * words, stream);
  oth.idx = (uint32_t*)scratch_get(sizeof(uint32_t) * words, stream);
  uint32_t* pos_a = (uint32_t*)scratch_get(sizeof(uint32_t) * words, stream);
  uint32_t* pos_b = (uint32_t*)scratch_get(sizeof(uint32_t) * words, stream);
  uint32_t* head = (uint32_t*)scratch_get(sizeof(uint32_t) * (words + 1), stream);
  int64_t* state = (int64_t*)scratch_get(sizeof(int64_t) * words, stream);
  int64_t* before = (int64_t*)scratch_get(sizeof(int64_t) * (words + 1), stream);
  int64_t* newval = (int64_t*)scratch_get(sizeof(int64_t) * words, stream);
  int64_t* counts = (int64_t*)scratch_get(sizeof(int64_t) * 256 * (size_t)max_tiles, stream);
  int64_t* first = (int64_t*)scratch_get(sizeof(int64_t) * (256 * (size_t)max_tiles + 1), stream);
  int64_t* d_words = (int64_t*)scratch_get(sizeof(int64_t) * 4, stream);
  if (!cur.word || !cur.gv || !cur.idx || !oth.word || !oth.gv || !oth.idx || !pos_a || !pos_b || !head || !state || !before ||
      !newval || !counts || !first || !d_words)
    return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  const int small_max = g_sort_small.load(std::memory_order_relaxed);
  const dim3 blk(kSortBlock);
  const uint32_t* pos = nullptr;   // round 0: a slot is its position
  uint32_t* pos_next = pos_a;
  int64_t m = n, groups = 1;
  for (int64_t d = 0; m > 0; d += 8) {
    const ScratchMark mark = scratch_mark(stream);   // (the scans' block sums: every round reuses the same bytes)
    const dim3 per_slot(sort_grid(m, kSortBlock));
    const int64_t ntiles = (m + kSortTile - 1) / kSortTile;
    const dim3 per_tile(sort_grid(ntiles, kSortWaves));
    hipLaunchKernelGGL(k_sort_keys, per_slot, blk, 0, hs, b, m, d, d == 0 ? 1 : 0, cur);
    MRX_HIP_TRY(hipGetLastError());
    const int last_pass = 8 + sort_group_passes(groups);
    for (int pass = 0; pass <= last_pass; ++pass) {
      // a digit that is 0 in every key of the round needs no pass: valid and the word's bytes at and behind the
      // longest text's end (pass p of 1..8 holds byte d + 8 - p of a text)
      if (known_max >= 0 && pass <= 8 && d + (pass == 0 ? 0 : 8 - pass) >= known_max) continue;
      hipLaunchKernelGGL(k_sort_hist, per_tile, blk, 0, hs, cur, m, pass, ntiles, counts);
      MRX_HIP_TRY(hipGetLastError());
      if (int rc = exclusive_scan(counts, 256 * ntiles, first, d_words, stream)) return rc;
      hipLaunchKernelGGL(k_sort_scatter, per_tile, blk, 0, hs, cur, oth, m, pass, ntiles, first);
      MRX_HIP_TRY(hipGetLastError());
      std::swap(cur, oth);
    }
    hipLaunchKernelGGL(k_sort_bounds, per_slot, blk, 0, hs, cur, m, state);
    MRX_HIP_TRY(hipGetLastError());
    if (int rc = exclusive_scan(state, m, before, d_words, stream)) return rc;
    hipLaunchKernelGGL(k_sort_heads, dim3(sort_grid(m + 1, kSortBlock)), blk, 0, hs, m, state, before, head);
    MRX_HIP_TRY(hipGetLastError());
    const int last_word = known_max >= 0 && d + 8 >= known_max ? 1 : 0;
    hipLaunchKernelGGL(k_sort_small, per_slot, blk, 0, hs, b, m, d, small_max, last_word, cur, pos, before, head, state, d_order,
                       newval);
    MRX_HIP_TRY(hipGetLastError());
    if (int rc = exclusive_scan(state, m, before, d_words + 1, stream)) return rc;
    hipLaunchKernelGGL(k_sort_compact, per_slot, blk, 0, hs, m, state, before, cur, pos, oth, pos_next);
    MRX_HIP_TRY(hipGetLastError());
    int64_t left = 0;
    MRX_HIP_TRY(hipMemcpyAsync(&left, d_words + 1, sizeof(int64_t), hipMemcpyDeviceToHost, hs));
    MRX_HIP_TRY(hipStreamSynchronize(hs));
    scratch_rewind(stream, mark);
    m = left & 0xffffffffll;
    groups = left >> 32;
    std::swap(cur, oth);
    pos = pos_next;
    pos_next = pos_next == pos_a ? pos_b : pos_a;
    ++g_sort_rounds;
  }
  if (d_rank || d_totals) {
    if (int rc = exclusive_scan(newval, n, before, d_totals ? d_totals : d_words + 2, stream)) return rc;
    if (d_rank) {
      hipLaunchKernelGGL(k_sort_rank, dim3(sort_grid(n, kSortBlock)), blk, 0, hs, n, d_order, newval, before, d_rank);
      MRX_HIP_TRY(hipGetLastError());
    }
  }
  return MRX_OK;
}

struct TakeArgs : PackedDest {   // d_rows: none (the caller's d_index is what a row came from)
  const int64_t* d_index;
  int64_t k;
};

// argument errors: nothing has touched the device when one of them returns
int take_check(const TextBatch& b, BatchForm form, int64_t n, const TakeArgs& a) {
  if (n < 0 || a.k < 0) return internal_fail(MRX_E_ARGUMENT, "n and k must be >= 0");
  if (a.out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "out_cap must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (!a.d_out_offsets || !a.d_totals || (a.k > 0 && !a.d_index) || (a.out_cap > 0 && !a.d_out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  return MRX_OK;
}

int take_run(const TextBatch& b, BatchForm form, int64_t n, int64_t known_max, const TakeArgs& a) {
  if (int rc = take_check(b, form, n, a)) return rc;
  hipStream_t hs = (hipStream_t)a.stream;
  if (a.k == 0) return filter_no_text(b, known_max, a);
  ScratchScope scope_(a.stream);
  int64_t* klen = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)a.k, a.stream);
  int32_t* err = (int32_t*)scratch_get(sizeof(int32_t), a.stream);
  if (!klen || !err) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  MRX_HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), hs));
  hipLaunchKernelGGL(k_take_lengths, dim3(sort_grid(a.k, kSortBlock)), dim3(kSortBlock), 0, hs, b, n, a.d_index, a.k, klen, err);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(klen, a.k, a.d_out_offsets, a.d_totals + 1, a.stream)) return rc;
  hipLaunchKernelGGL(k_take_totals, dim3(1), dim3(64), 0, hs, a.k, err, a.d_totals);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = filter_gather_kept(b, a.k, known_max, a.d_index, a.d_out_offsets, a.d_totals, a.d_out_data, a.out_cap, a.stream))
    return rc;
  return packed_verdict(a, -1, "take: an index is outside [0, n)");
}

int known_check(int64_t end_offset, int64_t max_text_len) {
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return MRX_OK;
}

}  // namespace

// mrx_internal.hpp: the sorted index's build
int sort_order_of(const TextBatch& b, BatchForm form, int64_t n, int64_t known_max, int64_t* d_order, int64_t* d_totals,
                  void* stream) {
  return sort_run(b, form, n, known_max, d_order, nullptr, d_totals, stream);
}
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_sort_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_order, int64_t* d_rank,
                 int64_t* d_totals, void* stream) {
  return sort_run(csr(d_data, d_offsets), BATCH_CSR, n, -1, d_order, d_rank, d_totals, stream);
}
int mrx_sort_known_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset, int64_t max_text_len,
                       int64_t* d_order, int64_t* d_rank, int64_t* d_totals, void* stream) {
  if (int rc = known_check(end_offset, max_text_len)) return rc;
  return sort_run(csr(d_data, d_offsets), BATCH_CSR, n, max_text_len, d_order, d_rank, d_totals, stream);
}
int mrx_sort_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                         int64_t* d_order, int64_t* d_rank, int64_t* d_totals, void* stream) {
  const TextBatch b = strided(d_data, stride, d_lens, len);
  return sort_run(b, BATCH_PITCH, n, b.pitch_longest(), d_order, d_rank, d_totals, stream);
}

int mrx_take_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, const int64_t* d_index, int64_t k,
                 int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals,
                 void* stream) {
  return take_run(csr(d_data, d_offsets), BATCH_CSR, n, -1, TakeArgs{{nullptr, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, d_index, k});
}
int mrx_take_known_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset, int64_t max_text_len,
                       const int64_t* d_index, int64_t k, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                       int64_t* d_totals, int64_t* totals, void* stream) {
  if (int rc = known_check(end_offset, max_text_len)) return rc;
  return take_run(csr(d_data, d_offsets), BATCH_CSR, n, max_text_len,
                  TakeArgs{{nullptr, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, d_index, k});
}
int mrx_take_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                         const int64_t* d_index, int64_t k, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                         int64_t* d_totals, int64_t* totals, void* stream) {
  return take_run(strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1,
                  TakeArgs{{nullptr, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, d_index, k});
}

// host buffers: argument errors before any device work, as the _dev entry points
int mrx_sort_batch(const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* order, int64_t* rank, int64_t* totals) {
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (!offsets || (n > 0 && !order)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n >= ((int64_t)1 << 31)) return internal_fail(MRX_E_ARGUMENT, "n must be below 2^31: a round keeps a text's index in 32 bits");
  DevBatch b; DevBuf<int64_t> od, rk, dt;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = od.alloc((size_t)n)) return rc;
  if (int rc = rk.alloc((size_t)n)) return rc;
  if (int rc = dt.alloc(1)) return rc;
  if (int rc = sort_run(csr(b.data, b.offsets), BATCH_CSR, n, b.longest, od.p, rk.p, dt.p, nullptr)) return rc;
  if (n > 0) MRX_HIP_TRY(hipMemcpy(order, od.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (n > 0 && rank) MRX_HIP_TRY(hipMemcpy(rank, rk.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (totals) MRX_HIP_TRY(hipMemcpy(totals, dt.p, sizeof(int64_t), hipMemcpyDeviceToHost));
  return MRX_OK;
}

int mrx_take_batch(const uint8_t* data, const int64_t* offsets, int64_t n, const int64_t* index, int64_t k,
                   int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals) {
  if (n < 0 || k < 0 || out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "n, k and out_cap must be >= 0");
  if (!offsets || !out_offsets || (k > 0 && !index) || (out_cap > 0 && !out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  DevBatch b; DevBuf<int64_t> ix, oo, dt; DevBuf<uint8_t> od;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = ix.alloc((size_t)k)) return rc;
  if (int rc = oo.alloc((size_t)k + 1)) return rc;
  if (int rc = dt.alloc(2)) return rc;
  if (int rc = od.alloc((size_t)out_cap)) return rc;
  if (k > 0) MRX_HIP_TRY(hipMemcpy(ix.p, index, sizeof(int64_t) * (size_t)k, hipMemcpyHostToDevice));
  int64_t tot[2] = {0, 0};
  const int rc = take_run(csr(b.data, b.offsets), BATCH_CSR, n, b.longest, TakeArgs{{nullptr, oo.p, od.p, out_cap, dt.p, tot, nullptr}, ix.p, k});
  if (totals && (rc == MRX_OK || rc == MRX_E_CAPACITY || tot[0] < 0)) { totals[0] = tot[0]; totals[1] = tot[1]; }
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  MRX_HIP_TRY(hipMemcpy(out_offsets, oo.p, sizeof(int64_t) * (size_t)(k + 1), hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot[1] > 0) MRX_HIP_TRY(hipMemcpy(out_data, od.p, (size_t)tot[1], hipMemcpyDeviceToHost));
  return rc;
}

void mrx_debug_sort_small(int max) { g_sort_small = max < 0 ? kSortSmallMax : max > kSortSmallMax ? kSortSmallMax : max; }
void mrx_debug_sort_grid(int workgroups) { g_sort_grid = workgroups > 0 ? workgroups : 0; }
int mrx_debug_sort_rounds(void) { return g_sort_rounds; }

}  // extern "C"
