// Dictionaries (include/mrx.h, "dictionaries"): an immutable handle built once from a batch of texts, the entries, and
// probed by any number of later batches: d_index[i] = the lowest j with entry j equal to text i, or -1.  Equality is
// distinct's (equal length, equal bytes), and so are the hash, the comparison and the table.
//
// Build, scratch under one ScratchScope, the handle's memory from hipMalloc:
//   k_dict_lengths      klen[j] = length of entry j, idx[j] = j, totals = {m, -}
//   exclusive_scan      the entries' CSR offsets, straight into the handle (total -> totals[1])
//   distinct_groups     distinct's k_distinct_hash, k_distinct_insert and k_distinct_first over the entries
//                       (mrx_distinct.hip: its kernels, its launches), into the handle's table
//   k_dict_fixup        every occupied slot becomes tag << 32 | (lowest index of its group + 1), and the occupied slots
//                       are counted: the number of different entries.  The first synchronisation reads that count,
//                       the insert's error word and the byte count, so that the copy's bytes can be allocated.
//   filter's gather     with kept_idx = 0..m-1: the packed copy of the entries (mrx_filter.hip, filter_gather_kept),
//                       and the second synchronisation: the caller's batch is no longer needed
// The entries that the build's kernels compare are the CALLER's (complete before the call); the copy is read by
// lookups only, and no lookup can start before the build has returned.
//
// Lookup: k_dict_lookup, one launch, hash and probe fused so that the hash never goes to memory.  A wavefront takes 64
// consecutive texts a round, a lane each.  A text of at most kLookupLaneMax bytes is hashed by its lane, a longer one
// by the 16 lanes of its quarter (k_distinct_hash's scheme, the sum kept in registers).  Lanes that hold equal texts
// are thinned to one leader (k_distinct_insert's scheme), and the leader walks the table with plain loads
// (mrx_lookup_bits.hpp, lookup_walk).  No atomics, no LDS, no waiting, no scratch, nothing read back.
//
// Filter: the lookup into d_index (or scratch), k_dict_flags, then filter's own tail (mrx_filter.hip, filter_compact).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"
#include "mrx_lookup_bits.hpp"

// Immutable once mrx_dict_build_* has returned: lookups only read it.
struct mrx_dict {
  int64_t m = 0;          // entries
  int64_t distinct = 0;   // ... of which different
  int64_t bytes = 0;      // of the packed copy
  uint64_t slots = 0;     // words of the table: a power of two >= 2 m (>= 2)
  uint64_t mask = ~0ull;  // mrx_debug_distinct_hash_mask() at build time: what every hash of this table was and-ed with
  unsigned long long* table = nullptr;
  int64_t* offsets = nullptr;   // [m + 1]
  uint8_t* data = nullptr;      // [bytes], 256-byte aligned, with 16 readable bytes behind
  ~mrx_dict() {
    if (table) (void)hipFree(table);
    if (offsets) (void)hipFree(offsets);
    if (data) (void)hipFree(data);
  }
};

namespace mrx {
namespace {

constexpr uint32_t kDictFilterFlags = MRX_FILTER_INVERT | MRX_FILTER_ALL;
constexpr int kLookupBlock = 256;
constexpr int kLookupLanes = 16;     // lanes that share a long text's hash
constexpr int kLookupLaneMax = 64;   // a text of at most this many bytes (four blocks) is hashed by one lane

const char* const kTooMany = "n must be below 2^31: a table slot keeps a text's index in 32 bits";

// what a probe reads of the handle
struct DictView {
  const uint64_t* table;
  uint64_t slots;
  uint64_t mask;
  const uint8_t* data;
  const int64_t* offsets;
};

__global__ __launch_bounds__(kLookupBlock) void k_dict_lengths(const TextBatch B, int64_t m, int64_t* __restrict__ klen,
                                                               int64_t* __restrict__ idx, int64_t* __restrict__ totals) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t L = 0;
    (void)B.text(i, &L);
    klen[i] = (int64_t)L;
    idx[i] = i;
    if (i == 0) totals[0] = m;
  }
}

// Every occupied slot holds a representative's index; first_at[rep] is the lowest index of its group (k_distinct_first).
// An occupied slot per group, so their number is the number of different entries: a ballot per wavefront and round,
// added up in the wavefront's first lane, and one atomic per wavefront at the end (one per round was 3 ms on 2^25 slots:
// half a million adds on the one address).
__global__ __launch_bounds__(kLookupBlock) void k_dict_fixup(unsigned long long* __restrict__ table, uint64_t slots,
                                                             const unsigned long long* __restrict__ first_at,
                                                             unsigned long long* __restrict__ occupied) {
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t rounds = (slots + nthreads - 1) / nthreads;   // (the same in every lane: the ballot is of whole wavefronts)
  unsigned long long seen = 0;
  for (uint64_t r = 0; r < rounds; ++r) {
    const uint64_t s = r * nthreads + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long word = s < slots ? table[s] : 0;
    if (word) table[s] = lookup_slot_word(word, (int64_t)first_at[lookup_slot_index(word)]);
    seen += (unsigned long long)__popcll(__ballot(word != 0));
  }
  if (((int)threadIdx.x & 63) == 0 && seen) atomicAdd(occupied, seen);
}

__global__ __launch_bounds__(kLookupBlock) void k_dict_lookup(const TextBatch B, int64_t n, const DictView D,
                                                              int64_t* __restrict__ index) {
  constexpr int G = kLookupLanes;
  const int lane = (int)threadIdx.x & 63, sub = lane % G, quarter = lane - sub;
  const int64_t nw = (int64_t)gridDim.x * (kLookupBlock / 64);
  const int64_t w = (int64_t)blockIdx.x * (kLookupBlock / 64) + ((int)threadIdx.x >> 6);
  for (int64_t base = w * 64; base < n; base += nw * 64) {   // (base is the same in all lanes of the wavefront)
    const int64_t i = base + lane;
    const bool active = i < n;
    int32_t L = 0;
    const uint8_t* tp = active ? B.text(i, &L) : nullptr;
    const bool wide = L > kLookupLaneMax;
    uint64_t h = 0;
    if (active && !wide) h = distinct_finish(distinct_partial(tp, L, 0, 1), L) & D.mask;
    unsigned long_ones = (unsigned)(__ballot(wide) >> quarter) & 0xffffu;   // the long texts of this lane's quarter
    while (long_ones) {   // (the same in the G lanes of a quarter: they are all here, and leave together)
      const int owner = quarter + (__ffs(long_ones) - 1);
      long_ones &= long_ones - 1;
      int32_t Lj;
      const uint8_t* pj = B.text(base + owner, &Lj);
      uint64_t sum = distinct_partial(pj, Lj, sub, G);
      for (int d = G / 2; d > 0; d >>= 1) sum += (uint64_t)__shfl_xor((unsigned long long)sum, d, G);
      if (lane == owner) h = distinct_finish(sum, Lj) & D.mask;   // (the butterfly leaves the whole sum in every lane)
    }
    // thin out: the lowest lane still to do leads, the lanes with its hash and its bytes follow it
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
    long long found = -1;
    if (active && follow == lane) found = (long long)lookup_walk(D.table, D.slots, h, tp, L, D.data, D.offsets);
    found = __shfl(found, follow);
    if (active) index[i] = (int64_t)found;
  }
}

// the predicate of the dictionary's filter: index[i] >= 0, MRX_FILTER_INVERT negates
__global__ __launch_bounds__(kLookupBlock) void k_dict_flags(const TextBatch B, int64_t n, const int64_t* __restrict__ index,
                                                             uint32_t flags, int64_t* __restrict__ klen,
                                                             int64_t* __restrict__ keep) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const bool kp = (index[i] >= 0) != ((flags & MRX_FILTER_INVERT) != 0);
    int32_t L = 0;
    (void)B.text(i, &L);
    klen[i] = kp ? (int64_t)L : 0;
    keep[i] = kp ? 1 : 0;
  }
}

int dict_build(const TextBatch& b, BatchForm form, int64_t m, void* stream, mrx_dict** out) {
  if (m < 0) return internal_fail(MRX_E_ARGUMENT, "m must be >= 0");
  if (!out) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = check_batch(b, form)) return rc;
  if (m >= ((int64_t)1 << 31)) return internal_fail(MRX_E_ARGUMENT, kTooMany);
  hipStream_t hs = (hipStream_t)stream;
  mrx_dict* d = new mrx_dict();
  struct Guard {   // the handle goes back on every early way out
    mrx_dict* d;
    ~Guard() { delete d; }
  } guard{d};
  d->m = m;
  d->mask = distinct_hash_mask();
  d->slots = 2;
  while (d->slots < 2 * (uint64_t)m) d->slots <<= 1;
  MRX_HIP_TRY(hipMalloc((void**)&d->table, sizeof(uint64_t) * (size_t)d->slots));
  MRX_HIP_TRY(hipMalloc((void**)&d->offsets, sizeof(int64_t) * ((size_t)m + 1)));
  MRX_HIP_TRY(hipMemsetAsync(d->table, 0, sizeof(uint64_t) * (size_t)d->slots, hs));
  if (m == 0) {   // no entry: an empty table answers every probe with -1
    MRX_HIP_TRY(hipMemsetAsync(d->offsets, 0, sizeof(int64_t), hs));
    MRX_HIP_TRY(hipMalloc((void**)&d->data, 16));
    MRX_HIP_TRY(hipStreamSynchronize(hs));
    guard.d = nullptr;
    *out = d;
    return MRX_OK;
  }
  ScratchScope scope_(stream);
  const size_t words = (size_t)m;
  int64_t* klen = (int64_t*)scratch_get(sizeof(int64_t) * words, stream);
  int64_t* idx = (int64_t*)scratch_get(sizeof(int64_t) * words, stream);
  uint64_t* hash = (uint64_t*)scratch_get(sizeof(uint64_t) * words, stream);
  unsigned long long* first_at = (unsigned long long*)scratch_get(sizeof(uint64_t) * words, stream);
  unsigned long long* count_at = (unsigned long long*)scratch_get(sizeof(uint64_t) * words, stream);
  int32_t* rep_of = (int32_t*)scratch_get(sizeof(int32_t) * words, stream);
  // {entries, bytes} for the gather, the occupied slots, the insert's error word
  int64_t* tail = (int64_t*)scratch_get(sizeof(int64_t) * 4, stream);
  if (!klen || !idx || !hash || !first_at || !count_at || !rep_of || !tail)
    return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  int64_t* totals = tail;
  unsigned long long* occupied = (unsigned long long*)(tail + 2);
  int32_t* err = (int32_t*)(tail + 3);
  MRX_HIP_TRY(hipMemsetAsync(tail, 0, sizeof(int64_t) * 4, hs));
  MRX_HIP_TRY(hipMemsetAsync(first_at, 0xFF, sizeof(uint64_t) * words, hs));   // the largest value: atomicMin's start
  MRX_HIP_TRY(hipMemsetAsync(count_at, 0, sizeof(uint64_t) * words, hs));
  const dim3 blk(kLookupBlock);
  hipLaunchKernelGGL(k_dict_lengths, dim3(distinct_grid(m, kLookupBlock)), blk, 0, hs, b, m, klen, idx, totals);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(klen, m, d->offsets, totals + 1, stream)) return rc;
  if (int rc = distinct_groups(b, m, d->mask, DistinctGroups{hash, d->table, d->slots, rep_of, first_at, count_at, err}, stream))
    return rc;
  hipLaunchKernelGGL(k_dict_fixup, dim3(distinct_grid((int64_t)d->slots, kLookupBlock)), blk, 0, hs, d->table, d->slots, first_at,
                     occupied);
  MRX_HIP_TRY(hipGetLastError());
  int64_t got[4] = {0, 0, 0, 0};
  MRX_HIP_TRY(hipMemcpyAsync(got, tail, sizeof(got), hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));   // the first of two: the copy's size
  if ((int32_t)got[3] != 0) return internal_fail(MRX_E_ARGUMENT, "dictionary: a probe of the table ran out");
  d->bytes = got[1];
  d->distinct = got[2];
  // 16 bytes more than the entries: the aligned 16-byte word around the last entry's end is the handle's own, and the
  // allocation's alignment makes the word around the first entry's start begin with it
  MRX_HIP_TRY(hipMalloc((void**)&d->data, (size_t)d->bytes + 16));
  if (int rc = filter_gather_kept(b, m, -1, idx, d->offsets, totals, d->data, d->bytes, stream))
    return rc;
  MRX_HIP_TRY(hipStreamSynchronize(hs));   // the second: the caller's batch may go, and the scratch with this call
  guard.d = nullptr;
  *out = d;
  return MRX_OK;
}

int dict_lookup(const mrx_dict* d, const TextBatch& b, BatchForm form, int64_t n, int64_t* d_index, void* stream) {
  if (!d) return internal_fail(MRX_E_ARGUMENT, "null dictionary");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (n > 0 && !d_index) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n == 0) return MRX_OK;
  const DictView view{(const uint64_t*)d->table, d->slots, d->mask, d->data, d->offsets};
  hipLaunchKernelGGL(k_dict_lookup, dim3(distinct_grid(n, kLookupBlock)), dim3(kLookupBlock), 0, (hipStream_t)stream, b, n, view,
                     d_index);
  MRX_HIP_TRY(hipGetLastError());
  set_last_kernel("k_dict_lookup");
  return MRX_OK;
}

struct DictFilterArgs {
  uint32_t flags;
  int64_t* d_index;
  PackedDest dest;
};

int dict_filter(const mrx_dict* d, const TextBatch& b, BatchForm form, int64_t n, int64_t known_max, const DictFilterArgs& a) {
  const PackedDest& o = a.dest;
  if (!d) return internal_fail(MRX_E_ARGUMENT, "null dictionary");
  if (a.flags & ~kDictFilterFlags) return internal_fail(MRX_E_ARGUMENT, "unknown flag bits");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (o.out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "out_cap must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (!o.d_out_offsets || !o.d_totals || (n > 0 && !o.d_rows) || (o.out_cap > 0 && !o.d_out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n == 0) return filter_no_text(b, known_max, o);
  ScratchScope scope_(o.stream);
  int64_t* klen = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, o.stream);
  int64_t* keep = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, o.stream);
  int64_t* pos = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(n + 1), o.stream);
  int64_t* rank = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(n + 1), o.stream);
  int64_t* index = a.d_index ? a.d_index : (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, o.stream);
  if (!klen || !keep || !pos || !rank || !index) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  if (int rc = dict_lookup(d, b, form, n, index, o.stream)) return rc;
  hipLaunchKernelGGL(k_dict_flags, dim3(distinct_grid(n, kLookupBlock)), dim3(kLookupBlock), 0, (hipStream_t)o.stream, b, n, index,
                     a.flags, klen, keep);
  MRX_HIP_TRY(hipGetLastError());
  return filter_compact(b, n, known_max, FilterWork{klen, keep, pos, rank}, o);
}

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_dict_build_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t m, void* stream, mrx_dict** out) {
  return dict_build(csr(d_data, d_offsets), BATCH_CSR, m, stream, out);
}
int mrx_dict_build_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t m,
                               void* stream, mrx_dict** out) {
  return dict_build(strided(d_data, stride, d_lens, len), BATCH_PITCH, m, stream, out);
}
void mrx_dict_free(mrx_dict* d) { delete d; }
int64_t mrx_dict_size(const mrx_dict* d) { return d ? d->m : 0; }
int64_t mrx_dict_distinct(const mrx_dict* d) { return d ? d->distinct : 0; }

int mrx_dict_lookup_dev(const mrx_dict* d, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_index,
                        void* stream) {
  return dict_lookup(d, csr(d_data, d_offsets), BATCH_CSR, n, d_index, stream);
}
int mrx_dict_lookup_strided_dev(const mrx_dict* d, const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len,
                                int64_t n, int64_t* d_index, void* stream) {
  return dict_lookup(d, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, d_index, stream);
}

int mrx_dict_filter_dev(const mrx_dict* d, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        int64_t* d_index, int64_t* d_kept_idx, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                        int64_t* d_totals, int64_t* totals, void* stream) {
  return dict_filter(d, csr(d_data, d_offsets), BATCH_CSR, n, -1,
                     DictFilterArgs{flags, d_index, {d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}});
}
int mrx_dict_filter_known_dev(const mrx_dict* d, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                              int64_t end_offset, int64_t max_text_len, int64_t* d_index, int64_t* d_kept_idx,
                              int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals,
                              void* stream) {
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return dict_filter(d, csr(d_data, d_offsets), BATCH_CSR, n, max_text_len,
                     DictFilterArgs{flags, d_index, {d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}});
}
int mrx_dict_filter_strided_dev(const mrx_dict* d, uint32_t flags, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                                int32_t len, int64_t n, int64_t* d_index, int64_t* d_kept_idx, int64_t* d_out_offsets,
                                uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  return dict_filter(d, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1,
                     DictFilterArgs{flags, d_index, {d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}});
}

// host buffers: argument errors before any device work, as the _dev entry points
int mrx_dict_lookup_batch(const uint8_t* dict_data, const int64_t* dict_offsets, int64_t m, const uint8_t* data,
                          const int64_t* offsets, int64_t n, int64_t* index) {
  if (m < 0 || n < 0) return internal_fail(MRX_E_ARGUMENT, "m and n must be >= 0");
  if (!dict_offsets || !offsets || (n > 0 && !index)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (m >= ((int64_t)1 << 31)) return internal_fail(MRX_E_ARGUMENT, kTooMany);
  DevBatch e, b;
  DevBuf<int64_t> ix;
  if (int rc = e.measure(dict_offsets, m)) return rc;
  if (int rc = b.measure(offsets, n)) return rc;
  if (e.nbytes < 0 || b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if ((e.nbytes > 0 && !dict_data) || (b.nbytes > 0 && !data)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = e.upload(dict_data, dict_offsets, m)) return rc;
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = ix.alloc((size_t)n)) return rc;
  mrx_dict* d = nullptr;
  if (int rc = dict_build(csr(e.data, e.offsets), BATCH_CSR, m, nullptr, &d)) return rc;
  int rc = dict_lookup(d, csr(b.data, b.offsets), BATCH_CSR, n, ix.p, nullptr);
  if (rc == MRX_OK && n > 0 && hipMemcpy(index, ix.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
    rc = internal_fail(MRX_E_NO_DEVICE, "copying the indices to the host failed");
  delete d;   // (behind the copy, which waited for the lookup)
  return rc;
}

}  // extern "C"
