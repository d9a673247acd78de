// Sorted index (include/mrx.h, "sorted index"): an immutable handle over a batch of texts, the entries, in sort's order,
// probed by any number of later batches: bisect_left / bisect_right, the range of entries that begin with a text, and the
// longest entry that is a prefix of a text.  The judgements are in mrx_sorted_bits.hpp.
//
// Build, scratch under one ScratchScope, the handle's memory from hipMalloc:
//   sort_order_of       sort's own rounds (mrx_sort.hip) into the handle's `order`, and the number of different entries
//   k_sorted_lengths    klen[p] = length of entry order[p]
//   exclusive_scan      the sorted entries' CSR offsets, straight into the handle (total -> the byte count).  The first
//                       synchronisation behind sort's reads that count and the distinct count, so that the copy's bytes
//                       can be allocated.
//   filter's gather     with kept_idx = order: the packed copy of the entries in sorted order (filter_gather_kept)
//   k_sorted_keys       the search aids: sort_word(entry, 0) and its valid count for every position, and every fstep-th
//                       of them once more as the fence posts; then the last synchronisation: the caller's batch may go
//
// Search: k_sorted_search, one launch, a lane per probe, grid-stride.  The lane runs mrx_sorted_bits.hpp's binary search
// with the depth it has proven against both bounds.  With the key aid the first words are searched with 8-byte loads and
// only the run of entries with the probe's first 8 bytes goes to the bytes; with the fence aid every workgroup first
// copies the posts to LDS, and the top steps of a key search touch no global memory.  No atomics, no scratch, nothing
// read back.  A text of many KiB is compared by its one lane: correct, not fast.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"
#include "mrx_sorted_bits.hpp"

// Immutable once mrx_sorted_build_* has returned: searches only read it.
struct mrx_sorted {
  int64_t m = 0;          // entries
  int64_t distinct = 0;   // ... of which different
  int64_t bytes = 0;      // of the packed copy
  int64_t fstep = 1;      // positions between two fence posts
  int fcount = 0;         // fence posts
  int64_t* order = nullptr;     // [m]: the original index of the entry at every position
  int64_t* offsets = nullptr;   // [m + 1]
  uint8_t* data = nullptr;      // [bytes], 256-byte aligned, with 16 readable bytes behind
  uint64_t* keys = nullptr;     // [m]
  uint8_t* valids = nullptr;    // [m]
  uint64_t* fkey = nullptr;     // [kSortedFence]
  uint8_t* fvalid = nullptr;    // [kSortedFence]
  ~mrx_sorted() {
    for (void* p : {(void*)order, (void*)offsets, (void*)data, (void*)keys, (void*)valids, (void*)fkey, (void*)fvalid})
      if (p) (void)hipFree(p);
  }
};

namespace mrx {
namespace {

constexpr int kSortedBlock = 256;
constexpr unsigned kSortedMaxGrid = 2048;   // 8 workgroups per CU; the kernels stride over what is left
constexpr int kSortedAidsDefault = SORTED_AID_KEYS | SORTED_AID_FENCE;

std::atomic<int> g_sorted_grid{0};                      // mrx_debug_sorted_grid(): workgroups at most (0 = no cap)
std::atomic<int> g_sorted_aids{kSortedAidsDefault};     // mrx_debug_sorted_aids()

const char* const kTooMany = "m must be below 2^31: sort keeps a text's index in 32 bits";

unsigned sorted_grid(int64_t items) {
  return grid_for(items, kSortedBlock, kSortedMaxGrid, g_sorted_grid.load(std::memory_order_relaxed));
}

__global__ __launch_bounds__(kSortedBlock) void k_sorted_lengths(const TextBatch B, int64_t m, const int64_t* __restrict__ order,
                                                                 int64_t* __restrict__ klen, int64_t* __restrict__ totals) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
    int32_t L = 0;
    (void)B.text(order[p], &L);
    klen[p] = (int64_t)L;
    if (p == 0) totals[0] = m;
  }
}

__global__ __launch_bounds__(kSortedBlock) void k_sorted_keys(const SortedView V, uint64_t* __restrict__ keys,
                                                              uint8_t* __restrict__ valids, uint64_t* __restrict__ fkey,
                                                              uint8_t* __restrict__ fvalid) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < V.m; p += (int64_t)gridDim.x * blockDim.x) {
    int64_t L;
    const uint8_t* e = sorted_entry(V, p, &L);
    int valid;
    const uint64_t w = sort_word(e, L, 0, &valid);
    keys[p] = w;
    valids[p] = (uint8_t)valid;
    if (p % V.fstep == 0) {   // post p / fstep < fcount = ceil(m / fstep)
      fkey[p / V.fstep] = w;
      fvalid[p / V.fstep] = (uint8_t)valid;
    }
  }
}

__global__ __launch_bounds__(kSortedBlock) void k_sorted_search(SortedView V, const TextBatch B, int64_t n, uint32_t mode,
                                                                int64_t* __restrict__ lo, int64_t* __restrict__ hi) {
  __shared__ uint64_t s_fkey[kSortedFence];
  __shared__ uint8_t s_fvalid[kSortedFence];
  if (V.fcount > 0) {   // (the same in every lane: the barrier is uniform)
    for (int q = (int)threadIdx.x; q < V.fcount; q += kSortedBlock) {
      s_fkey[q] = V.fkey[q];
      s_fvalid[q] = V.fvalid[q];
    }
    __syncthreads();
    V.fkey = s_fkey;
    V.fvalid = s_fvalid;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t L = 0;
    const uint8_t* p = B.text(i, &L);
    int64_t a, b;
    sorted_search_one(V, mode, p, (int64_t)L, &a, &b);
    if (lo) lo[i] = a;
    if (hi) hi[i] = b;
  }
}

int sorted_build(const TextBatch& b, BatchForm form, int64_t m, int64_t known_max, void* stream, mrx_sorted** out) {
  if (m < 0) return internal_fail(MRX_E_ARGUMENT, "m must be >= 0");
  if (!out) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = check_batch(b, form)) return rc;
  if (m >= ((int64_t)1 << 31)) return internal_fail(MRX_E_ARGUMENT, kTooMany);
  hipStream_t hs = (hipStream_t)stream;
  mrx_sorted* s = new mrx_sorted();
  struct Guard {   // the handle goes back on every early way out
    mrx_sorted* s;
    ~Guard() { delete s; }
  } guard{s};
  s->m = m;
  s->fstep = sorted_fence_step(m);
  s->fcount = (int)((m + s->fstep - 1) / s->fstep);
  const size_t words = (size_t)(m > 0 ? m : 1);
  MRX_HIP_TRY(hipMalloc((void**)&s->order, sizeof(int64_t) * words));
  MRX_HIP_TRY(hipMalloc((void**)&s->offsets, sizeof(int64_t) * (words + 1)));
  MRX_HIP_TRY(hipMalloc((void**)&s->keys, sizeof(uint64_t) * words));
  MRX_HIP_TRY(hipMalloc((void**)&s->valids, words));
  MRX_HIP_TRY(hipMalloc((void**)&s->fkey, sizeof(uint64_t) * kSortedFence));
  MRX_HIP_TRY(hipMalloc((void**)&s->fvalid, kSortedFence));
  if (m == 0) {   // no entry: every bisect answers 0, every longest prefix -1
    MRX_HIP_TRY(hipMemsetAsync(s->offsets, 0, sizeof(int64_t), hs));
    MRX_HIP_TRY(hipMalloc((void**)&s->data, 16));
    MRX_HIP_TRY(hipStreamSynchronize(hs));
    guard.s = nullptr;
    *out = s;
    return MRX_OK;
  }
  ScratchScope scope_(stream);
  int64_t* klen = (int64_t*)scratch_get(sizeof(int64_t) * words, stream);
  int64_t* tail = (int64_t*)scratch_get(sizeof(int64_t) * 4, stream);   // {entries, bytes} for the gather, the distinct count
  if (!klen || !tail) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  {
    const ScratchMark mark = scratch_mark(stream);   // sort's 76 bytes a text go back before the gather takes its own
    if (int rc = sort_order_of(b, form, m, known_max, s->order, tail + 2, stream)) return rc;
    scratch_rewind(stream, mark);
  }
  const dim3 blk(kSortedBlock);
  hipLaunchKernelGGL(k_sorted_lengths, dim3(sorted_grid(m)), blk, 0, hs, b, m, s->order, klen, tail);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(klen, m, s->offsets, tail + 1, stream)) return rc;
  int64_t got[3] = {0, 0, 0};
  MRX_HIP_TRY(hipMemcpyAsync(got, tail, sizeof(got), hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));   // the copy's size
  s->bytes = got[1];
  s->distinct = got[2];
  // 16 bytes more than the entries: the aligned 16-byte word around the last entry's end is the handle's own, and the
  // allocation's alignment makes the word around the first entry's start begin with it
  MRX_HIP_TRY(hipMalloc((void**)&s->data, (size_t)s->bytes + 16));
  if (int rc = filter_gather_kept(b, m, known_max, s->order, s->offsets, tail, s->data, s->bytes, stream)) return rc;
  const SortedView view{s->data, s->offsets, m, nullptr, nullptr, nullptr, nullptr, s->fstep, s->fcount};
  hipLaunchKernelGGL(k_sorted_keys, dim3(sorted_grid(m)), blk, 0, hs, view, s->keys, s->valids, s->fkey, s->fvalid);
  MRX_HIP_TRY(hipGetLastError());
  MRX_HIP_TRY(hipStreamSynchronize(hs));   // the caller's batch may go, and the scratch with this call
  guard.s = nullptr;
  *out = s;
  return MRX_OK;
}

int sorted_search(const mrx_sorted* s, uint32_t mode, const TextBatch& b, BatchForm form, int64_t n, int64_t* d_lo,
                  int64_t* d_hi, void* stream) {
  if (!s) return internal_fail(MRX_E_ARGUMENT, "null sorted index");
  if (mode != MRX_SORTED_EQUAL && mode != MRX_SORTED_PREFIX && mode != MRX_SORTED_LONGEST)
    return internal_fail(MRX_E_ARGUMENT, "unknown search mode");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (n > 0 && !d_lo && !d_hi) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n == 0) return MRX_OK;
  const int aids = g_sorted_aids.load(std::memory_order_relaxed);
  const bool keys = (aids & SORTED_AID_KEYS) != 0, fence = keys && (aids & SORTED_AID_FENCE) != 0;
  const SortedView view{s->data,
                        s->offsets,
                        s->m,
                        keys ? s->keys : nullptr,
                        keys ? s->valids : nullptr,
                        fence ? s->fkey : nullptr,
                        fence ? s->fvalid : nullptr,
                        s->fstep,
                        fence ? s->fcount : 0};
  hipLaunchKernelGGL(k_sorted_search, dim3(sorted_grid(n)), dim3(kSortedBlock), 0, (hipStream_t)stream, view, b, n, mode, d_lo,
                     d_hi);
  MRX_HIP_TRY(hipGetLastError());
  set_last_kernel("k_sorted_search");
  return MRX_OK;
}

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_sorted_build_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t m, void* stream, mrx_sorted** out) {
  return sorted_build(csr(d_data, d_offsets), BATCH_CSR, m, -1, stream, out);
}
int mrx_sorted_build_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t m,
                                 void* stream, mrx_sorted** out) {
  const TextBatch b = strided(d_data, stride, d_lens, len);
  return sorted_build(b, BATCH_PITCH, m, b.pitch_longest(), stream, out);
}
void mrx_sorted_free(mrx_sorted* s) { delete s; }
int64_t mrx_sorted_size(const mrx_sorted* s) { return s ? s->m : 0; }
int64_t mrx_sorted_distinct(const mrx_sorted* s) { return s ? s->distinct : 0; }

int mrx_sorted_order_dev(const mrx_sorted* s, int64_t* d_order, void* stream) {
  if (!s) return internal_fail(MRX_E_ARGUMENT, "null sorted index");
  if (s->m > 0 && !d_order) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (s->m > 0)
    MRX_HIP_TRY(hipMemcpyAsync(d_order, s->order, sizeof(int64_t) * (size_t)s->m, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MRX_OK;
}

int mrx_sorted_search_dev(const mrx_sorted* s, uint32_t mode, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                          int64_t* d_lo, int64_t* d_hi, void* stream) {
  return sorted_search(s, mode, csr(d_data, d_offsets), BATCH_CSR, n, d_lo, d_hi, stream);
}
int mrx_sorted_search_strided_dev(const mrx_sorted* s, uint32_t mode, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                                  int32_t len, int64_t n, int64_t* d_lo, int64_t* d_hi, void* stream) {
  return sorted_search(s, mode, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, d_lo, d_hi, stream);
}

// host buffers: argument errors before any device work, as the _dev entry points
int mrx_sorted_search_batch(const uint8_t* entry_data, const int64_t* entry_offsets, int64_t m, uint32_t mode, const uint8_t* data,
                            const int64_t* offsets, int64_t n, int64_t* lo, int64_t* hi) {
  if (m < 0 || n < 0) return internal_fail(MRX_E_ARGUMENT, "m and n must be >= 0");
  if (mode != MRX_SORTED_EQUAL && mode != MRX_SORTED_PREFIX && mode != MRX_SORTED_LONGEST)
    return internal_fail(MRX_E_ARGUMENT, "unknown search mode");
  if (!entry_offsets || !offsets || (n > 0 && !lo && !hi)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (m >= ((int64_t)1 << 31)) return internal_fail(MRX_E_ARGUMENT, kTooMany);
  DevBatch e, b;
  DevBuf<int64_t> dl, dh;
  if (int rc = e.measure(entry_offsets, m)) return rc;
  if (int rc = b.measure(offsets, n)) return rc;
  if (e.nbytes < 0 || b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if ((e.nbytes > 0 && !entry_data) || (b.nbytes > 0 && !data)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = e.upload(entry_data, entry_offsets, m)) return rc;
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = dl.alloc((size_t)n)) return rc;
  if (int rc = dh.alloc((size_t)n)) return rc;
  mrx_sorted* s = nullptr;
  if (int rc = sorted_build(csr(e.data, e.offsets), BATCH_CSR, m, e.longest, nullptr, &s)) return rc;
  int rc = sorted_search(s, mode, csr(b.data, b.offsets), BATCH_CSR, n, dl.p, dh.p, nullptr);
  if (rc == MRX_OK && n > 0 &&
      ((lo && hipMemcpy(lo, dl.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) ||
       (hi && hipMemcpy(hi, dh.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)))
    rc = internal_fail(MRX_E_NO_DEVICE, "copying the positions to the host failed");
  delete s;   // (behind the copies, which waited for the search)
  return rc;
}

void mrx_debug_sorted_grid(int workgroups) { g_sorted_grid = workgroups > 0 ? workgroups : 0; }
int mrx_debug_sorted_aids(int mask) {
  if (mask >= 0) g_sorted_aids = mask & (SORTED_AID_KEYS | SORTED_AID_FENCE);
  else if (mask == -1) g_sorted_aids = kSortedAidsDefault;
  return g_sorted_aids.load();
}

}  // extern "C"
