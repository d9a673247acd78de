// Filter (include/mrx.h, "filter"): the texts in which a pattern's search matches -- or any / all members of a set
// match -- compacted into a new packed CSR batch on the device, in their original order.
//
// Route.  The predicate is the existing one and nothing else: one pattern runs its search
// (run_search_any through member_search) into scratch, a set its matches call (the members' search hits as bit rows).
//   k_filter_flags    kept length and keep flag of every text, set mode and inversion folded in
//   exclusive_scan    twice: byte positions (total -> d_totals[1]) and ranks (total -> d_totals[0])
//   k_filter_scatter  d_kept_idx and d_out_offsets
//   k_filter_gather / k_filter_gather_text   the bytes
// Everything is enqueued without a look at the device in between: the gather reads kept and bytes from d_totals and
// writes nothing when the bytes exceed out_cap.  With a host `totals` the call reads d_totals back once, at the end.
//
// The gather is output centric: a lane owns one 16-byte block of the output, aligned on the output ADDRESS, whatever
// texts lie in it.  It finds the kept text that holds the block's first byte, then takes bytes from that text and
// the following ones until the block is full: each piece is read from its source through a 32-byte register window
// (two aligned 16-byte loads, the second only when the piece reaches into it), shifted into place and or-ed into the
// block.  A block inside the output goes out as one aligned 16-byte store; only the first block (an unaligned
// d_out_data) and the last one (the end of the output) are written byte by byte, so nothing outside [0, bytes) is
// touched.  Work is balanced by output bytes, not by texts: a 4 MiB text is 2^18 blocks spread over every wavefront,
// 64-byte texts share blocks and each lane loops over the texts in its block.
// The search for a block's text is what a lane per block would pay log2(kept) dependent loads for.  A wavefront takes
// one contiguous run of blocks, 64 per round: it bisects all kept texts once for its first block, then per round
// gallops forward from the last round's text to the text of the round's last byte (uniform, broadcast loads), and
// each lane bisects only the texts between the two -- none at all inside a long text.  That walk is gather_blocks
// (mrx_gather_bits.hpp), the one copy that extract, expand and format use too; k_filter_gather adds its block's fill.
// k_filter_gather_text is the text-centric form for batches of short texts: 16 lanes take one kept text, move the
// aligned 16-byte blocks that lie inside its output row through the same window and write the row's unaligned head
// and tail byte by byte.  One text's offsets and index are loaded once for all its blocks, which is why it measured
// faster than the block form on texts of 64 bytes to 1 KiB (profiles/filter.md); on 4 MiB texts it is 8 to 16 times
// slower (16 lanes walk a text alone), and a workgroup per text lost to the block form there and was dropped.
// Route rule (a pure function of the batch shape, nothing is timed): the text form when the batch's longest text is
// known to the host -- a fixed pitch, or a CSR batch with known bounds -- and at most kFilterTextMax bytes; the block
// form otherwise, so a CSR batch of unknown shape is served by the form that no outlier can starve.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_gather_bits.hpp"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"

namespace mrx {
namespace {

constexpr uint32_t kFilterFlags = MRX_FILTER_INVERT | MRX_FILTER_ALL;
constexpr int kFilterBlock = 256;
constexpr unsigned kFilterMaxGrid = 2048;   // 8 workgroups per CU; the kernels stride over what is left

constexpr int kFilterLanes = 16;            // lanes per kept text in k_filter_gather_text
constexpr int64_t kFilterTextMax = 4096;    // the text form serves batches whose longest text is at most this

std::atomic<int> g_filter_form{0};   // mrx_debug_filter_form(): 0 rule, 1 block form, 16 text form

// what the scatter wrote and the gather reads
struct FilterOut {
  const int64_t* kept_idx;   // [kept] original index of each kept text
  const int64_t* out_off;    // [kept + 1] CSR of the output
  const int64_t* totals;     // {kept, bytes}
  uint8_t* out;
  int64_t out_cap;
};

// one pattern: start[i] >= 0.  A set: bit row i of its matches call (k members, `words` words a text), any bit or,
// with MRX_FILTER_ALL, every one of the k.  MRX_FILTER_INVERT negates.
__global__ __launch_bounds__(kFilterBlock) void k_filter_flags(const TextBatch B, int64_t n,
                                                               const int32_t* __restrict__ start,
                                                               const uint64_t* __restrict__ bits, int k, int words,
                                                               uint32_t flags, int64_t* __restrict__ klen,
                                                               int64_t* __restrict__ keep) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    bool hit;
    if (start) {
      hit = start[i] >= 0;
    } else if (flags & MRX_FILTER_ALL) {
      hit = true;
      for (int w = 0; w < words; ++w) {
        const uint64_t full = (w == words - 1 && (k & 63)) ? ((1ull << (k & 63)) - 1) : ~0ull;
        hit = hit && (bits[i * words + w] & full) == full;
      }
    } else {
      hit = false;
      for (int w = 0; w < words; ++w) hit = hit || bits[i * words + w] != 0;
    }
    const bool kp = hit != ((flags & MRX_FILTER_INVERT) != 0);
    int32_t L = 0;
    (void)B.text(i, &L);
    klen[i] = kp ? (int64_t)L : 0;
    keep[i] = kp ? 1 : 0;
  }
}

// rank[n + 1], pos[n + 1]: the exclusive scans of keep and klen.  Entry n closes the output's CSR.
__global__ __launch_bounds__(kFilterBlock) void k_filter_scatter(int64_t n, const int64_t* __restrict__ keep,
                                                                 const int64_t* __restrict__ rank,
                                                                 const int64_t* __restrict__ pos,
                                                                 int64_t* __restrict__ kept_idx,
                                                                 int64_t* __restrict__ out_off) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i == n) {
      out_off[rank[n]] = pos[n];
    } else if (keep[i]) {
      const int64_t r = rank[i];
      kept_idx[r] = i;
      out_off[r] = pos[i];
    }
  }
}

__global__ __launch_bounds__(kFilterBlock) void k_filter_gather(const TextBatch B, const FilterOut O) {
  const int64_t kept = O.totals[0], bytes = O.totals[1];
  if (bytes <= 0 || bytes > O.out_cap) return;
  gather_blocks<kFilterBlock>(O.out, bytes, O.out_off, kept, [&](int64_t r, int64_t, int64_t p0, int64_t pos, int64_t endp) {
    g_u128 acc = 0;
    while (pos < endp) {   // the kept texts of the block one by one: most have a byte
      const int64_t s = O.out_off[r], e = O.out_off[r + 1];
      if (e > pos) {
        const int take = (int)((e < endp ? e : endp) - pos);
        int32_t L;
        const uint8_t* tp = B.text(O.kept_idx[r], &L);
        acc = gather_place(acc, tp + (pos - s), take, (int)(pos - p0));
        pos += take;
      }
      ++r;
    }
    return acc;
  });
}

__global__ __launch_bounds__(kFilterBlock) void k_filter_gather_text(const TextBatch B, const FilterOut O) {
  constexpr int G = kFilterLanes;
  const int64_t kept = O.totals[0], bytes = O.totals[1];
  if (bytes <= 0 || bytes > O.out_cap) return;
  const int sub = (int)threadIdx.x % G;
  const int64_t ngroups = (int64_t)gridDim.x * (kFilterBlock / G);
  for (int64_t r = (int64_t)blockIdx.x * (kFilterBlock / G) + (int)threadIdx.x / G; r < kept; r += ngroups) {
    const int64_t s = O.out_off[r], len = O.out_off[r + 1] - s;
    if (len <= 0) continue;
    int32_t L;
    const uint8_t* tp = B.text(O.kept_idx[r], &L);
    uint8_t* dst = O.out + s;
    const int64_t to_boundary = (int64_t)((16 - ((uintptr_t)dst & 15)) & 15);
    const int64_t h = to_boundary < len ? to_boundary : len;   // bytes in front of the row's first aligned block
    const int64_t t0 = h + ((len - h) & ~(int64_t)15);         // ... and from here on behind its last one
    for (int64_t q = sub; q < h; q += G) dst[q] = tp[q];
    for (int64_t q = h + 16 * (int64_t)sub; q < t0; q += 16 * (int64_t)G) gather_store16(dst + q, gather_window(tp + q, 16));
    for (int64_t q = t0 + sub; q < len; q += G) dst[q] = tp[q];
  }
}

unsigned filter_grid(int64_t items, int64_t per) { return grid_for(items, per, kFilterMaxGrid); }

// the route rule: the text form when the host knows the batch's longest text and it is at most kFilterTextMax
bool filter_text_form(const TextBatch& b, int64_t known_max) {
  const int forced = g_filter_form.load(std::memory_order_relaxed);
  const int64_t longest = b.offsets ? known_max : b.pitch_longest();   // < 0: not known to the host
  return forced ? forced == 16 : (longest >= 0 && longest <= kFilterTextMax);
}

struct FilterArgs : PackedDest {   // d_rows: d_kept_idx
  uint32_t flags;
};

// argument errors, then refusals: nothing has touched the device when one of them returns
int filter_check(const mrx_handle* h, const mrx_set* set, bool is_set, const TextBatch& b, BatchForm form, int64_t n,
                 const FilterArgs& a) {
  if (is_set ? !set : !h) return internal_fail(MRX_E_ARGUMENT, is_set ? "null set" : "null handle");
  if (a.flags & ~kFilterFlags) return internal_fail(MRX_E_ARGUMENT, "unknown flag bits");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (a.out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "out_cap must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (!a.d_out_offsets || !a.d_totals || (n > 0 && !a.d_rows) || (a.out_cap > 0 && !a.d_out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  const std::string refused = is_set ? set_members_refusal(set) : handle_refusal(h);
  if (!refused.empty()) return internal_fail(MRX_E_UNSUPPORTED, refused);
  return MRX_OK;
}

int filter_run(const mrx_handle* h, const mrx_set* set, bool is_set, const TextBatch& b, BatchForm form, int64_t n,
               int64_t known_total, int64_t known_max, const FilterArgs& a) {
  if (int rc = filter_check(h, set, is_set, b, form, n, a)) return rc;
  hipStream_t hs = (hipStream_t)a.stream;
  if (n == 0) return filter_no_text(b, known_max, a);
  ScratchScope scope_(a.stream);
  const int k = is_set ? (int)mrx_set_size(set) : 1;
  const int words = (k + 63) / 64;
  int64_t* klen = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, a.stream);
  int64_t* keep = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, a.stream);
  int64_t* pos = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(n + 1), a.stream);
  int64_t* rank = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(n + 1), a.stream);
  // the predicate's answer: start / end of one pattern's search, or the set's bit rows
  void* pred = scratch_get(is_set ? sizeof(uint64_t) * (size_t)n * words : sizeof(int32_t) * 2 * (size_t)n, a.stream);
  if (!klen || !keep || !pos || !rank || !pred) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  if (is_set) {
    if (int rc = set_matches(set, b, n, (uint64_t*)pred, a.stream, known_total, known_max)) return rc;
  } else {
    if (int rc = member_search(h, b, n, (int32_t*)pred, (int32_t*)pred + n, a.stream, known_total, known_max)) return rc;
  }
  const dim3 blk(kFilterBlock);
  hipLaunchKernelGGL(k_filter_flags, dim3(filter_grid(n, kFilterBlock)), blk, 0, hs, b, n, is_set ? nullptr : (const int32_t*)pred,
                     is_set ? (const uint64_t*)pred : nullptr, k, words, a.flags, klen, keep);
  MRX_HIP_TRY(hipGetLastError());
  return filter_compact(b, n, known_max, FilterWork{klen, keep, pos, rank}, a);
}

int filter_known(const mrx_handle* h, const mrx_set* set, bool is_set, const uint8_t* d_data, const int64_t* d_offsets,
                 int64_t n, int64_t end_offset, int64_t max_text_len, const FilterArgs& a) {
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return filter_run(h, set, is_set, csr(d_data, d_offsets), BATCH_CSR, n, end_offset, max_text_len, a);
}

// host buffers: argument errors and refusals before any device work, as the _dev entry points
int filter_batch(const mrx_handle* h, const mrx_set* set, bool is_set, uint32_t flags, const uint8_t* data,
                 const int64_t* offsets, int64_t n, int64_t* kept_idx, int64_t* out_offsets, uint8_t* out_data,
                 int64_t out_cap, int64_t* totals) {
  if (is_set ? !set : !h) return internal_fail(MRX_E_ARGUMENT, is_set ? "null set" : "null handle");
  if (flags & ~kFilterFlags) return internal_fail(MRX_E_ARGUMENT, "unknown flag bits");
  if (n < 0 || out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "n and out_cap must be >= 0");
  if (!offsets || !out_offsets || (n > 0 && !kept_idx) || (out_cap > 0 && !out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  const std::string refused = is_set ? set_members_refusal(set) : handle_refusal(h);
  if (!refused.empty()) return internal_fail(MRX_E_UNSUPPORTED, refused);
  DevBatch b; DevBuf<int64_t> ki, oo, dt; DevBuf<uint8_t> od;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = ki.alloc((size_t)n)) return rc;
  if (int rc = oo.alloc((size_t)n + 1)) return rc;
  if (int rc = dt.alloc(2)) return rc;
  if (int rc = od.alloc((size_t)out_cap)) return rc;
  int64_t tot[2] = {0, 0};
  const FilterArgs a{{ki.p, oo.p, od.p, out_cap, dt.p, tot, nullptr}, flags};
  const int rc = filter_known(h, set, is_set, b.data, b.offsets, n, b.nbytes, b.longest, a);
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  if (totals) { totals[0] = tot[0]; totals[1] = tot[1]; }
  if (tot[0] > 0) MRX_HIP_TRY(hipMemcpy(kept_idx, ki.p, sizeof(int64_t) * (size_t)tot[0], hipMemcpyDeviceToHost));
  MRX_HIP_TRY(hipMemcpy(out_offsets, oo.p, sizeof(int64_t) * (size_t)(tot[0] + 1), hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot[1] > 0) MRX_HIP_TRY(hipMemcpy(out_data, od.p, (size_t)tot[1], hipMemcpyDeviceToHost));
  return rc;
}

}  // namespace

int filter_no_text(const TextBatch& b, int64_t known_max, const PackedDest& a) {
  if (int rc = packed_empty(a)) return rc;
  set_last_kernel(filter_text_form(b, known_max) ? "k_filter_gather_text" : "k_filter_gather");
  return MRX_OK;
}

int filter_compact(const TextBatch& b, int64_t n, int64_t known_max, const FilterWork& w, const PackedDest& a) {
  hipStream_t hs = (hipStream_t)a.stream;
  if (int rc = exclusive_scan(w.klen, n, w.pos, a.d_totals + 1, a.stream)) return rc;
  if (int rc = exclusive_scan(w.keep, n, w.rank, a.d_totals, a.stream)) return rc;
  hipLaunchKernelGGL(k_filter_scatter, dim3(filter_grid(n + 1, kFilterBlock)), dim3(kFilterBlock), 0, hs, n, w.keep, w.rank, w.pos,
                     a.d_rows, a.d_out_offsets);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = filter_gather_kept(b, n, known_max, a.d_rows, a.d_out_offsets, a.d_totals, a.d_out_data, a.out_cap, a.stream))
    return rc;
  return packed_verdict(a);
}

int filter_gather_kept(const TextBatch& b, int64_t n, int64_t known_max, const int64_t* d_kept_idx,
                       const int64_t* d_out_offsets, const int64_t* d_totals, uint8_t* d_out_data, int64_t out_cap,
                       void* stream) {
  const bool text_form = filter_text_form(b, known_max);
  if (out_cap > 0) {   // (nothing fits a capacity of 0, and no empty output has a byte to move)
    hipStream_t hs = (hipStream_t)stream;
    const dim3 blk(kFilterBlock);
    const FilterOut O{d_kept_idx, d_out_offsets, d_totals, d_out_data, out_cap};
    if (text_form)
      hipLaunchKernelGGL(k_filter_gather_text, dim3(filter_grid(n, kFilterBlock / kFilterLanes)), blk, 0, hs, b, O);
    else   // a wavefront per 64 blocks = 1 KiB of output at least
      hipLaunchKernelGGL(k_filter_gather, dim3(filter_grid(out_cap / 16 + 2, kFilterBlock)), blk, 0, hs, b, O);
    MRX_HIP_TRY(hipGetLastError());
  }
  set_last_kernel(text_form ? "k_filter_gather_text" : "k_filter_gather");
  return MRX_OK;
}
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_filter_dev(const mrx_handle* h, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                   int64_t* d_kept_idx, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                   int64_t* totals, void* stream) {
  return filter_run(h, nullptr, false, csr(d_data, d_offsets), BATCH_CSR, n, -1, -1,
                    FilterArgs{{d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, flags});
}
int mrx_filter_known_dev(const mrx_handle* h, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                         int64_t end_offset, int64_t max_text_len, int64_t* d_kept_idx, int64_t* d_out_offsets,
                         uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  return filter_known(h, nullptr, false, d_data, d_offsets, n, end_offset, max_text_len,
                      FilterArgs{{d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, flags});
}
int mrx_filter_strided_dev(const mrx_handle* h, uint32_t flags, const uint8_t* d_data, int64_t stride,
                           const int32_t* d_lens, int32_t len, int64_t n, int64_t* d_kept_idx, int64_t* d_out_offsets,
                           uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  return filter_run(h, nullptr, false, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1, -1,
                    FilterArgs{{d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, flags});
}
int mrx_filter_batch(const mrx_handle* h, uint32_t flags, const uint8_t* data, const int64_t* offsets, int64_t n,
                     int64_t* kept_idx, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals) {
  return filter_batch(h, nullptr, false, flags, data, offsets, n, kept_idx, out_offsets, out_data, out_cap, totals);
}

int mrx_set_filter_dev(const mrx_set* s, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                       int64_t* d_kept_idx, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap,
                       int64_t* d_totals, int64_t* totals, void* stream) {
  return filter_run(nullptr, s, true, csr(d_data, d_offsets), BATCH_CSR, n, -1, -1,
                    FilterArgs{{d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, flags});
}
int mrx_set_filter_known_dev(const mrx_set* s, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                             int64_t end_offset, int64_t max_text_len, int64_t* d_kept_idx, int64_t* d_out_offsets,
                             uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  return filter_known(nullptr, s, true, d_data, d_offsets, n, end_offset, max_text_len,
                      FilterArgs{{d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, flags});
}
int mrx_set_filter_strided_dev(const mrx_set* s, uint32_t flags, const uint8_t* d_data, int64_t stride,
                               const int32_t* d_lens, int32_t len, int64_t n, int64_t* d_kept_idx,
                               int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                               int64_t* totals, void* stream) {
  return filter_run(nullptr, s, true, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1, -1,
                    FilterArgs{{d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, flags});
}
int mrx_set_filter_batch(const mrx_set* s, uint32_t flags, const uint8_t* data, const int64_t* offsets, int64_t n,
                         int64_t* kept_idx, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals) {
  return filter_batch(nullptr, s, true, flags, data, offsets, n, kept_idx, out_offsets, out_data, out_cap, totals);
}

void mrx_debug_filter_form(int form) { g_filter_form = (form == 1 || form == 16) ? form : 0; }

}  // extern "C"
