// Host code that the entry points share.  The packed-output tail of the byte movers: the n == 0 result, the read-back
// of {rows, bytes} with the capacity verdict, and the workgroup count.  Host-buffer staging of the mrx_*_batch wrappers
// (mrx_kernels.hip, mrx_sub.hip, mrx_capall.hip, mrx_split.hip, mrx_set.hip): a CSR batch copied to the device with
// offsets made relative to its first byte, and device buffers for the outputs, all freed on every way out.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mrx.h"
#include "mrx_internal.hpp"

#define MRX_HIP_TRY(expr)                                                                                    \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess)                                                                                    \
      return mrx::internal_fail(MRX_E_NO_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));         \
  } while (0)

namespace mrx {
// ---- the packed-output tail of the byte movers (PackedDest, mrx_internal.hpp) --------------------------------------
// The n == 0 result: an output CSR of no row and {0, 0} on both sides.  (The kernel's name is the caller's to report.)
// ntotals: the entries of the totals, {rows, bytes} first (lines has four).
inline int packed_empty(const PackedDest& d, int ntotals = 2) {
  hipStream_t hs = (hipStream_t)d.stream;
  MRX_HIP_TRY(hipMemsetAsync(d.d_out_offsets, 0, sizeof(int64_t), hs));
  MRX_HIP_TRY(hipMemsetAsync(d.d_totals, 0, ntotals * sizeof(int64_t), hs));
  if (d.totals) std::fill(d.totals, d.totals + ntotals, (int64_t)0);
  return MRX_OK;
}
// Behind the gather.  Without a host `totals` the call has only enqueued; with one, d_totals = {rows, bytes} is read
// back once and turned into the verdict.  piece_cap: the capacity in rows of an operation that has one (extract,
// expand), else < 0.  failed: the message of an operation whose kernels report a failure of their own as rows < 0 (take,
// distinct), else nullptr.  ntotals: the entries of the totals that are read back (lines: four).
inline int packed_verdict(const PackedDest& d, int64_t piece_cap = -1, const char* failed = nullptr, int ntotals = 2) {
  if (!d.totals) return MRX_OK;
  hipStream_t hs = (hipStream_t)d.stream;
  MRX_HIP_TRY(hipMemcpyAsync(d.totals, d.d_totals, ntotals * sizeof(int64_t), hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));
  if (failed && d.totals[0] < 0) return internal_fail(MRX_E_ARGUMENT, failed);
  if (piece_cap >= 0 && d.totals[0] > piece_cap)
    return internal_fail(MRX_E_CAPACITY, "piece buffers too small: need " + std::to_string(d.totals[0]));
  if (d.totals[1] > d.out_cap)
    return internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(d.totals[1]));
  return MRX_OK;
}
// workgroups for `items` at `per` a workgroup: at least one, at most max_grid, and at most `cap` where a test has set
// one (mrx_debug_*_grid; 0 = none)
inline unsigned grid_for(int64_t items, int64_t per, unsigned max_grid, int cap = 0) {
  int64_t g = (items + per - 1) / per;
  g = g < 1 ? 1 : g > (int64_t)max_grid ? (int64_t)max_grid : g;
  return (unsigned)(cap > 0 && g > cap ? cap : g);
}

// ---- host-buffer staging -------------------------------------------------------------------------------------------
struct DevBatch {
  uint8_t* data = nullptr;
  int64_t* offsets = nullptr;
  int64_t nbytes = 0;    // after measure(): bytes of the batch, and its longest text
  int64_t longest = 0;
  std::vector<int64_t> rel;
  ~DevBatch() { if (data) (void)hipFree(data); if (offsets) (void)hipFree(offsets); }
  // host work only, so that a wrapper can still refuse (nbytes < 0: the offsets decrease) before anything is allocated
  int measure(const int64_t* h_off, int64_t n) {
    if (n < 0 || !h_off) return internal_fail(MRX_E_ARGUMENT, "bad batch");
    rel.resize((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) {
      rel[i] = h_off[i] - h_off[0];
      if (i > 0) longest = std::max(longest, rel[i] - rel[i - 1]);
    }
    nbytes = rel[n];
    return MRX_OK;
  }
  int upload(const uint8_t* h_data, const int64_t* h_off, int64_t n) {
    if (rel.empty())
      if (int rc = measure(h_off, n)) return rc;
    MRX_HIP_TRY(hipMalloc((void**)&data, (size_t)nbytes + 64));
    MRX_HIP_TRY(hipMalloc((void**)&offsets, sizeof(int64_t) * (n + 1)));
    if (nbytes) MRX_HIP_TRY(hipMemcpy(data, h_data + h_off[0], (size_t)nbytes, hipMemcpyHostToDevice));
    MRX_HIP_TRY(hipMemcpy(offsets, rel.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));
    return MRX_OK;
  }
};
template <class T>
struct DevBuf {
  T* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t count) { MRX_HIP_TRY(hipMalloc((void**)&p, sizeof(T) * (count ? count : 1))); return MRX_OK; }
};
// the packed-batch outputs of the extract family (mrx_extract.hip, mrx_expand.hip) on host buffers: device buffers for
// them, and what is valid copied out
struct HostOut {
  int64_t* owner;
  int64_t* out_offsets;
  uint8_t* out_data;
  int64_t* totals;
};
struct DevOut {
  DevBuf<int64_t> ow, oo, dt;
  DevBuf<uint8_t> od;
  int alloc(int64_t piece_cap, int64_t out_cap) {
    if (int rc = ow.alloc((size_t)piece_cap)) return rc;
    if (int rc = oo.alloc((size_t)piece_cap + 1)) return rc;
    if (int rc = dt.alloc(2)) return rc;
    return od.alloc((size_t)out_cap);
  }
  // rc: the device call's.  owner and offsets when the pieces fit, the bytes when they fit too
  int copy_out(int rc, const int64_t tot[2], int64_t piece_cap, const HostOut& o) {
    if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
    if (o.totals) { o.totals[0] = tot[0]; o.totals[1] = tot[1]; }
    if (tot[0] > piece_cap) return rc;
    if (tot[0] > 0) MRX_HIP_TRY(hipMemcpy(o.owner, ow.p, sizeof(int64_t) * (size_t)tot[0], hipMemcpyDeviceToHost));
    MRX_HIP_TRY(hipMemcpy(o.out_offsets, oo.p, sizeof(int64_t) * (size_t)(tot[0] + 1), hipMemcpyDeviceToHost));
    if (rc == MRX_OK && tot[1] > 0) MRX_HIP_TRY(hipMemcpy(o.out_data, od.p, (size_t)tot[1], hipMemcpyDeviceToHost));
    return rc;
  }
};
inline int host_out_check(int64_t n, int64_t piece_cap, int64_t out_cap, const int64_t* offsets, const HostOut& o) {
  if (n < 0 || piece_cap < 0 || out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "n, piece_cap and out_cap must be >= 0");
  if (!offsets || !o.out_offsets || (piece_cap > 0 && !o.owner) || (out_cap > 0 && !o.out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  return MRX_OK;
}
}  // namespace mrx
