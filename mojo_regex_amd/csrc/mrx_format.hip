// Format (include/mrx.h, "format"): one record per row from a template, text columns and number columns -- the
// inverse of numbers, shaped like expand -- packed into a new CSR batch on the device, in row order.
//
// Route.  The host parses the template once (parse_repl_template: the grammar of sub and expand) into
// expand's segment table and a literal buffer; the columns that the template names become SLOTS, in column order.  The
// table, the slots' descriptions and the literals are uploaded into the call's scratch, and the call runs
//   k_format_sizes   a lane per row: for each slot the cell's word and descriptor (mrx_format_bits.hpp: a text's
//                    address and length; a number's magnitude, sign, digit count and point position, with the 128-bit
//                    scaling of a FIXED cell done here, once), the record's length and the row's status
//   exclusive_scan   of the lengths, straight into d_out_offsets; sum -> d_totals[1]
//   k_format_gather  the bytes
// The gather is the block walk of the other byte movers (gather_blocks, mrx_gather_bits.hpp); its fill walks the
// record's segments as k_expand_gather's does (format_block).  A literal and a text cell go through gather_place; a
// number cell is rendered in registers and placed by the same mask and shift (format_place).  No atomics, no LDS.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_format_bits.hpp"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"
#include "mrx_plan.hpp"

namespace mrx {
namespace {

constexpr int kFormatBlock = 256;
constexpr unsigned kFormatMaxGrid = 2048;   // 8 workgroups per CU, as expand; the kernels stride over what is left

std::atomic<int> g_format_grid{0};   // mrx_debug_format_grid(): workgroups of both kernels at most (0 = no cap of its own)

// one referenced column, as the sizes kernel reads it
struct FormatCol {
  TextBatch text;           // MRX_COL_TEXT
  const uint64_t* values;   // a number column: int64[n], or the bits of double[n]
  const uint8_t* status;    // ... and its status bytes, or nullptr
  int32_t kind, arg, refs, pad_;
};

struct FormatArgs : PackedDest {   // d_rows: none
  const char* tpl;
  size_t tpl_len;
  const mrx_column* cols;
  int32_t ncols;
  int64_t n;
  uint8_t* d_row_status;
};

TextBatch column_text(const mrx_column& c) {
  return c.d_offsets ? csr((const uint8_t*)c.d_values, c.d_offsets) : strided((const uint8_t*)c.d_values, c.stride, c.d_lens, c.len);
}

// A template on the host.  A reference to a column the call does not have contributes nothing and is dropped here; the
// literals on both sides of it become one segment.  Slots are numbered in column order, so that the first slot whose
// cell is not written is the lowest-numbered such column.
struct HostTpl {
  std::vector<ExpandSeg> segs;
  std::vector<FormatCol> slots;
  std::vector<uint8_t> blob;   // what is uploaded: the segments, the slots, then (16-byte aligned) the literals and 16 bytes more
  size_t slots_at = 0, lits_at = 0;
  int64_t lit_total = 0;
};
HostTpl parse_template(const FormatArgs& a) {
  HostTpl t;
  const std::string r(a.tpl ? a.tpl : "", a.tpl_len);
  const std::vector<ReplSeg> parsed = parse_repl_template(r);
  int refs[10] = {0}, slot_of[10];
  for (const ReplSeg& sg : parsed)
    if (sg.group_ref > 0 && sg.group_ref <= a.ncols) ++refs[sg.group_ref];
  for (int j = 1; j <= 9; ++j) {
    slot_of[j] = -1;
    if (!refs[j]) continue;
    const mrx_column& c = a.cols[j - 1];
    slot_of[j] = (int)t.slots.size();
    t.slots.push_back(FormatCol{c.kind == MRX_COL_TEXT ? column_text(c) : TextBatch{}, (const uint64_t*)c.d_values, c.d_status,
                                c.kind, c.arg, refs[j], 0});
  }
  std::string lits;
  for (const ReplSeg& sg : parsed) {
    if (sg.group_ref > 0) {
      if (sg.group_ref <= a.ncols) t.segs.push_back(ExpandSeg{0, 0, slot_of[sg.group_ref], 0});
    } else {
      if (!t.segs.empty() && t.segs.back().slot < 0) t.segs.back().lit_len += sg.length;
      else t.segs.push_back(ExpandSeg{(int64_t)lits.size(), sg.length, -1, 0});
      lits.append(r, (size_t)sg.start, (size_t)sg.length);
    }
  }
  t.lit_total = (int64_t)lits.size();
  t.slots_at = (sizeof(ExpandSeg) * t.segs.size() + 15) & ~(size_t)15;
  t.lits_at = (t.slots_at + sizeof(FormatCol) * t.slots.size() + 15) & ~(size_t)15;
  t.blob.assign(t.lits_at + ((lits.size() + 15) & ~(size_t)15) + 16, 0);
  if (!t.segs.empty()) memcpy(t.blob.data(), t.segs.data(), sizeof(ExpandSeg) * t.segs.size());
  if (!t.slots.empty()) memcpy(t.blob.data() + t.slots_at, t.slots.data(), sizeof(FormatCol) * t.slots.size());
  if (!lits.empty()) memcpy(t.blob.data() + t.lits_at, lits.data(), lits.size());
  return t;
}

// what the gather reads besides the cells
struct FormatOut {
  FormatSrc S;
  const int64_t* totals;   // {rows, bytes}
  uint8_t* out;
  int64_t out_cap;
};

__global__ __launch_bounds__(kFormatBlock) void k_format_sizes(const FormatCol* __restrict__ cols, int nslots, int64_t lit_total,
                                                                int64_t n, uint64_t* __restrict__ word,
                                                                int32_t* __restrict__ desc, int64_t* __restrict__ plen,
                                                                uint8_t* __restrict__ row_status,
                                                                int64_t* __restrict__ totals) {
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (first == 0) totals[0] = n;
  for (int64_t r = first; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t len = lit_total;
    int rs = MRX_NUM_OK;
    for (int q = 0; q < nslots; ++q) {
      const FormatCol& c = cols[q];
      uint64_t w = 0;
      int32_t d = 0;
      if (c.kind == MRX_COL_TEXT) {
        int32_t L;
        const uint8_t* tp = c.text.text(r, &L);
        w = (uint64_t)(uintptr_t)tp;
        d = L > 0 ? L : 0;
      } else {
        int st = c.status ? (int)c.status[r] : MRX_NUM_OK;
        if (st == MRX_NUM_OK) st = format_cell(c.kind, c.arg, c.values[r], &w, &d);
        if (st != MRX_NUM_OK) {   // nothing is printed, a fill word least of all
          d = 0;
          if (rs == MRX_NUM_OK) rs = st;
        }
      }
      word[(int64_t)q * n + r] = w;
      desc[(int64_t)q * n + r] = d;
      len += (int64_t)c.refs * format_desc_len(d);
    }
    plen[r] = len;
    if (row_status) row_status[r] = (uint8_t)rs;
  }
}

// (no occupancy asked for: expand's bound of 8 waves per SIMD leaves this kernel 64 VGPRs, and the rendering of a number
// cell then spills 40 bytes a lane to scratch memory; without the bound it takes 86 VGPRs, 5 waves per SIMD, no scratch)
__global__ __launch_bounds__(kFormatBlock) void k_format_gather(const FormatOut O) {
  const int64_t rows = O.S.rows, bytes = O.totals[1];
  if (bytes <= 0 || bytes > O.out_cap) return;
  gather_blocks<kFormatBlock>(O.out, bytes, O.S.out_off, rows, [&](int64_t r, int64_t hi, int64_t p0, int64_t pos, int64_t endp) {
    return format_block(O.S, r, hi, p0, pos, endp);
  });
}

unsigned format_grid(int64_t items, int64_t per) {
  return grid_for(items, per, kFormatMaxGrid, g_format_grid.load(std::memory_order_relaxed));
}

// what every entry point refuses about a column whatever memory its pointers mean
int column_spec_check(const mrx_column& c) {
  switch (c.kind) {
    case MRX_COL_TEXT:
      return MRX_OK;
    case MRX_COL_INT10:
    case MRX_COL_INT16:
      if (c.arg < 0 || c.arg > 20) return internal_fail(MRX_E_ARGUMENT, "an integer column's digits K must be in [0, 20]");
      return MRX_OK;
    case MRX_COL_FIXED:
      if (c.arg < 0 || c.arg > 9) return internal_fail(MRX_E_ARGUMENT, "a fixed column's precision P must be in [0, 9]");
      return MRX_OK;
    default:
      return internal_fail(MRX_E_ARGUMENT, "kind must be MRX_COL_TEXT, MRX_COL_INT10, MRX_COL_INT16 or MRX_COL_FIXED");
  }
}

// argument errors: nothing has touched the device when one of them returns
int format_check(const FormatArgs& a) {
  if (a.n < 0 || a.out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "n and out_cap must be >= 0");
  if (a.ncols < 1 || a.ncols > 9) return internal_fail(MRX_E_ARGUMENT, "ncols must be in [1, 9]");
  if (!a.tpl && a.tpl_len > 0) return internal_fail(MRX_E_ARGUMENT, "null template of nonzero length");
  if (!a.cols || !a.d_out_offsets || !a.d_totals || (a.out_cap > 0 && !a.d_out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  for (int j = 0; j < a.ncols; ++j) {
    const mrx_column& c = a.cols[j];
    if (int rc = column_spec_check(c)) return rc;
    if (c.kind == MRX_COL_TEXT)
      if (int rc = check_batch(column_text(c), BATCH_PITCH)) return rc;
    if (a.n > 0 && !c.d_values) return internal_fail(MRX_E_ARGUMENT, "null argument");
  }
  return MRX_OK;
}

int format_run(const FormatArgs& a) {
  if (int rc = format_check(a)) return rc;
  hipStream_t hs = (hipStream_t)a.stream;
  if (a.n == 0) {
    if (int rc = packed_empty(a)) return rc;
    set_last_kernel("k_format_gather");
    return MRX_OK;
  }
  // The template's host copy is pageable memory in this frame: hipMemcpyAsync has staged it when it returns, as for
  // expand's template.
  ScratchScope scope_(a.stream);
  const HostTpl t = parse_template(a);
  const size_t n = (size_t)a.n, nslots = t.slots.size(), cells = n * (nslots ? nslots : 1);
  int64_t* plen = (int64_t*)scratch_get(sizeof(int64_t) * n, a.stream);
  uint64_t* word = (uint64_t*)scratch_get(sizeof(uint64_t) * cells, a.stream);
  int32_t* desc = (int32_t*)scratch_get(sizeof(int32_t) * cells, a.stream);
  uint8_t* d_tpl = (uint8_t*)scratch_get(t.blob.size(), a.stream);
  if (!plen || !word || !desc || !d_tpl) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  MRX_HIP_TRY(hipMemcpyAsync(d_tpl, t.blob.data(), t.blob.size(), hipMemcpyHostToDevice, hs));
  const dim3 blk(kFormatBlock);
  hipLaunchKernelGGL(k_format_sizes, dim3(format_grid(a.n, kFormatBlock)), blk, 0, hs, (const FormatCol*)(d_tpl + t.slots_at),
                     (int)nslots, t.lit_total, a.n, word, desc, plen, a.d_row_status, a.d_totals);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(plen, a.n, a.d_out_offsets, a.d_totals + 1, a.stream)) return rc;
  if (a.out_cap > 0 && !t.segs.empty()) {   // (nothing fits a capacity of 0, and no empty output has a byte to move)
    const FormatOut O{FormatSrc{d_tpl + t.lits_at, (const ExpandSeg*)d_tpl, (int32_t)t.segs.size(), 0, a.n, word, desc, a.d_out_offsets},
                      a.d_totals, a.d_out_data, a.out_cap};
    // a wavefront per 64 blocks = 1 KiB of output at least
    hipLaunchKernelGGL(k_format_gather, dim3(format_grid(a.out_cap / 16 + 2, kFormatBlock)), blk, 0, hs, O);
    MRX_HIP_TRY(hipGetLastError());
  }
  set_last_kernel("k_format_gather");
  return packed_verdict(a);
}

// a host column's buffers on the device
struct DevColumn {
  DevBatch text;
  DevBuf<uint8_t> bytes, status;
  DevBuf<int32_t> lens;
  DevBuf<uint64_t> values;
};

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_format_dev(const char* tpl, size_t tpl_len, const mrx_column* cols, int32_t ncols, int64_t n, int64_t* d_out_offsets,
                   uint8_t* d_out_data, int64_t out_cap, uint8_t* d_row_status, int64_t* d_totals, int64_t* totals,
                   void* stream) {
  return format_run(FormatArgs{{nullptr, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, tpl, tpl_len, cols, ncols, n,
                               d_row_status});
}

// host buffers: argument errors before any device work, as the _dev entry point
int mrx_format_batch(const char* tpl, size_t tpl_len, const mrx_column* cols, int32_t ncols, int64_t n, int64_t* out_offsets,
                     uint8_t* out_data, int64_t out_cap, uint8_t* row_status, int64_t* totals) {
  int64_t fake_totals[2];   // (the device call wants one; this wrapper allocates its own)
  if (int rc = format_check(FormatArgs{{nullptr, out_offsets, out_data, out_cap, fake_totals, nullptr, nullptr}, tpl, tpl_len, cols,
                                       ncols, n, row_status}))
    return rc;
  std::vector<std::unique_ptr<DevColumn>> held;
  std::vector<mrx_column> dcols(cols, cols + ncols);
  for (int j = 0; j < ncols; ++j) {   // measured first: nothing is allocated for offsets that decrease
    const mrx_column& c = cols[j];
    held.emplace_back(new DevColumn);
    if (c.kind != MRX_COL_TEXT || !c.d_offsets) continue;
    if (int rc = held.back()->text.measure(c.d_offsets, n)) return rc;
    for (int64_t i = 0; i < n; ++i)
      if (c.d_offsets[i + 1] < c.d_offsets[i]) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  }
  for (int j = 0; j < ncols && n > 0; ++j) {
    const mrx_column& c = cols[j];
    DevColumn& d = *held[j];
    if (c.kind == MRX_COL_TEXT && c.d_offsets) {
      if (int rc = d.text.upload((const uint8_t*)c.d_values, c.d_offsets, n)) return rc;
      dcols[j].d_values = d.text.data;
      dcols[j].d_offsets = d.text.offsets;
    } else if (c.kind == MRX_COL_TEXT) {
      const size_t nb = (size_t)n * (size_t)c.stride;
      if (int rc = d.bytes.alloc(nb + 64)) return rc;
      MRX_HIP_TRY(hipMemcpy(d.bytes.p, c.d_values, nb, hipMemcpyHostToDevice));
      dcols[j].d_values = d.bytes.p;
      if (c.d_lens) {
        if (int rc = d.lens.alloc((size_t)n)) return rc;
        MRX_HIP_TRY(hipMemcpy(d.lens.p, c.d_lens, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
        dcols[j].d_lens = d.lens.p;
      }
    } else {
      if (int rc = d.values.alloc((size_t)n)) return rc;
      MRX_HIP_TRY(hipMemcpy(d.values.p, c.d_values, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice));
      dcols[j].d_values = d.values.p;
      if (c.d_status) {
        if (int rc = d.status.alloc((size_t)n)) return rc;
        MRX_HIP_TRY(hipMemcpy(d.status.p, c.d_status, (size_t)n, hipMemcpyHostToDevice));
        dcols[j].d_status = d.status.p;
      }
    }
  }
  DevBuf<int64_t> oo, dt;
  DevBuf<uint8_t> od, rs;
  if (int rc = oo.alloc((size_t)n + 1)) return rc;
  if (int rc = dt.alloc(2)) return rc;
  if (int rc = od.alloc((size_t)out_cap)) return rc;
  if (int rc = rs.alloc((size_t)n)) return rc;
  int64_t tot[2] = {0, 0};
  const int rc = format_run(FormatArgs{{nullptr, oo.p, od.p, out_cap, dt.p, tot, nullptr}, tpl, tpl_len, dcols.data(), ncols, n,
                                       row_status ? rs.p : nullptr});
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  if (totals) { totals[0] = tot[0]; totals[1] = tot[1]; }
  MRX_HIP_TRY(hipMemcpy(out_offsets, oo.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost));
  if (row_status && n > 0) MRX_HIP_TRY(hipMemcpy(row_status, rs.p, (size_t)n, hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot[1] > 0) MRX_HIP_TRY(hipMemcpy(out_data, od.p, (size_t)tot[1], hipMemcpyDeviceToHost));
  return rc;
}

void mrx_debug_format_grid(int workgroups) { g_format_grid = workgroups > 0 ? workgroups : 0; }

int mrx_testing_format_one(int32_t kind, int32_t arg, int64_t value_word, uint8_t out[32]) {
  const mrx_column c{kind, arg, nullptr, nullptr, 0, nullptr, 0, 0, nullptr};
  if (kind == MRX_COL_TEXT || !out) return -(int)MRX_NUM_MALFORMED;
  if (column_spec_check(c)) return -(int)MRX_NUM_MALFORMED;
  uint64_t mag = 0;
  int32_t desc = 0;
  const int st = format_cell(kind, arg, (uint64_t)value_word, &mag, &desc);
  if (st != MRX_NUM_OK) return -st;
  return format_cell_bytes(mag, desc, out);
}

}  // extern "C"
