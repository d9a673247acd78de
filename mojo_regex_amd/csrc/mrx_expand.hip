// Expand (include/mrx.h, "expand"): one record per captures_all row -- a template whose \1..\9 are replaced by the
// row's groups, "the bytes sub() puts in place of each match" -- packed into a new CSR batch on the device, in row order.
//
// Route.  The host parses the template once (parse_repl_template: the grammar of sub) into a segment
// table and a literal buffer, uploads both into the call's scratch, and the primitive runs
//   k_expand_sizes   a lane per row: its text by bisection of the row CSR, the clamped pairs of the groups the template
//                    names, then the owner, the record's length and the row's source entry (scratch: the text's
//                    position and the clamped pairs, so that the gather neither bisects for the text nor loads its length)
//   exclusive_scan   of the lengths, straight into d_out_offsets; sum -> d_totals[1]
//   k_expand_gather  the bytes
// mrx_expand_* puts captures_all in front (rows into scratch).  captures_all returns its total through one stream
// synchronisation, so the primitive then runs over exactly that many rows, not over the capacity.
//
// The gather is the block walk of filter and extract (gather_blocks, mrx_gather_bits.hpp).  What is new is inside a
// record: the lane walks the template's segments from the record's start to its own position (expand_seek) and then
// takes bytes segment by segment, from the text for a group and from the literal buffer for a literal (expand_block,
// mrx_expand_bits.hpp).  One form only: work is balanced by output bytes.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_expand_bits.hpp"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"
#include "mrx_plan.hpp"

namespace mrx {
namespace {

constexpr int kExpandBlock = 256;
constexpr unsigned kExpandMaxGrid = 2048;   // 8 workgroups per CU; the kernels stride over what is left

std::atomic<int> g_expand_grid{0};   // mrx_debug_expand_grid(): workgroups of the gather at most (0 = no cap of its own)

// where the records go, the rows and the template: the arguments behind the batch of mrx_expand_spans_dev
struct ExpandArgs : PackedDest {   // d_rows: d_owner
  const int64_t* d_prefix;
  const int32_t* d_groups;   // [rows][row_pairs][2]: the rows of captures_all
  int32_t row_pairs;
  const char* tpl;
  size_t tpl_len;
  int64_t piece_cap;
};

// the groups a template names, each once: slot q is pair[q] of a row and is referenced refs[q] times
struct ExpandSlots {
  int32_t n;
  int32_t pair[9];
  int32_t refs[9];
};

// A template on the host.  A reference to a group the rows do not hold (j > row_pairs - 1) contributes nothing and is
// dropped here; the literals on both sides of it become one segment.
struct HostTpl {
  std::vector<ExpandSeg> segs;
  std::vector<uint8_t> blob;   // what is uploaded: the segment table, then (16-byte aligned) the literals and 16 bytes more
  size_t lits_at = 0;
  ExpandSlots sl{};
  int64_t lit_total = 0;
};
HostTpl parse_template(const char* tpl, size_t tpl_len, int row_pairs) {
  HostTpl t;
  const std::string r(tpl ? tpl : "", tpl_len);
  std::string lits;
  int slot_of[10];
  for (int& s : slot_of) s = -1;
  for (const ReplSeg& sg : parse_repl_template(r)) {
    if (sg.group_ref > 0) {
      if (sg.group_ref > row_pairs - 1) continue;
      int& slot = slot_of[sg.group_ref];
      if (slot < 0) {
        slot = t.sl.n++;
        t.sl.pair[slot] = sg.group_ref - 1;
      }
      ++t.sl.refs[slot];
      t.segs.push_back(ExpandSeg{0, 0, slot, 0});
    } else {
      if (!t.segs.empty() && t.segs.back().slot < 0) t.segs.back().lit_len += sg.length;
      else t.segs.push_back(ExpandSeg{(int64_t)lits.size(), sg.length, -1, 0});
      lits.append(r, (size_t)sg.start, (size_t)sg.length);
    }
  }
  t.lit_total = (int64_t)lits.size();
  t.lits_at = (sizeof(ExpandSeg) * t.segs.size() + 15) & ~(size_t)15;
  t.blob.assign(t.lits_at + ((lits.size() + 15) & ~(size_t)15) + 16, 0);
  if (!t.segs.empty()) memcpy(t.blob.data(), t.segs.data(), sizeof(ExpandSeg) * t.segs.size());
  if (!lits.empty()) memcpy(t.blob.data() + t.lits_at, lits.data(), lits.size());
  return t;
}

// what the sizes kernel and the scan wrote and the gather reads
struct ExpandOut {
  ExpandSrc S;
  const int64_t* totals;   // {pieces, bytes}
  int64_t cap;             // rows the sizes kernel and the scan ran over
  uint8_t* out;
  int64_t out_cap;
};

// Rows that do not all fit get no owner and length 0 (the rows are not read: bytes is then 0, a lower bound).
__global__ __launch_bounds__(kExpandBlock) void k_expand_sizes(const TextBatch B, int64_t n, const int64_t* __restrict__ prefix,
                                                                const int32_t* __restrict__ rows, int row_pairs,
                                                                const ExpandSlots sl, int64_t lit_total, int64_t cap,
                                                                int64_t* __restrict__ owner, int64_t* __restrict__ plen,
                                                                int64_t* __restrict__ base, int32_t* __restrict__ pairs,
                                                                int64_t* __restrict__ totals) {
  const int64_t pieces = prefix[n];
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (first == 0) totals[0] = pieces;
  const int64_t fit = pieces <= cap ? pieces : 0;
  for (int64_t r = first; r < cap; r += (int64_t)gridDim.x * blockDim.x) {
    if (r >= fit) {
      plen[r] = 0;
      continue;
    }
    const int64_t i = gather_last_le(prefix, 0, n, r);   // prefix[i] <= r < prefix[i + 1]: texts without rows are passed
    int32_t L;
    const uint8_t* tp = B.text(i, &L);
    int64_t len = lit_total;
    for (int q = 0; q < sl.n; ++q) {
      const int2 se = *(const int2*)(rows + 2 * (r * row_pairs + sl.pair[q]));
      const int32_t s = se.x < 0 ? 0 : se.x < L ? se.x : L;
      const int32_t e = se.y < s ? s : se.y < L ? se.y : L;
      *(int2*)(pairs + 2 * (r * sl.n + q)) = make_int2(s, e);
      len += (int64_t)sl.refs[q] * (e - s);
    }
    owner[r] = i;
    plen[r] = len;
    base[r] = (int64_t)(tp - B.data);
  }
}

// (8 waves per SIMD asked for: the lookups are latency, not arithmetic; without the bound the kernel takes 65 VGPRs, one
// more than 8 waves allow, with it 62 and still no scratch)
__global__ __launch_bounds__(kExpandBlock, 8) void k_expand_gather(const ExpandOut O) {
  const int64_t pieces = O.totals[0], bytes = O.totals[1];
  if (pieces > O.cap || bytes <= 0 || bytes > O.out_cap) return;
  gather_blocks<kExpandBlock>(O.out, bytes, O.S.out_off, pieces, [&](int64_t r, int64_t hi, int64_t p0, int64_t pos, int64_t endp) {
    return expand_block(O.S, r, hi, p0, pos, endp);
  });
}

// argument errors: nothing has touched the device when one of them returns.  own_rows: the rows are the call's own
// (mrx_expand_*: captures_all's, in scratch)
int expand_check(const TextBatch& b, BatchForm form, int64_t n, const ExpandArgs& a, bool own_rows) {
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (a.piece_cap < 0 || a.out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "piece_cap and out_cap must be >= 0");
  if (a.row_pairs < 1) return internal_fail(MRX_E_ARGUMENT, "row_pairs must be >= 1");
  if (!a.tpl && a.tpl_len > 0) return internal_fail(MRX_E_ARGUMENT, "null template of nonzero length");
  if ((uintptr_t)a.d_groups & 7) return internal_fail(MRX_E_ARGUMENT, "d_rows must be 8-byte aligned");
  if (int rc = check_batch(b, form)) return rc;
  if (!a.d_prefix || !a.d_out_offsets || !a.d_totals || (a.piece_cap > 0 && (!a.d_rows || (!own_rows && !a.d_groups))) ||
      (a.out_cap > 0 && !a.d_out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  return MRX_OK;
}

int expand_empty(const ExpandArgs& a) {   // n == 0
  if (int rc = packed_empty(a)) return rc;
  set_last_kernel("k_expand_gather");
  return MRX_OK;
}

// The device steps on a checked batch with n > 0, inside the caller's ScratchScope, over `cap` rows (the primitive:
// piece_cap; behind captures_all: the rows it found, or 0 when they did not fit); d_prefix[n] and the rows may still be
// on their way on a.stream.  The template's host copy is pageable memory in this frame: hipMemcpyAsync has staged it
// when it returns, as for sub's template.
int expand_enqueue(const TextBatch& b, int64_t n, const ExpandArgs& a, int64_t cap) {
  hipStream_t hs = (hipStream_t)a.stream;
  const HostTpl t = parse_template(a.tpl, a.tpl_len, a.row_pairs);
  const size_t held = (size_t)(cap > 0 ? cap : 1), nslots = (size_t)t.sl.n;
  int64_t* plen = (int64_t*)scratch_get(sizeof(int64_t) * held, a.stream);
  int64_t* base = (int64_t*)scratch_get(sizeof(int64_t) * held, a.stream);
  int32_t* pairs = (int32_t*)scratch_get(sizeof(int32_t) * 2 * held * (nslots ? nslots : 1), a.stream);
  uint8_t* d_tpl = (uint8_t*)scratch_get(t.blob.size(), a.stream);
  if (!plen || !base || !pairs || !d_tpl) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  MRX_HIP_TRY(hipMemcpyAsync(d_tpl, t.blob.data(), t.blob.size(), hipMemcpyHostToDevice, hs));
  const dim3 blk(kExpandBlock);
  hipLaunchKernelGGL(k_expand_sizes, dim3(grid_for(cap, kExpandBlock, kExpandMaxGrid)), blk, 0, hs, b, n, a.d_prefix, a.d_groups,
                     (int)a.row_pairs, t.sl, t.lit_total, cap, a.d_rows, plen, base, pairs, a.d_totals);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(plen, cap, a.d_out_offsets, a.d_totals + 1, a.stream)) return rc;
  if (a.out_cap > 0 && cap > 0 && !t.segs.empty()) {   // (nothing fits a capacity of 0, and no empty output has a byte to move)
    const ExpandOut O{ExpandSrc{b.data, d_tpl + t.lits_at, (const ExpandSeg*)d_tpl, (int32_t)t.segs.size(), t.sl.n, base, pairs,
                                a.d_out_offsets},
                      a.d_totals, cap, a.d_out_data, a.out_cap};
    // a wavefront per 64 blocks = 1 KiB of output at least
    const unsigned grid = grid_for(a.out_cap / 16 + 2, kExpandBlock, kExpandMaxGrid, g_expand_grid.load(std::memory_order_relaxed));
    hipLaunchKernelGGL(k_expand_gather, dim3(grid), blk, 0, hs, O);
    MRX_HIP_TRY(hipGetLastError());
  }
  set_last_kernel("k_expand_gather");
  return packed_verdict(a, a.piece_cap);
}

int spans_run(const TextBatch& b, BatchForm form, int64_t n, const ExpandArgs& a) {
  if (int rc = expand_check(b, form, n, a, false)) return rc;
  if (n == 0) return expand_empty(a);
  ScratchScope scope_(a.stream);
  return expand_enqueue(b, n, a, a.piece_cap);
}

// captures_all's rows into scratch, then the primitive over the rows it found.  Argument errors, then captures_all's
// refusals (its own code and text), before anything is enqueued.
template <class CapturesAll>
int expand_run(const mrx_handle* h, int64_t count, const TextBatch& b, BatchForm form, int64_t n, int64_t* d_match_prefix,
               ExpandArgs a, CapturesAll&& captures_all) {
  if (!h) return internal_fail(MRX_E_ARGUMENT, "null handle");
  if (count < 0) return internal_fail(MRX_E_ARGUMENT, "count must be >= 0");
  a.d_prefix = d_match_prefix;
  a.row_pairs = mrx_num_groups(h) + 1;
  if (int rc = expand_check(b, form, n, a, true)) return rc;
  if (int rc = captures_all_refusal(h)) return rc;
  if (n == 0) {
    MRX_HIP_TRY(hipMemsetAsync(d_match_prefix, 0, sizeof(int64_t), (hipStream_t)a.stream));
    return expand_empty(a);
  }
  ScratchScope scope_(a.stream);
  int32_t* rows = (int32_t*)scratch_get(sizeof(int32_t) * 2 * (size_t)a.row_pairs * (size_t)(a.piece_cap > 0 ? a.piece_cap : 1),
                                        a.stream);
  if (!rows) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  int64_t total = 0;
  const int rc = captures_all(rows, &total);
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  a.d_groups = rows;
  // rows that do not fit: the kernels run over no row, leave {total, 0} in d_totals and write no byte
  const int rc2 = expand_enqueue(b, n, a, rc == MRX_OK ? total : 0);
  if (rc2 == MRX_OK && rc != MRX_OK)   // (totals == NULL: the host knows this one shortage all the same)
    return internal_fail(MRX_E_CAPACITY, "piece buffers too small: need " + std::to_string(total));
  return rc2;
}

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_expand_spans_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, const int64_t* d_prefix,
                         const int32_t* d_rows, int32_t row_pairs, const char* tpl, size_t tpl_len, int64_t piece_cap,
                         int64_t* d_owner, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                         int64_t* totals, void* stream) {
  return spans_run(csr(d_data, d_offsets), BATCH_CSR, n,
                   ExpandArgs{{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, d_prefix, d_rows, row_pairs,
                              tpl, tpl_len, piece_cap});
}
int mrx_expand_spans_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                                 const int64_t* d_prefix, const int32_t* d_rows, int32_t row_pairs, const char* tpl,
                                 size_t tpl_len, int64_t piece_cap, int64_t* d_owner, int64_t* d_out_offsets,
                                 uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  return spans_run(strided(d_data, stride, d_lens, len), BATCH_PITCH, n,
                   ExpandArgs{{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, d_prefix, d_rows, row_pairs,
                              tpl, tpl_len, piece_cap});
}
int mrx_expand_spans_batch(const uint8_t* data, const int64_t* offsets, int64_t n, const int64_t* prefix, const int32_t* rows,
                           int32_t row_pairs, const char* tpl, size_t tpl_len, int64_t piece_cap, int64_t* owner,
                           int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals) {
  const HostOut o{owner, out_offsets, out_data, totals};
  if (int rc = host_out_check(n, piece_cap, out_cap, offsets, o)) return rc;
  if (row_pairs < 1) return internal_fail(MRX_E_ARGUMENT, "row_pairs must be >= 1");
  if (!tpl && tpl_len > 0) return internal_fail(MRX_E_ARGUMENT, "null template of nonzero length");
  if (!prefix || (n > 0 && prefix[n] > 0 && !rows)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n > 0 && prefix[n] < 0) return internal_fail(MRX_E_ARGUMENT, "prefix[n] must be >= 0");
  DevBatch b; DevOut d; DevBuf<int64_t> pre; DevBuf<int32_t> rw;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  // the kernel reads the rows that fit: the rows buffer holds piece_cap rows at least
  const size_t have = n > 0 ? (size_t)prefix[n] : 0, held = have > (size_t)piece_cap ? have : (size_t)piece_cap;
  if (int rc = pre.alloc((size_t)n + 1)) return rc;
  if (int rc = rw.alloc(held * 2 * (size_t)row_pairs)) return rc;
  if (int rc = d.alloc(piece_cap, out_cap)) return rc;
  MRX_HIP_TRY(hipMemcpy(pre.p, prefix, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice));
  if (have) MRX_HIP_TRY(hipMemcpy(rw.p, rows, sizeof(int32_t) * 2 * (size_t)row_pairs * have, hipMemcpyHostToDevice));
  int64_t tot[2] = {0, 0};
  const int rc = mrx_expand_spans_dev(b.data, b.offsets, n, pre.p, rw.p, row_pairs, tpl, tpl_len, piece_cap, d.ow.p, d.oo.p,
                                      d.od.p, out_cap, d.dt.p, tot, nullptr);
  return d.copy_out(rc, tot, piece_cap, o);
}

int mrx_expand_dev(const mrx_handle* h, const char* tpl, size_t tpl_len, int64_t count, const uint8_t* d_data,
                   const int64_t* d_offsets, int64_t n, int64_t* d_match_prefix, int64_t* d_owner, int64_t* d_out_offsets,
                   int64_t match_cap, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  return expand_run(h, count, csr(d_data, d_offsets), BATCH_CSR, n, d_match_prefix,
                    ExpandArgs{{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, nullptr, nullptr, 1, tpl,
                               tpl_len, match_cap},
                    [&](int32_t* rows, int64_t* total) {
                      return mrx_captures_all_dev(h, d_data, d_offsets, n, count, d_match_prefix, rows, match_cap, total, stream);
                    });
}
int mrx_expand_strided_dev(const mrx_handle* h, const char* tpl, size_t tpl_len, int64_t count, const uint8_t* d_data,
                           int64_t stride, const int32_t* d_lens, int32_t len, int64_t n, int64_t* d_match_prefix,
                           int64_t* d_owner, int64_t* d_out_offsets, int64_t match_cap, uint8_t* d_out_data, int64_t out_cap,
                           int64_t* d_totals, int64_t* totals, void* stream) {
  return expand_run(h, count, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, d_match_prefix,
                    ExpandArgs{{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, nullptr, nullptr, 1, tpl,
                               tpl_len, match_cap},
                    [&](int32_t* rows, int64_t* total) {
                      return mrx_captures_all_strided_dev(h, d_data, stride, d_lens, len, n, count, d_match_prefix, rows,
                                                          match_cap, total, stream);
                    });
}
int mrx_expand_batch(const mrx_handle* h, const char* tpl, size_t tpl_len, int64_t count, const uint8_t* data,
                     const int64_t* offsets, int64_t n, int64_t* match_prefix, int64_t* owner, int64_t* out_offsets,
                     int64_t match_cap, uint8_t* out_data, int64_t out_cap, int64_t* totals) {
  if (!h) return internal_fail(MRX_E_ARGUMENT, "null handle");
  if (count < 0) return internal_fail(MRX_E_ARGUMENT, "count must be >= 0");
  const HostOut o{owner, out_offsets, out_data, totals};
  if (int rc = host_out_check(n, match_cap, out_cap, offsets, o)) return rc;
  if (!tpl && tpl_len > 0) return internal_fail(MRX_E_ARGUMENT, "null template of nonzero length");
  if (!match_prefix) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = captures_all_refusal(h)) return rc;
  DevBatch b; DevOut d; DevBuf<int64_t> pre;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = pre.alloc((size_t)n + 1)) return rc;
  if (int rc = d.alloc(match_cap, out_cap)) return rc;
  int64_t tot[2] = {0, 0};
  const int rc = mrx_expand_dev(h, tpl, tpl_len, count, b.data, b.offsets, n, pre.p, d.ow.p, d.oo.p, match_cap, d.od.p, out_cap,
                                d.dt.p, tot, nullptr);
  if (rc == MRX_OK || rc == MRX_E_CAPACITY)
    MRX_HIP_TRY(hipMemcpy(match_prefix, pre.p, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost));
  return d.copy_out(rc, tot, match_cap, o);
}

void mrx_debug_expand_grid(int workgroups) { g_expand_grid = workgroups > 0 ? workgroups : 0; }

}  // extern "C"
