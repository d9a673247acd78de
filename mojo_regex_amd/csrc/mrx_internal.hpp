// Internal glue between the translation units of libmrx_hip.so (not part of any ABI).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define MRX_HD __host__ __device__ __forceinline__
#else
#define MRX_HD inline
#endif

struct mrx_handle;
struct mrx_set;
namespace mrx {
// records the calling thread's last error message (mrx_last_error()) and returns `code`
int internal_fail(int code, const std::string& msg);

// ---- where the texts of a batch live: the one form that entry points, host code and kernels pass on ------------
// CSR (offsets != nullptr: text i is data[offsets[i], offsets[i + 1])) or fixed pitch (text i begins at data + i * stride
// and is lens[i], or without lens `len`, bytes long).  The kernels' Layout (mrx_core.hpp) begins with these fields.
struct TextBatch {
  const uint8_t* data = nullptr;
  const int64_t* offsets = nullptr;
  int64_t stride = 0;
  const int32_t* lens = nullptr;
  int32_t len = 0;
  MRX_HD const uint8_t* text(int64_t i, int32_t* L) const {   // first byte and length of text i
    if (offsets) {
      const int64_t a = offsets[i];
      *L = (int32_t)(offsets[i + 1] - a);
      return data + a;
    }
    *L = lens ? lens[i] : len;
    return data + i * stride;
  }
  int64_t pitch_longest() const { return lens ? stride : (int64_t)len; }   // fixed pitch: no text is longer
};
inline TextBatch csr(const uint8_t* data, const int64_t* offsets) { return TextBatch{data, offsets, 0, nullptr, 0}; }
inline TextBatch strided(const uint8_t* data, int64_t stride, const int32_t* lens, int32_t len) {
  return TextBatch{data, nullptr, stride, lens, len};
}
// The one check of a caller's batch, MRX_OK or MRX_E_ARGUMENT with the message that the entry point has always
// given: BATCH_CSR refuses null offsets; BATCH_PITCH checks the pitch and the common length of a batch without
// offsets (one with offsets passes), BATCH_PITCH_TERSE (sub and captures_all of one pattern) with one message for
// both.  mrx_findall*_dev, mrx_split_dev and mrx_sub*_dev have never checked their offsets and pass csr() on as it is.
enum BatchForm { BATCH_CSR, BATCH_PITCH, BATCH_PITCH_TERSE };
int check_batch(const TextBatch& b, BatchForm form);

// ---- mrx_stream_bits.hip: findall of short fixed-pitch texts in one launch, events kept in registers ----------
struct DevPlan;
// 0 (default) / 1: MRX_STREAM_BITS=1 in the environment, mrx_debug_stream_bits(1) at run time
int stream_bits_mode();
void stream_bits_set_mode(int on);
void stream_bits_set_trace(int64_t* d_trace);   // measurement: 4 x int64 per 64-text task (nullptr = off)
// can this plan / batch shape take the form? (fixed pitch, 16-byte aligned, texts of at most 1 KiB, a search
// automaton in byte or code columns)
bool stream_bits_eligible(const DevPlan& p, const uint8_t* data, int64_t stride, int64_t max_len, int64_t n);
size_t stream_bits_ctrl_words(int64_t n);   // 8-byte words of look-back state the launch needs (zeroed by it)
size_t stream_bits_args_bytes();            // bytes of device memory for its argument block
// init: zeroes the look-back words and writes the argument block; scan: the one launch.  Both on `stream`.
// d_prefix[n + 1], d_spans[span_cap][2], d_total are the outputs.
int stream_bits_init(int64_t n, int64_t max_len, int64_t* d_prefix, int32_t* d_spans, int64_t span_cap, int64_t* d_total, void* d_ctrl,
                     void* d_args, void* stream);
int stream_bits_scan(const DevPlan& p, const uint8_t* d_blob, const uint8_t* data, int64_t stride, const int32_t* lens,
                     int32_t len, int64_t max_len, int64_t n, const void* d_args, void* stream);

// ---- mrx_set.hip: pattern sets over the handles of their members ----------------------------------------------
struct HostPlan;
const HostPlan& handle_plan(const mrx_handle* h);
// the single-pattern count / search of this handle take the streaming kernel's restart-per-position walk
// (not the anchored automaton) -- what a set may run in its shared pass
bool handle_count_streams(const mrx_handle* h);
bool handle_search_streams(const mrx_handle* h);
// why the handle's count / search would be refused before any work is enqueued ("" = it would run)
std::string handle_refusal(const mrx_handle* h);
// MRX_OK, or the code with which mrx_captures_all_* refuses this handle's pattern (its text in mrx_last_error()):
// host work only, so a call that runs captures_all behind its own checks can refuse before it enqueues anything
int captures_all_refusal(const mrx_handle* h);
void set_last_kernel(const char* name);
// per-call scratch of the calling thread on `stream` (see mrx_release_scratch); a set call opens one scope around
// its own allocations and the single-pattern calls it makes
void scratch_scope_enter(void* stream);
void scratch_scope_leave(void* stream);
// One per API call (entry points nest: sub -> findall, a set -> its members): whatever exit path the outermost call
// takes, bad-argument and HIP-error returns included, its allocations are returned to the arena, so the next call
// reuses the same bytes instead of growing the arena.
struct ScratchScope {
  void* stream;
  explicit ScratchScope(void* st) : stream(st) { scratch_scope_enter(stream); }
  ~ScratchScope() { scratch_scope_leave(stream); }
  ScratchScope(const ScratchScope&) = delete;
  ScratchScope& operator=(const ScratchScope&) = delete;
};
void* scratch_get(size_t bytes, void* stream);   // nullptr: HIP error
// a position in the calling thread's arena on `stream`: a set call rewinds to it behind each member's call (the
// next member's work runs after it on the same stream), so that its scratch does not grow with the set size
struct ScratchMark {
  std::vector<size_t> used;
};
ScratchMark scratch_mark(void* stream);
void scratch_rewind(void* stream, const ScratchMark& m);
// byte count (d_offsets[n]) and longest text of a CSR batch: one small kernel and one stream synchronisation
int batch_bounds(const int64_t* d_offsets, int64_t n, void* stream, int64_t* total, int64_t* max_len);
// exclusive prefix sum of n int64 into d_prefix[n + 1]; *d_total receives the sum
int exclusive_scan(const int64_t* d_in, int64_t n, int64_t* d_prefix, int64_t* d_total, void* stream);
// mrx_count_dev / mrx_findall_known_dev (total == NULL: asynchronous) of one handle on a checked batch;
// known_total / known_max: the CSR batch's bounds (< 0: not known)
int member_count(const mrx_handle* h, const TextBatch& b, int64_t n, int32_t* counts, void* stream, int64_t known_total,
                 int64_t known_max);
int member_findall(const mrx_handle* h, const TextBatch& b, int64_t n, int64_t* d_prefix, int32_t* d_spans,
                   int64_t span_cap, void* stream, int64_t known_total, int64_t known_max);
// mrx_search_dev of one handle on a checked batch (filter), with the CSR batch's bounds as above
int member_search(const mrx_handle* h, const TextBatch& b, int64_t n, int32_t* d_start, int32_t* d_end, void* stream,
                  int64_t known_total, int64_t known_max);
// mrx_set.hip: "member j: reason" if a member's search would be refused ("" = the set's search would run)
std::string set_members_refusal(const mrx_set* s);
// mrx_set_matches_dev on a checked batch (set filter), with the CSR batch's bounds as above
int set_matches(const mrx_set* s, const TextBatch& b, int64_t n, uint64_t* d_bits, void* stream, int64_t known_total,
                int64_t known_max);
// mrx_filter.hip: the tail of filter's compaction on a checked batch, for a caller that has chosen the kept texts
// itself (distinct, take).  d_kept_idx[kept], d_out_offsets[kept + 1] and d_totals = {kept, bytes} are on the
// device, written by work enqueued before; the kept texts' bytes go to d_out_data, by filter's kernels under filter's
// route rule (known_max: a CSR batch's longest text, < 0 = not known), and nothing is written when bytes > out_cap
// or bytes <= 0.  The kernels read d_kept_idx[r] only to find the source of output row r: filter and distinct pass
// ascending indices, take passes them in any order and with repeats.  n bounds kept (take: n is its k, which may
// exceed the batch's text count).  Enqueues only; reports the kernel's name through mrx_last_kernel_name().
int filter_gather_kept(const TextBatch& b, int64_t n, int64_t known_max, const int64_t* d_kept_idx,
                       const int64_t* d_out_offsets, const int64_t* d_totals, uint8_t* d_out_data, int64_t out_cap,
                       void* stream);
// mrx_filter.hip: filter from the flags on, for a caller with a predicate of its own (dictionaries): the two scans, the
// scatter, the gather above and, with a host `totals`, the one read-back and the capacity verdict -- what mrx_filter_*
// runs behind its own flags kernel.  klen[n] (the kept length, 0 for a dropped text) and keep[n] (1 / 0) were written by
// work enqueued before; pos[n + 1] and rank[n + 1] are the scans' outputs.  All four are the caller's scratch.
struct FilterWork {
  int64_t* klen;
  int64_t* keep;
  int64_t* pos;
  int64_t* rank;
};
// Where a byte mover leaves its packed CSR batch, as the contracts of include/mrx.h have it: the one destination of
// filter, extract, expand, format, take, distinct and the dictionaries' filter.  The argument structs of those calls
// begin with it; what it ends in on the host (the n == 0 result, the read-back and the capacity verdict) is in
// mrx_host_batch.hpp.
struct PackedDest {
  int64_t* d_rows;          // an index per output row: filter's kept_idx, extract's and expand's owner, distinct's first
                            // (format and take have none: nullptr)
  int64_t* d_out_offsets;   // [rows + 1]
  uint8_t* d_out_data;
  int64_t out_cap;
  int64_t* d_totals;        // {rows, bytes} on the device
  int64_t* totals;          // ... and on the host, or nullptr: the call only enqueues
  void* stream;
};
int filter_compact(const TextBatch& b, int64_t n, int64_t known_max, const FilterWork& w, const PackedDest& a);
int filter_no_text(const TextBatch& b, int64_t known_max, const PackedDest& a);   // the n == 0 result, and the kernel's name
// mrx_distinct.hip: distinct's first three steps on a checked batch of n >= 1 texts, for a caller that keeps the table
// (dictionaries): k_distinct_hash, k_distinct_insert and k_distinct_first, launched as distinct launches them.  `table`
// (`slots` words, a power of two >= 2 n) and count_at[n] are zero, first_at[n] is all ones and *err is 0 when the
// work runs; hash[n] and rep_of[n] are outputs.  mask: what the hash is and-ed with (distinct_hash_mask()).
struct DistinctGroups {
  uint64_t* hash;
  unsigned long long* table;
  uint64_t slots;
  int32_t* rep_of;
  unsigned long long* first_at;
  unsigned long long* count_at;
  int32_t* err;
};
int distinct_groups(const TextBatch& b, int64_t n, uint64_t mask, const DistinctGroups& g, void* stream);
uint64_t distinct_hash_mask();                        // mrx_debug_distinct_hash_mask(): all ones unless a test set it
unsigned distinct_grid(int64_t items, int64_t per);   // workgroups for `items` at `per` a workgroup, capped by the hook
// mrx_sort.hip: mrx_sort_dev on a batch in either form, for a caller that keeps the order (the sorted index): d_order[n]
// and d_totals[1] = {different texts}; known_max: the longest text (< 0 = not known).  Checks its arguments as
// mrx_sort_dev does and synchronises once per round.
int sort_order_of(const TextBatch& b, BatchForm form, int64_t n, int64_t known_max, int64_t* d_order, int64_t* d_totals,
                  void* stream);
// the scan timer of mrx_timing_scan_ms around a launch sequence: begin returns a token for end
void* scan_timer_begin(void* stream);
void scan_timer_end(void* token);
}  // namespace mrx
