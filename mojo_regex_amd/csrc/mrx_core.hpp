// The core of libmrx_hip.so as a HIP unit sees it (.hip files only): where the texts of a batch live for a kernel
// (Layout), the handle, and the host functions of mrx_kernels.hip that launch the regex kernels on a handle.  What is
// declared here is defined in mrx_kernels.hip, once: its thread_local state (last error, last kernel, scratch arena,
// timing counters, current device) is reached through these functions and never defined a second time.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>

#include "../../include/mrx.h"
#include "mrx_device.hpp"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"

namespace mrx {

constexpr int kBlock = 256;  // 4 wavefronts

struct Layout : TextBatch {  // where text i lives (TextBatch: data, offsets, stride, lens, len), and what kernels add
  Layout() = default;
  Layout(const TextBatch& b) : TextBatch(b) {}
  // Stepper kernels only (ragged batches with a few very long texts): k_wstep leaves texts of at least
  // `split` bytes to k_req_wave, which in turn skips the shorter ones; 0 = no split
  int32_t split = 0;
  // k_wstep / k_req_wave<STEP_SLOTS / STEP_EMIT> and k_slots_gather_wide: slot rows sized by the text
  // (len / 4 + 32 spans, see slot_row()) instead of kStepSlots, so that long texts rarely need the second walk
  int32_t wide_slots = 0;
  // Views (the `start` argument, mrx_*_at_*): with offsets != nullptr, text i is the vlen[i] bytes at
  // data + offsets[i] (offsets need not be contiguous); nullptr = plain CSR
  const int32_t* vlen = nullptr;
  const uint32_t* vskip = nullptr;   // with vlen: the per-text word k_stream_findall's VIRT form expects
  // k_mwalk<STEP_SLOTS / STEP_EMIT> only: text i is a piece of a longer text and its spans are reported as positions
  // of that text, vbase[i] + position in the piece (FindallJob::step_scan's pieces); nullptr = as found
  const int32_t* vbase = nullptr;
  // per text: first occurrence of the backtracking matcher's literal, last occurrence << 1 | has-newline
  // (k_litscan in front of the lane-per-text kernels, see bt_prepass()); nullptr = not computed
  const int2* pre = nullptr;
  // marks of the positions at which a match begins (k_backscan -> k_wstep<., 0, 0, 0, 1>): one bit per byte of the
  // text's FRAME (the 16-byte blocks that hold it: bit f = frame position f, the text begins at f = address & 15),
  // text i's words from bm_row(i) on -- a multiple of four, so that the four words of a 128-byte window are one
  // aligned 16-byte load; bm_cnt[i] = how many marks text i has
  const uint32_t* bm = nullptr;
  const int32_t* bm_cnt = nullptr;
  __host__ __device__ __forceinline__ int64_t bm_row(int64_t i) const {
    return 4 * (offsets ? (offsets[i] >> 7) + 2 * i : i * ((stride >> 7) + 2));
  }
  // first slot of text i's row and the row's capacity (wide rows)
  __device__ __forceinline__ int64_t slot_row(int64_t i, int* cap) const {
    if (offsets) {
      const int64_t a = (offsets[i] >> 2) + 32 * i, b = (offsets[i + 1] >> 2) + 32 * (i + 1);
      *cap = (int)(b - a);
      return a;
    }
    const int64_t row = (int64_t)((lens ? stride : (int64_t)len) >> 2) + 32;
    *cap = (int)row;
    return i * row;
  }
  __device__ __forceinline__ Text text(int64_t i) const {
    Text t = offsets ? Text(data + offsets[i], vlen ? vlen[i] : (int)(offsets[i + 1] - offsets[i]))
                     : Text(data + i * stride, lens ? lens[i] : len);
    if (pre) { const int2 v = pre[i]; t.pre_first = v.x; t.pre_last_nl = v.y; }
    return t;
  }
};
// every kernel's argument block holds a Layout: its size and field offsets are part of the device code
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(sizeof(Layout) == 96 && offsetof(Layout, data) == 0 && offsetof(Layout, len) == 32 &&
                  offsetof(Layout, split) == 36 && offsetof(Layout, bm_cnt) == 88,
              "Layout must keep its layout");
#pragma clang diagnostic pop

__device__ __forceinline__ Ctx stage_tables(const DevPlan& p, const uint8_t* __restrict__ blob,
                                            uint8_t* lds) {
  // cooperative 4-byte copy of the plan blob into LDS
  const uint32_t* src = (const uint32_t*)blob;
  uint32_t* dst = (uint32_t*)lds;
  const int words = p.blob_bytes >> 2;
  for (int i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
  __syncthreads();
  Ctx c;
  c.p = p;
  c.cls = lds + p.off_cls;
  c.first = lds + p.off_first;
  c.trans = (const uint16_t*)(lds + p.off_trans);
  c.lit = lds + p.off_lit;
  c.pre = lds + p.off_pre;
  c.bs_cls = lds + p.off_bs_cls;
  c.bs_mask = (const uint64_t*)(lds + p.off_bs_mask);
  c.bs_follow = (const uint64_t*)(lds + p.off_bs_follow);
  c.bt_items = (const BtItem*)(lds + (p.off_bt_items >= 0 ? p.off_bt_items : 0));
  c.bt_tbl = lds + (p.off_bt_tbl >= 0 ? p.off_bt_tbl : 0);
  c.bt_lit = lds + (p.off_bt_lit >= 0 ? p.off_bt_lit : 0);
  return c;
}
}  // namespace mrx

// The compiled tables live once per device that has used the handle (uploaded on first use there,
// never freed or replaced before mrx_free): concurrent calls on one handle from threads bound to
// different GPUs each see their own device's copy.
constexpr int kMaxDevices = 64;
struct mrx_handle {
  mrx::HostPlan hp;
  std::atomic<uint8_t*> d_blobs[kMaxDevices];
  std::mutex mu;   // serialises the first upload per device
  std::string describe_cache;
  // sub: matches per KiB of input the last batch held (0 = nothing seen yet): sizes the span buffer of the next
  // call so that a dense batch (more than one match per eight bytes) does not scan twice every time
  mutable std::atomic<int64_t> sub_matches_per_kib{0};
  // findall of a required-byte plan on long texts: the wavefront-per-text kernel or pieces on the multi-walk kernel?
  // Neither candidate density nor batch shape predicts it (profiles/r04_suite_routes.md), so the first two calls of a
  // batch shape try each route (see ReqTune) and the faster one is kept.
  // Four measured calls per batch shape: each route once untimed (its scratch gets allocated), then each route timed --
  // two HIP events on the caller's stream around the call's work, read by a LATER call of the shape once the last pair
  // has completed: no call ever waits for the tuner, and callers that enqueue back to back are served as well.
  struct ReqTune {
    int issued = 0, choice = 0;   // calls measured so far (0..4); choice: 1 wavefront kernel, 2 pieces
    bool probed = false;
    float ms_wave = 0, ms_pieces = 0;
    hipEvent_t ev[4][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    int dev = 0;                  // device the events belong to (part of the key)
  };
  mutable std::mutex tune_mu;
  mutable std::map<uint32_t, ReqTune> req_tune;
  // findall on texts FULL of matches (config 5: a match every six bytes): event rows instead of records (ST_ROWS,
  // k_decode_rows).  How full a batch is, the handle's previous eligible call tells: its total travels to pinned host
  // memory behind the call's work and is looked at by the next call if it has arrived -- no call waits for it.
  struct DenseProbe {
    int64_t* host_total = nullptr;   // pinned
    hipEvent_t ev = nullptr;
    bool pending = false;
    int64_t bytes = 0;               // of the batch the pending total belongs to
    int dev = 0, dense = 0;          // dense: 1 = the last batch seen held at least one match per kDenseBytesPerSpan bytes
  };
  mutable DenseProbe dense_probe;    // (under tune_mu)
  mrx_handle() { for (auto& b : d_blobs) b.store(nullptr, std::memory_order_relaxed); }
};

namespace mrx {
// ---- host side: mrx_kernels.hip ----------------------------------------------------------------------------------
// the calling thread's current device (set by ensure_device() at the start of every entry point); H_BLOB(h) is the
// handle's table copy on that device
int current_device();
#define H_BLOB(h) ((h)->d_blobs[mrx::current_device()].load(std::memory_order_acquire))
int ensure_device(const mrx_handle* h);
int check_lds(const mrx_handle* h);
int check_search_supported(const mrx_handle* h);
size_t lds_for(const mrx_handle* h);
int grid_cap();                           // workgroups that fill the current device: 8 per CU
int device_grid(int64_t n, int block);    // workgroups of `block` lanes for n items: at least one, at most grid_cap()
int force_generic();    // mrx_debug_force_generic()'s level
int long_text_mode();   // mrx_debug_long_text_kernels()'s mode
// the measurement knobs that sub's kernels read from the environment, once
struct EnvKnobs {
  int decode_grid, decode_reverse, piece_c, fused_skew, fused_debug;
  int subc_debug;   // k_subc_sizes / k_subc_emit with phases left out (timing only): 1 no walk, 2 no bitmaps, 4 no per-match store; 8 no gap copies, 32 no replacement bytes, 64 no stores
  int subs_debug;   // k_subs_wave with phases left out (timing only, the output is wrong): 1 replacement bytes, 2 kept bytes, 4 stores, 8 frame phase, 16 match phase
  bool piece_c_set;
};
int env_int(const char* name, int dflt);
const EnvKnobs& env_knobs();
// byte count and longest text of a CSR batch: both live on the device (one small kernel, one sync)
int csr_stats(const Layout& lay, int64_t n, hipStream_t s, int64_t* total, int64_t* max_len);
// the literal prefilter in front of the lane-per-text kernels: *out is `lay` with Layout::pre filled in where it pays
int bt_prepass(const mrx_handle* h, const Layout& lay, int64_t n, hipStream_t s, Layout* out);
int run_findall(const mrx_handle* h, const Layout& lay, int64_t n, int64_t* d_prefix, int32_t* d_spans, int64_t span_cap,
                int64_t* total, void* stream, bool match_next_sequence = false, int64_t known_total = -1, int64_t known_max = -1);
// exclusive scan of n counts (int32_t or int64_t) into prefix[n + 1]; *d_total receives the sum
template <class T>
int device_scan(const T* d_in, int64_t n, int64_t* d_prefix, int64_t* d_total, hipStream_t s);
// A phase that began with nothing in use (the head of a call) hands its bytes to what follows: the next phase
// allocates where it lay.  Further inside a call -- something is held at the mark -- the bytes stay until the scope
// closes, so that what follows lies where it always lay.
void scratch_reuse_from(hipStream_t s, const ScratchMark& m);
// scratch_get() into P, or the call returns with the text that this allocation's failure has always had
#define MRX_SCRATCH(P, BYTES, S)                                                                                \
  do {                                                                                                          \
    if (!((P) = (decltype(P))mrx::scratch_get((BYTES), (S))))                                                   \
      return mrx::internal_fail(MRX_E_NO_DEVICE, std::string("scratch_alloc((void**)&" #P ", " #BYTES ", " #S "): ") + \
                                                     hipGetErrorString(hipGetLastError()));                     \
  } while (0)
struct ScanTimer {  // HIP events around the dominant scan kernel, on its own stream (mrx_timing_scan_ms)
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t s;
  bool on;
  explicit ScanTimer(hipStream_t st, bool enable = true);
  void stop();
};

// plans with a backtracker route take the kernel instantiations that carry its interpreter (k_match<., true> ...)
inline bool plan_uses_backtracker(const mrx_handle* h) {
  return (h->hp.dev.flags & (PF_BT_FIRST | PF_BT_SEARCH)) != 0 && h->hp.dev.bt_nitems > 0;
}
// ... 2: the lean instantiation for deterministic chains (DevPlan::bt_flags bit 5: no choice stack), 1: the full one
inline int bt_kernel_kind(const mrx_handle* h, bool wanted) {
  static const bool full_only = getenv("MRX_BT_FULL") && getenv("MRX_BT_FULL")[0] == '1';   // A/B: chains on the full interpreter
  if (!wanted) return 0;
  return ((h->hp.dev.bt_flags & 32) && !full_only) ? 2 : 1;
}
#define MRX_BT_DISPATCH(KIND, LAUNCH)        \
  do {                                       \
    if ((KIND) == 2) { LAUNCH(2); }          \
    else if ((KIND) == 1) { LAUNCH(1); }     \
    else { LAUNCH(0); }                      \
  } while (0)

// ---- mrx_sub.hip -------------------------------------------------------------------------------------------------
// what a spans route returns when the batch is the lane-per-text kernels' after all (sub and captures_all)
constexpr int kSubsRetryGeneric = 1 << 20;
// Rows at a fixed pitch without padding (no per-text lengths, len == stride) are a CSR batch whose offsets are
// i * stride: written once on the device into the caller's scratch scope, so that the call takes every route of a
// CSR batch, with the batch's bounds known (n * stride bytes, no text longer than stride).
inline bool rows_unpadded(const TextBatch& b, int64_t n) { return !b.lens && (int64_t)b.len == b.stride && n > 0; }
int rows_as_csr(const TextBatch& b, int64_t n, void* st, TextBatch* out);
// the refusal of \1..\9 on a pattern that has neither the fixed-width form nor the flat backtracking program
// (sub with a group template, captures_all); MRX_OK when the pattern has one
int group_template_refusal(const mrx_handle* h);

// ---- mrx_capall.hip ----------------------------------------------------------------------------------------------
const char* capall_route_name(const mrx_handle* h);   // mrx_describe()'s device.capall: "chain", "fixed" or "general"
}  // namespace mrx
