/*
 * mrx_testing.h -- measurement and testing hooks of libmrx_hip.so.
 *
 * NOT part of the drop-in boundary (include/mrx.h): nothing here corresponds to a reference
 * interface.  bench.py uses the timing hooks for the roofline object; the parity tests use the
 * debug switches to run one batch through two kernel families and compare them text by text.
 * The switches are process-wide; set them while no call is in flight.
 */
#ifndef MRX_TESTING_H
#define MRX_TESTING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Average duration (ms) of the dominant scan kernel over the launches made by
 * this thread since the last reset, measured with HIP events on the launch
 * stream; launches = number of scan-kernel launches measured. */
void mrx_timing_reset(void);
void mrx_timing_enable(int on);
double mrx_timing_scan_ms(int64_t* launches);
const char* mrx_last_kernel_name(void);
/* Testing aid: route every call to the generic lane-per-text kernels (the streaming kernel is
 * then never used) so that the two implementations can be compared on the same batch. */
void mrx_debug_force_generic(int on);
/* Testing aid: the treatments of long texts (pieces cut at synchronising bytes, a wavefront per text) are chosen by
 * the batch's average text length; 1 = always use them (pieces of 200 bytes where the plan has synchronising bytes),
 * 2 = never, 3 = as 1 but stepper plans take the wavefront-per-text kernel instead of pieces, 0 = by length. */
void mrx_debug_long_text_kernels(int mode);
/* findall of streamable plans runs as three launches (scan -> prefix sums -> decode; the default, and
 * the faster form as measured) or as ONE (scan, CSR offsets by decoupled look-back and spans fused);
 * same results either way.  0 = three launches, 1 = one launch when a 64-text task has at least
 * 32 KiB, 2 = one launch for short texts too.  Environment: MRX_FUSED=0|1|2 at compile time. */
void mrx_debug_fused_findall(int mode);
/* 1: findall of streamable plans over fixed-pitch texts of at most 1 KiB (16-byte aligned pitch, search automaton in
 * byte or code columns) runs as ONE launch that keeps every text's event bits in registers and writes offsets and
 * spans at their final place (k_stream_bits: no record stream, 1.27 GB of traffic instead of 1.74 GB on the headline
 * batch).  0 (default) = scan -> prefix sums -> decode: the one launch measured 4 % slower on 1 KiB texts and 1.5-3 x
 * slower on shorter ones (profiles/r04_stream_bits.md: its expansion costs as many VALU instructions as the scan).
 * Same results.  Environment: MRX_STREAM_BITS=1. */
void mrx_debug_stream_bits(int on);
/* Measurement: k_stream_bits writes four device clock readings (10 ns ticks) per 64-text task into d_trace
 * [4 * tasks]: task taken, texts walked and count published, count of all texts before known, spans written.
 * NULL = off (default). */
void mrx_debug_stream_bits_trace(int64_t* d_trace);
/* Ragged (CSR) batches of streamable plans with a reset byte are scanned by k_stream_dyn -- 256-text tasks,
 * a lane takes the next text when its own ends -- from 16384 texts up; 1 = always, 2 = never, 0 = by size. */
void mrx_debug_dynamic_texts(int mode);
/* 1: findall of a fixed-pitch batch of 2^18 texts and more runs as two halves on two streams (the decode of the
 * first under the scan of the second); 0 (default: the split measured slower) = one batch, three launches on the
 * caller's stream.  Results are the same. */
void mrx_debug_split_findall(int on);
/* findall of a batch full of matches by event rows (k_stream_findall<ST_ROWS> + k_decode_rows; texts of 2 KiB and more at
 * an aligned fixed pitch, common length a multiple of 128): 0 = when the handle's previous call found one match per 20
 * bytes or more (default), 1 = whenever the batch has the shape, 2 = never */
void mrx_debug_dense_rows(int mode);
/* PF_MW_TRIES plans: 1 = always the pending-tries walk; 0 (default) = the handle times it against
 * marks + stepper on the first calls of a batch shape (256 texts and more) and keeps the faster route. */
void mrx_debug_tries_always(int on);
/* regex.sub with \\1..\\9 on a deterministic chain: 1 = always measure every match's replacement
 * (k_subc_sizes), 0 (default) = templates under which every match gains the same number of bytes skip that pass. */
void mrx_debug_chain_sub_general(int on);
/* Host-side run of the one-pass table of an empty-match plan whose walks read beyond their match (build_emptywalk2(),
 * mrx_plan.cpp): findall of ONE text on the CPU, for tests that pin the table to the oracle without a GPU.  Returns the
 * number of spans (spans[2 k], spans[2 k + 1] for k < min(count, cap)), -1 when the handle has no such table. */
int mrx_testing_emptywalk_findall(const mrx_handle* h, const uint8_t* text, int len, int32_t* spans, int cap);
/* sub assembled from findall spans: lanes that share one text in k_subs_wave (16, 32 or 64; texts whose
 * frame or output exceed the group's LDS tiles go to k_subs_emit); 0 = k_subs_emit for every text,
 * anything else = chosen from the average text length. */
void mrx_debug_subs_group(int lanes);
/* The backtracking matcher's literal pass (k_litscan): 0 = one lane per text, 1 = always in pieces (208 bytes, so
 * that short test texts are cut, at positions that are not multiples of 16), anything else = in 2 KiB pieces
 * when the batch has few texts.  Results are the same. */
void mrx_debug_litscan_pieces(int mode);
/* Stepper plans with a multi-walk table (several walks side by side in one pass, k_mwalk; `multiwalk=yes` in
 * mrx_describe) use it for findall / count / search; 2 = never (the windowed stepper's restart-per-position loop
 * instead; also no backward marks and no fixed-length form of the bitset union pass), 3 = the multi-walk kernel
 * without its packed-start form (starts as 16-bit halves moved by byte permutes, texts below 64 KiB), anything else
 * = where the plan has one.  Results are the same. */
void mrx_debug_multiwalk(int mode);
/* Placement experiments (profiles/r03_scan_forms.md): the streaming findall's record stream begins `bytes` (a multiple
 * of 16) behind the start of its scratch allocation.  Results are the same. */
void mrx_debug_rec_skew(int64_t bytes);
/* The three-launch findall of texts of at most 1 KiB at a 16-byte aligned fixed pitch (no offsets, no rows / bits /
 * fused / dynamic / split / pieces form) writes its event records in 12 bytes instead of 16: {F of the even group, F of
 * the odd group, start | before << 10 | pair << 20 | lane << 26} (csrc/mrx_rec12.hpp).  0 = never (16-byte records
 * everywhere), anything else = by that rule (default).  Results are the same.  Environment: MRX_REC12=0. */
void mrx_debug_rec12(int mode);
/* The packing of that record's third word on the host, for tests without a GPU: packs the four fields and writes what
 * the extractors give back to out = {start, pair, lane, before}.  Returns 0, or -1 when a field is out of range
 * (start 0..1023, pair 0..32, lane 0..63, before 0..1023) or out is NULL. */
int mrx_testing_rec12_roundtrip(int start, int pair, int lane, int before, int32_t out[4]);
/* k_decode's lean pass (csrc/mrx_decode_bits.hpp): wavefronts of the streaming findall's two-word records (12 or 16
 * bytes; not the dynamic, split, pieces or fused forms) whose spans fit one LDS tile expand their records without a
 * per-span bounds test, with the fixed-length form chosen per wavefront, the start as a max and record loads that do
 * not branch.  0 = the general tile loop everywhere (k_decode<..., false> in a kernel trace), anything else = the lean
 * pass (k_decode<..., true>; default).  Results are the same.  Environment: MRX_DECODE_LEAN=0. */
void mrx_debug_decode_lean(int mode);
/* Which form the last k_decode launch of the streaming findall took: 1 = the lean instantiation, 0 = the general one
 * (switch off, or a form the lean pass does not cover: dynamic tasks, 32-bit positions, one-word records), -1 = no such
 * launch yet.  Process-wide, like mrx_last_kernel_name. */
int mrx_debug_last_decode_lean(void);
/* That expansion on the host, for tests without a GPU.  Record i of n is {f_even[i], f_odd[i]}, the event words of the
 * even and the odd group of the pair at text position pb[i]; start[i] = start of the walk alive at the pair's first byte;
 * fixed_len > 0 = every match is that long.  Writes the record's number of spans (at most 32) to counts[i] and their
 * (start, end), in text order, to spans[64 i ...] (room for 32 spans a record).  Returns 0, or -1 when n or fixed_len is
 * negative or an array is NULL. */
int mrx_testing_decode_expand(int64_t n, const uint32_t* f_even, const uint32_t* f_odd, const int32_t* start, const int32_t* pb,
                              int fixed_len, int32_t* counts, int32_t* spans);
/* k_decode's tile store loops (the lean pass and the multi-pass loop of every record, slot and task form; not the dense
 * row windows, not k_decode_rows): 0 = one span per lane and trip, an 8-byte store each (k_decode<..., false> in a kernel
 * trace), anything else = two spans per lane and trip in one 16-byte store, single spans only at the ends of a
 * wavefront's range (k_decode<..., true>; default).  Results are the same.  Environment: MRX_DECODE_STORE16=0. */
void mrx_debug_decode_store16(int mode);
/* Which of the two the last k_decode launch took (the streaming findall, its split and pieces forms): 1 = 16-byte
 * stores, 0 = 8-byte stores (switch off, or k_decode_rows ran instead), -1 = no such launch yet.  Process-wide. */
int mrx_debug_last_decode_store16(void);
/* The index arithmetic of the 16-byte form on the host (decode_store_plan, csrc/mrx_decode_bits.hpp), for tests without
 * a GPU.  A wavefront's nspan spans are the span indices pre0 .. pre0 + nspan - 1 of a buffer whose address / 8 has
 * parity addr_parity; span_cap = capacity of the buffer in spans.  out = {odd, head, npairs, tail, nclip}: span k sits
 * at tile slot k + odd; nclip spans leave -- span 0 alone when head, then npairs pairs from span `head` on, then one
 * more span alone when tail.  Returns 0, or -1 when nspan is negative, addr_parity is not 0 or 1, or out is NULL. */
int mrx_testing_decode_store_plan(int64_t pre0, int addr_parity, int nspan, int64_t span_cap, int32_t out[5]);
/* include/mrx_comm.h, padded form of mrx_allgatherv_spans: its two device steps on buffers the caller fills as
 * ncclAllGather would have, so that the multi-rank arithmetic can be checked on one GPU.
 * meta_all: meta_stride int64 words per rank -- 2: {texts, spans}; 4: {texts (-1: that rank's arguments were invalid),
 * spans, capacity of that rank's global offsets buffer, of its global spans buffer}, the words the library gathers.
 * shift: out[i] = prefix[i + 1] + (spans of the ranks before `rank`) for i < n_local, 0 up to pad_to.
 * compact: stage_prefix[r][P], stage_spans[r][cap][2] -> global CSR; *d_status = MRX_OK, MRX_E_CAPACITY (some rank's
 * capacities, or these, do not hold the result: nothing is written) or MRX_E_ARGUMENT (some rank was invalid). */
int mrx_testing_comm_shift(const int64_t* d_prefix, int64_t n_local, const int64_t* d_meta_all, int meta_stride, int rank,
                           int64_t* d_out, int64_t pad_to, void* stream);
int mrx_testing_comm_compact(const int64_t* d_meta_all, int meta_stride, int nranks, const int64_t* d_stage_prefix, int64_t P,
                             const int32_t* d_stage_spans, int64_t cap, int64_t* d_gprefix, int64_t gprefix_cap,
                             int32_t* d_gspans, int64_t gspans_cap, int32_t* d_status, void* stream);
/* Pattern sets (include/mrx.h): 0 = the route rule (the members' own calls: measured faster at every set size), 1 = the
 * shared pass for every member that is eligible whatever the
 * batch shape, 2 = every member through its own single-pattern call.  Results are the same. */
void mrx_debug_set_route(int mode);
/* The packed tables of a set walked on the CPU over ONE text, as the shared-pass kernel walks them, for tests that pin
 * the packing to the oracle without a GPU.  op: 0 count (out[k]), 1 search (out[2 k]: start, end), 2 matches (out[k]:
 * 0 / 1).  Members outside the shared pass of that operation get -2. */
struct mrx_set;
int mrx_testing_set_run(const struct mrx_set* s, int op, const uint8_t* text, int len, int32_t* out);
/* Filter (include/mrx.h): which kernel moves the kept bytes.  0 = the rule (k_filter_gather_text, 16 lanes per kept
 * text, when the host knows the batch's longest text and it is at most 4 KiB; k_filter_gather, a lane per 16-byte
 * output block, otherwise: profiles/filter.md), 1 = the block form always, 16 = the text form always.  Results are
 * the same. */
void mrx_debug_filter_form(int form);
/* Extract (include/mrx.h): the byte mover reports itself as "k_extract_gather" through mrx_last_kernel_name().  Its grid
 * is sized by out_cap, a wavefront per 1 KiB at least; `workgroups` > 0 caps it (4 wavefronts each), so that a test makes
 * one wavefront run several rounds of 64 blocks without an output of many megabytes.  0 (default) = no cap.  Results are
 * the same. */
void mrx_debug_extract_grid(int workgroups);
/* Expand (include/mrx.h): the byte mover reports itself as "k_expand_gather"; its grid is sized and capped as extract's
 * (mrx_debug_extract_grid), by a switch of its own.  0 (default) = no cap.  Results are the same. */
void mrx_debug_expand_grid(int workgroups);
/* Distinct (include/mrx.h): `mask` is and-ed onto every text's hash before the table sees it; all ones (default) = the
 * hash as it is.  0 puts every text into one probe chain with equal tags, so that every decision is a byte comparison
 * (the probe is then quadratic: keep n small); 3 gives four chains.  Results are the same.
 * Dictionaries (include/mrx.h) hash as distinct does, so the mask applies to them: the mask in force when
 * mrx_dict_build_* runs is stored in the handle and used by every lookup and filter on it, whatever the hook says by
 * then.  Changing the hook later cannot separate a handle from its own table; it takes effect for the next build. */
void mrx_debug_distinct_hash_mask(uint64_t mask);
/* Distinct: `workgroups` > 0 caps the grids of its own kernels (4 wavefronts each), so that a test makes one wavefront
 * run several rounds without a batch of millions of texts.  0 (default) = no cap.  Results are the same.  The cap also
 * holds for a dictionary's build and for its lookup kernel, "k_dict_lookup" in mrx_last_kernel_name(). */
void mrx_debug_distinct_grid(int workgroups);
/* Sort (include/mrx.h): a group of 2 to `max` positions whose texts agree so far is finished at once by comparing its
 * members with each other (k_sort_small); larger ones go through another radix round.  64 is the default and the
 * largest value (a negative or larger argument restores it); 0 sends every group through radix rounds, one per 8 bytes
 * that its texts share: keep shared prefixes short then.  Results are the same.  Sort reports "k_sort_small" through
 * mrx_last_kernel_name(), take the byte mover of filter that it ran. */
void mrx_debug_sort_small(int max);
/* Sort and take: `workgroups` > 0 caps the grids of their own kernels (4 wavefronts each), so that a test makes one
 * wavefront run several tiles of a radix pass without a batch of millions of texts.  0 (default) = no cap.  Results
 * are the same. */
void mrx_debug_sort_grid(int workgroups);
/* Sort: the number of 8-byte refinement rounds, each with one synchronisation of the stream, that the calling thread's
 * last sort call took (0 for a batch without texts, and before any call). */
int mrx_debug_sort_rounds(void);
/* Sorted index (include/mrx.h): `workgroups` > 0 caps the grids of its kernels (4 wavefronts each), so that a test makes
 * a lane search several probes, a grid's stride apart, without a batch of millions of texts.  0 (default) = no cap.  The
 * search reports itself as "k_sorted_search" through mrx_last_kernel_name().  Results are the same. */
void mrx_debug_sorted_grid(int workgroups);
/* Sorted index: which search aids every later search uses, as a mask: 1 = the key array (the entries' first words are
 * searched with 8-byte loads before any entry's bytes), 2 = the fence posts in LDS above it (they need the keys: 2 alone
 * is 0).  0 = the plain binary search over the entries' bytes.  -1 restores the default, any other negative value changes
 * nothing.  Returns the mask in force.  A handle holds both aids whatever the mask was at its build.  Results are the
 * same (profiles/sorted.md has the times). */
int mrx_debug_sorted_aids(int mask);
/* Numbers (include/mrx.h): the one kernel reports itself as "k_parse" through mrx_last_kernel_name().  Its grid is a
 * lane per row, capped as extract's; `workgroups` > 0 caps it further (4 wavefronts each), so that a test makes one
 * wavefront run several rounds of 64 rows without millions of them.  0 (default) = no cap of its own.  Results are the
 * same. */
void mrx_debug_parse_grid(int workgroups);
/* Format (include/mrx.h): the byte mover reports itself as "k_format_gather"; its grid is sized and capped as expand's
 * (mrx_debug_expand_grid), and the sizes kernel's, a lane per row, likewise, both by this switch of their own.  0
 * (default) = no cap.  Results are the same. */
void mrx_debug_format_grid(int workgroups);
/* The per-cell formatter of a number column on the CPU, for tests that pin it to Python's % without a GPU: kind and arg
 * as in mrx_column, value_word the int64 or the bits of the double.  Writes the cell to out and returns its length (at
 * most 21), or minus the status (-MRX_NUM_RANGE: the cell is not answered; -MRX_NUM_MALFORMED: MRX_COL_TEXT, a kind or
 * an arg that mrx_format_dev refuses, or a null out). */
int mrx_testing_format_one(int32_t kind, int32_t arg, int64_t value_word, uint8_t out[32]);
/* Keywords (include/mrx.h): the piece size P of every later call is `bytes` (> 0; 16 and 32 cut short test texts into
 * several pieces with entries longer than two of them); 0 (default) = the rule that the contract states.  The pass
 * reports itself as "k_kw_count" or "k_kw_emit" through mrx_last_kernel_name().  Results are the same. */
void mrx_debug_kw_piece(int64_t bytes);
/* Keywords: 0 = every row of the table is read from global memory, anything else (default) = the rows of the shallowest
 * states, as many as fit 32 KiB, are kept in LDS beside the class map.  Results are the same. */
void mrx_debug_kw_tier(int on);
/* Keywords on the CPU, for tests without a GPU: the automaton is built from the entries (entry j = entry_data[
 * entry_offsets[j], entry_offsets[j + 1]), flags as mrx_kw_build) and the walk of the kernels runs over the same pieces
 * (the pinned size, else the rule), one after the other, on the texts data[offsets[i], offsets[i + 1]).  Outputs as
 * mrx_kw_findall_batch: text_prefix int64[n + 1], entries int32[span_cap], spans int32[span_cap][2], *total (may be
 * NULL).  describe (may be NULL) receives at most describe_cap bytes of what mrx_kw_describe would print.  Returns
 * MRX_OK, MRX_E_CAPACITY (the prefix and *total are valid) or the build's error. */
int mrx_debug_kw_host_findall(const uint8_t* entry_data, const int64_t* entry_offsets, int64_t m, uint32_t flags,
                              const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* text_prefix, int32_t* entries,
                              int32_t* spans, int64_t span_cap, int64_t* total, char* describe, size_t describe_cap);
/* Keywords, leftmost and sub on the CPU, for tests without a GPU: the automaton of the reversed entries is built as the
 * handle builds it, and the walk back, the selection, the rows and the block fill of the kernels run over the same pieces
 * (the pinned size of mrx_debug_kw_piece, else the rule), one after the other.  Entries and texts as
 * mrx_debug_kw_host_findall; outputs, capacity rules and return codes as mrx_kw_leftmost_batch and mrx_kw_sub_batch, the
 * replacements on the host too.  On the device the operations report themselves as "k_kw_sub_select" and
 * "k_kw_sub_gather" through mrx_last_kernel_name(). */
int mrx_debug_kw_host_leftmost(const uint8_t* entry_data, const int64_t* entry_offsets, int64_t m, uint32_t flags, int64_t count,
                               const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* text_prefix, int32_t* entries,
                               int32_t* spans, int64_t span_cap, int64_t* total);
int mrx_debug_kw_host_sub(const uint8_t* entry_data, const int64_t* entry_offsets, int64_t m, uint32_t flags,
                          const uint8_t* repl_data, const int64_t* repl_offsets, int64_t r, int64_t count, const uint8_t* data,
                          const int64_t* offsets, int64_t n, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap,
                          int32_t* nsub, int64_t* totals);
/* Lines (include/mrx.h): bytes > 0 pins the piece size P of every later call (rounded up to a multiple of 1024, a
 * wavefront's round), 0 restores the default, a negative value changes nothing.  Returns the P in force: tests place
 * their separators by it.  The pass reports itself as "k_lines_emit" through mrx_last_kernel_name().  Results are the
 * same. */
int64_t mrx_debug_lines_piece(int64_t bytes);
/* How often mrx_lines_* has synchronised with the device on this process so far: the CSR form's read-back of its two
 * offsets and every read-back of the totals. */
int64_t mrx_debug_lines_syncs(void);
/* Lines on the CPU, for tests without a GPU: the block walk of the kernels over the same pieces (the pinned size, else
 * the default), one after the other, on the texts data[offsets[i], offsets[i + 1]).  Arguments, outputs, capacity rules
 * and return codes as mrx_lines_batch. */
int mrx_debug_lines_host(uint32_t flags, uint8_t sep, const uint8_t* data, const int64_t* offsets, int64_t n,
                         int64_t* line_prefix, int64_t* owner, int64_t* out_offsets, int64_t piece_cap, uint8_t* out_data,
                         int64_t out_cap, int64_t* totals);
/* Fields (include/mrx.h): `lanes`, a power of two from 1 to 64, pins G, the lanes that share a text, for every later
 * call; 0 restores the rule (the mean text length where the call knows it); any other value changes nothing.  Returns
 * the pin in force (0 = the rule).  The kernel reports itself as "k_fields" through mrx_last_kernel_name().  Results are
 * the same. */
int mrx_debug_fields_group(int lanes);
/* Fields: the G, the lanes that shared a text, of the last launch on this process, pinned or chosen by the rule (0 = no
 * launch yet; a batch without texts launches nothing).  Process-wide, like mrx_last_kernel_name. */
int mrx_debug_fields_last_group(void);
/* Fields: `workgroups` > 0 caps the grid, so that a test makes one wavefront run many rounds of texts without millions
 * of them, as mrx_debug_parse_grid does.  0 (default) = no cap of its own.  Results are the same. */
void mrx_debug_fields_grid(int workgroups);
/* Fields on the CPU, for tests without a GPU: the walk of the kernel over the same groups and rounds (the pinned G, else
 * the rule from the mean length), one text after the other, on the texts data[offsets[i], offsets[i + 1]).  Arguments,
 * outputs and return codes as mrx_fields_batch. */
int mrx_debug_fields_host(uint32_t flags, uint8_t delim, const int32_t* columns, int32_t f, const uint8_t* data,
                          const int64_t* offsets, int64_t n, int32_t* rows, int32_t* nf, int64_t* prefix);
/* Quoted fields on the CPU: mrx_debug_fields_host with the quote, over the same groups and rounds as the kernel and with
 * the same parity arithmetic (the ballot of a group's lanes is put together lane by lane).  The buffer that the walk
 * reads holds quote bytes around the texts.  Arguments, outputs and return codes as mrx_fields_quoted_batch. */
int mrx_debug_fields_quoted_host(uint32_t flags, uint8_t delim, uint8_t quote, const int32_t* columns, int32_t f,
                                 const uint8_t* data, const int64_t* offsets, int64_t n, int32_t* rows, int32_t* nf,
                                 uint8_t* quoted, int64_t* prefix);
/* Translate (include/mrx.h): bytes > 0 pins the piece size P of every later call of the packed form (rounded up to a
 * multiple of 1024, a wavefront's round), 0 restores the default, a negative value changes nothing.  Returns the P in
 * force: tests place their runs by it.  The passes report themselves as "k_translate_map" (same-length form) and
 * "k_translate_emit" through mrx_last_kernel_name(), strip as "k_strip".  Results are the same. */
int64_t mrx_debug_translate_piece(int64_t bytes);
/* How often mrx_translate_* has synchronised with the device on this process so far: the CSR form's read-back of its two
 * offsets and every read-back of the totals.  (Strip never does.) */
int64_t mrx_debug_translate_syncs(void);
/* Translate and strip on the CPU, for tests without a GPU: the block walks of the kernels, over the same pieces (the
 * pinned size, else the default), one block after the other, on the texts data[offsets[i], offsets[i + 1]).  Arguments, outputs, capacity rules and return codes as
 * mrx_translate_batch and mrx_strip_batch. */
int mrx_debug_translate_host(const uint8_t* table, const uint8_t* delete_set, const uint8_t* squeeze_set, const uint8_t* data,
                             const int64_t* offsets, int64_t n, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap,
                             int64_t* totals);
int mrx_debug_strip_host(const uint8_t* set, uint32_t flags, const uint8_t* data, const int64_t* offsets, int64_t n,
                         int32_t* rows, int64_t* prefix);
/* Bytes of device memory the calling thread's scratch arenas hold (see mrx_release_scratch). */
size_t mrx_debug_scratch_bytes(void);
/* ... and how many of them are handed out and not yet rewound.  Scratch belongs to the call's scope, so between calls
 * this is 0 whichever way the last call returned. */
size_t mrx_debug_scratch_in_use(void);

#ifdef __cplusplus
}
#endif
#endif /* MRX_TESTING_H */
