"""ctypes binding of include/mrx.h plus the reference-shaped Python interface.

See the package docstring for the mapping to src/regex/matcher.mojo.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libmrx_hip.so"
_lib = None

MRX_OK, MRX_E_SYNTAX, MRX_E_UNSUPPORTED, MRX_E_NO_DEVICE, MRX_E_CAPACITY, MRX_E_ARGUMENT = range(6)


class MrxError(RuntimeError):
    """Any failure reported by libmrx_hip.so."""


class RegexSyntaxError(MrxError):
    """The reference's lexer/parser raises on this pattern (same message)."""


class UnsupportedPattern(MrxError):
    """The reference routes this pattern/operation to an engine outside the hot
    path this library implements (backtracking NFA, OnePass)."""


def library_path() -> str:
    # MRX_LIB: measurement hook (tools/ablate.sh loads instrumented builds of the same library)
    return os.environ.get("MRX_LIB") or os.path.join(_HERE, _LIB_NAME)


def load_library():
    """Load libmrx_hip.so (built in-tree by __graft_entry__.build()).  Loud
    failure if it is missing: there is no other implementation to fall back to."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise MrxError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
    try:
        # PyTorch wheels bundle their own HIP runtime.  Load it first so that the
        # process holds ONE libamdhip64 (ours resolves to the copy already mapped);
        # two runtimes in one process do not share the device.
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(path)
    H = C.c_void_p
    u8p, i32p, i64p = C.c_void_p, C.c_void_p, C.c_void_p
    sigs = {
        "mrx_compile": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(H)]),
        "mrx_compile_ex": (C.c_int, [C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(H)]),
        "mrx_free": (None, [H]),
        "mrx_last_error": (C.c_char_p, []),
        "mrx_engine_type": (C.c_char_p, [H]),
        "mrx_stats": (C.c_char_p, [H]),
        "mrx_describe": (C.c_size_t, [H, C.c_char_p, C.c_size_t]),
        "mrx_num_groups": (C.c_int, [H]),
        "mrx_match_first_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i32p, i32p, C.c_void_p]),
        "mrx_search_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i32p, i32p, C.c_void_p]),
        "mrx_match_first_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i32p,
                                                  i32p, C.c_void_p]),
        "mrx_search_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i32p, i32p,
                                             C.c_void_p]),
        "mrx_is_match_dev": (C.c_int, [H, u8p, i64p, C.c_int64, u8p, C.c_void_p]),
        "mrx_is_match_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, u8p, C.c_void_p]),
        "mrx_match_first_at_dev": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int32, i32p, i32p, i32p, C.c_void_p]),
        "mrx_search_at_dev": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int32, i32p, i32p, i32p, C.c_void_p]),
        "mrx_is_match_at_dev": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int32, i32p, u8p, C.c_void_p]),
        "mrx_match_first_at_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, C.c_int32, i32p,
                                                     i32p, i32p, C.c_void_p]),
        "mrx_search_at_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, C.c_int32, i32p,
                                                i32p, i32p, C.c_void_p]),
        "mrx_is_match_at_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, C.c_int32, i32p,
                                                  u8p, C.c_void_p]),
        "mrx_findall_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i64p, i32p, C.c_int64,
                                      C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_findall_known_dev": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i32p, C.c_int64,
                                           C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_findall_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p,
                                              i32p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_count_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i32p, C.c_void_p]),
        "mrx_count_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i32p, C.c_void_p]),
        "mrx_captures_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i32p, C.c_void_p]),
        "mrx_captures_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i32p, C.c_void_p]),
        "mrx_captures_all_dev": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int64, i64p, i32p, C.c_int64,
                                           C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_captures_all_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, C.c_int64, i64p, i32p,
                                                   C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_captures_all_batch": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int64, i64p, i32p, C.c_int64,
                                             C.POINTER(C.c_int64)]),
        "mrx_sub_dev": (C.c_int, [H, C.c_char_p, C.c_size_t, C.c_int64, u8p, i64p, C.c_int64, i64p,
                                  u8p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_sub_known_dev": (C.c_int, [H, C.c_char_p, C.c_size_t, C.c_int64, u8p, i64p, C.c_int64, C.c_int64, C.c_int64,
                                        i64p, u8p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_sub_strided_dev": (C.c_int, [H, C.c_char_p, C.c_size_t, C.c_int64, u8p, C.c_int64, i32p, C.c_int32,
                                          C.c_int64, i64p, u8p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_match_first_batch": (C.c_int, [H, u8p, i64p, C.c_int64, i32p, i32p]),
        "mrx_search_batch": (C.c_int, [H, u8p, i64p, C.c_int64, i32p, i32p]),
        "mrx_is_match_batch": (C.c_int, [H, u8p, i64p, C.c_int64, u8p]),
        "mrx_split_batch": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int64, i64p, i32p, C.c_int64, C.POINTER(C.c_int64)]),
        "mrx_split_dev": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_split_strided_dev": (C.c_int, [H, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                            C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_findall_batch": (C.c_int, [H, u8p, i64p, C.c_int64, i64p, i32p, C.c_int64,
                                        C.POINTER(C.c_int64)]),
        "mrx_captures_batch": (C.c_int, [H, u8p, i64p, C.c_int64, i32p]),
        "mrx_sub_batch": (C.c_int, [H, C.c_char_p, C.c_size_t, C.c_int64, u8p, i64p, C.c_int64, i64p,
                                    u8p, C.c_int64, C.POINTER(C.c_int64)]),
        "mrx_timing_reset": (None, []),
        "mrx_timing_enable": (None, [C.c_int]),
        "mrx_timing_scan_ms": (C.c_double, [C.POINTER(C.c_int64)]),
        "mrx_last_kernel_name": (C.c_char_p, []),
        "mrx_debug_force_generic": (None, [C.c_int]),
        "mrx_debug_long_text_kernels": (None, [C.c_int]),
        "mrx_debug_fused_findall": (None, [C.c_int]),
        "mrx_debug_stream_bits": (None, [C.c_int]),
        "mrx_debug_stream_bits_trace": (None, [C.c_void_p]),
        "mrx_debug_dynamic_texts": (None, [C.c_int]),
        "mrx_debug_subs_group": (None, [C.c_int]),
        "mrx_debug_split_findall": (None, [C.c_int]),
        "mrx_debug_dense_rows": (None, [C.c_int]),
        "mrx_debug_tries_always": (None, [C.c_int]),
        "mrx_debug_chain_sub_general": (None, [C.c_int]),
        "mrx_testing_emptywalk_findall": (C.c_int, [H, C.c_char_p, C.c_int, i32p, C.c_int]),
        "mrx_debug_litscan_pieces": (None, [C.c_int]),
        "mrx_debug_multiwalk": (None, [C.c_int]),
        "mrx_debug_rec_skew": (None, [C.c_int64]),
        "mrx_debug_rec12": (None, [C.c_int]),
        "mrx_testing_rec12_roundtrip": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
        "mrx_debug_decode_lean": (None, [C.c_int]),
        "mrx_debug_last_decode_lean": (C.c_int, []),
        "mrx_testing_decode_expand": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_void_p]),
        "mrx_debug_decode_store16": (None, [C.c_int]),
        "mrx_debug_last_decode_store16": (C.c_int, []),
        "mrx_testing_decode_store_plan": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int32)]),
        "mrx_release_scratch": (None, []),
        "mrx_debug_scratch_bytes": (C.c_size_t, []),
        "mrx_debug_scratch_in_use": (C.c_size_t, []),
        "mrx_version": (C.c_char_p, []),
        # include/mrx_comm.h: results exchange between ranks (RCCL, opened on first use)
        "mrx_comm_unique_id": (C.c_int, [C.c_void_p]),
        "mrx_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(H)]),
        "mrx_comm_free": (None, [H]),
        "mrx_comm_rank": (C.c_int, [H]),
        "mrx_comm_size": (C.c_int, [H]),
        "mrx_comm_spans_staging_bytes": (C.c_size_t, [H, C.c_int64, C.c_int64]),
        "mrx_comm_reserve": (C.c_int, [H, C.c_size_t]),
        "mrx_allgather_fixed": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
        "mrx_allgatherv_rows": (C.c_int, [H, C.c_void_p, C.c_int64, C.c_size_t, C.c_void_p, C.c_int64,
                                          C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_allgatherv_spans": (C.c_int, [H, i64p, C.c_int64, i32p, C.c_int64, C.c_int64, i64p, C.c_int64, i32p,
                                           C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32p, C.c_void_p]),
        "mrx_testing_comm_shift": (C.c_int, [i64p, C.c_int64, i64p, C.c_int, C.c_int, i64p, C.c_int64, C.c_void_p]),
        "mrx_testing_comm_compact": (C.c_int, [i64p, C.c_int, C.c_int, i64p, C.c_int64, i32p, C.c_int64, i64p, C.c_int64,
                                               i32p, C.c_int64, i32p, C.c_void_p]),
        # pattern sets
        "mrx_set_compile": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int32, C.c_uint32, C.POINTER(H)]),
        "mrx_set_free": (None, [H]),
        "mrx_set_size": (C.c_int32, [H]),
        "mrx_set_describe": (C.c_size_t, [H, C.c_char_p, C.c_size_t]),
        "mrx_set_search_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i32p, i32p, C.c_void_p]),
        "mrx_set_search_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i32p, i32p, C.c_void_p]),
        "mrx_set_count_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i32p, C.c_void_p]),
        "mrx_set_count_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i32p, C.c_void_p]),
        "mrx_set_matches_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i64p, C.c_void_p]),
        "mrx_set_matches_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, C.c_void_p]),
        "mrx_set_findall_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i64p, i32p, i32p, C.c_int64, C.POINTER(C.c_int64),
                                          C.c_void_p]),
        "mrx_set_findall_known_dev": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i32p, i32p,
                                                C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_set_findall_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i32p, i32p,
                                                  C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_set_findall_batch": (C.c_int, [H, u8p, i64p, C.c_int64, i64p, i32p, i32p, C.c_int64, C.POINTER(C.c_int64)]),
        "mrx_set_sub_dev": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int64, u8p, i64p, C.c_int64, i64p, u8p, C.c_int64,
                                      i32p, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_set_sub_known_dev": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int64, u8p, i64p, C.c_int64, C.c_int64,
                                            C.c_int64, i64p, u8p, C.c_int64, i32p, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_set_sub_strided_dev": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int64, u8p, C.c_int64, i32p, C.c_int32,
                                              C.c_int64, i64p, u8p, C.c_int64, i32p, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_set_sub_batch": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int64, u8p, i64p, C.c_int64, i64p, u8p, C.c_int64,
                                        i32p, C.POINTER(C.c_int64)]),
        # filter: (handle, flags) | the batch | (kept_idx, out_offsets, out_data, out_cap, d_totals, totals, stream)
        "mrx_filter_dev": (C.c_int, [H, C.c_uint32, u8p, i64p, C.c_int64, i64p, i64p, u8p, C.c_int64, i64p,
                                     C.c_void_p, C.c_void_p]),
        "mrx_filter_known_dev": (C.c_int, [H, C.c_uint32, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i64p, u8p,
                                           C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_filter_strided_dev": (C.c_int, [H, C.c_uint32, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i64p, u8p,
                                             C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_filter_batch": (C.c_int, [H, C.c_uint32, u8p, i64p, C.c_int64, i64p, i64p, u8p, C.c_int64, C.c_void_p]),
        "mrx_set_filter_dev": (C.c_int, [H, C.c_uint32, u8p, i64p, C.c_int64, i64p, i64p, u8p, C.c_int64, i64p,
                                         C.c_void_p, C.c_void_p]),
        "mrx_set_filter_known_dev": (C.c_int, [H, C.c_uint32, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i64p,
                                               u8p, C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_set_filter_strided_dev": (C.c_int, [H, C.c_uint32, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i64p,
                                                 u8p, C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_set_filter_batch": (C.c_int, [H, C.c_uint32, u8p, i64p, C.c_int64, i64p, i64p, u8p, C.c_int64, C.c_void_p]),
        "mrx_debug_filter_form": (None, [C.c_int]),
        # extract: the batch | (prefix, spans, row_pairs, pair, piece_cap, owner, out_offsets, out_data, out_cap, d_totals,
        # totals, stream); with a handle (handle) | the batch | (piece_prefix, owner, out_offsets, piece_cap, out_data, ...)
        "mrx_gather_spans_dev": (C.c_int, [u8p, i64p, C.c_int64, i64p, i32p, C.c_int32, C.c_int32, C.c_int64, i64p, i64p,
                                           u8p, C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_gather_spans_strided_dev": (C.c_int, [u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i32p, C.c_int32,
                                                   C.c_int32, C.c_int64, i64p, i64p, u8p, C.c_int64, i64p, C.c_void_p,
                                                   C.c_void_p]),
        "mrx_gather_spans_batch": (C.c_int, [u8p, i64p, C.c_int64, i64p, i32p, C.c_int32, C.c_int32, C.c_int64, i64p, i64p,
                                             u8p, C.c_int64, C.c_void_p]),
        "mrx_extract_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i64p, i64p, i64p, C.c_int64, u8p, C.c_int64, i64p,
                                      C.c_void_p, C.c_void_p]),
        "mrx_extract_known_dev": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i64p, i64p, C.c_int64, u8p,
                                            C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_extract_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i64p, i64p, C.c_int64,
                                              u8p, C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_extract_batch": (C.c_int, [H, u8p, i64p, C.c_int64, i64p, i64p, i64p, C.c_int64, u8p, C.c_int64, C.c_void_p]),
        "mrx_debug_extract_grid": (None, [C.c_int]),
        # expand: the batch | (prefix, rows, row_pairs, tpl, tpl_len, piece_cap, owner, out_offsets, out_data, out_cap,
        # d_totals, totals, stream); with a handle (handle, tpl, tpl_len, count) | the batch | (match_prefix, owner,
        # out_offsets, match_cap, out_data, ...)
        "mrx_expand_spans_dev": (C.c_int, [u8p, i64p, C.c_int64, i64p, i32p, C.c_int32, C.c_char_p, C.c_size_t, C.c_int64,
                                           i64p, i64p, u8p, C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_expand_spans_strided_dev": (C.c_int, [u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i32p, C.c_int32,
                                                   C.c_char_p, C.c_size_t, C.c_int64, i64p, i64p, u8p, C.c_int64, i64p,
                                                   C.c_void_p, C.c_void_p]),
        "mrx_expand_spans_batch": (C.c_int, [u8p, i64p, C.c_int64, i64p, i32p, C.c_int32, C.c_char_p, C.c_size_t, C.c_int64,
                                             i64p, i64p, u8p, C.c_int64, C.c_void_p]),
        "mrx_expand_dev": (C.c_int, [H, C.c_char_p, C.c_size_t, C.c_int64, u8p, i64p, C.c_int64, i64p, i64p, i64p, C.c_int64,
                                     u8p, C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_expand_strided_dev": (C.c_int, [H, C.c_char_p, C.c_size_t, C.c_int64, u8p, C.c_int64, i32p, C.c_int32, C.c_int64,
                                             i64p, i64p, i64p, C.c_int64, u8p, C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_expand_batch": (C.c_int, [H, C.c_char_p, C.c_size_t, C.c_int64, u8p, i64p, C.c_int64, i64p, i64p, i64p,
                                       C.c_int64, u8p, C.c_int64, C.c_void_p]),
        "mrx_debug_expand_grid": (None, [C.c_int]),
        # distinct: the batch | (group_of, first, counts, out_offsets, out_data, out_cap, d_totals, totals, stream)
        "mrx_distinct_dev": (C.c_int, [u8p, i64p, C.c_int64, i64p, i64p, i64p, i64p, u8p, C.c_int64, i64p, C.c_void_p,
                                       C.c_void_p]),
        "mrx_distinct_known_dev": (C.c_int, [u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i64p, i64p, i64p, u8p,
                                             C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_distinct_strided_dev": (C.c_int, [u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i64p, i64p, i64p, u8p,
                                               C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_distinct_batch": (C.c_int, [u8p, i64p, C.c_int64, i64p, i64p, i64p, i64p, u8p, C.c_int64, C.c_void_p]),
        "mrx_debug_distinct_hash_mask": (None, [C.c_uint64]),
        "mrx_debug_distinct_grid": (None, [C.c_int]),
        # dictionaries: build: the entries | (stream, out); lookup: handle | the batch | (index, stream); filter:
        # (handle, flags) | the batch | (index, kept_idx, out_offsets, out_data, out_cap, d_totals, totals, stream)
        "mrx_dict_build_dev": (C.c_int, [u8p, i64p, C.c_int64, C.c_void_p, C.POINTER(H)]),
        "mrx_dict_build_strided_dev": (C.c_int, [u8p, C.c_int64, i32p, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(H)]),
        "mrx_dict_free": (None, [H]),
        "mrx_dict_size": (C.c_int64, [H]),
        "mrx_dict_distinct": (C.c_int64, [H]),
        "mrx_dict_lookup_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i64p, C.c_void_p]),
        "mrx_dict_lookup_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, C.c_void_p]),
        "mrx_dict_filter_dev": (C.c_int, [H, C.c_uint32, u8p, i64p, C.c_int64, i64p, i64p, i64p, u8p, C.c_int64, i64p,
                                          C.c_void_p, C.c_void_p]),
        "mrx_dict_filter_known_dev": (C.c_int, [H, C.c_uint32, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i64p, i64p,
                                                u8p, C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_dict_filter_strided_dev": (C.c_int, [H, C.c_uint32, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i64p,
                                                  i64p, u8p, C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_dict_lookup_batch": (C.c_int, [u8p, i64p, C.c_int64, u8p, i64p, C.c_int64, i64p]),
        # sorted index: build as a dictionary's; search: (handle, mode) | the batch | (lo, hi, stream)
        "mrx_sorted_build_dev": (C.c_int, [u8p, i64p, C.c_int64, C.c_void_p, C.POINTER(H)]),
        "mrx_sorted_build_strided_dev": (C.c_int, [u8p, C.c_int64, i32p, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(H)]),
        "mrx_sorted_free": (None, [H]),
        "mrx_sorted_size": (C.c_int64, [H]),
        "mrx_sorted_distinct": (C.c_int64, [H]),
        "mrx_sorted_order_dev": (C.c_int, [H, i64p, C.c_void_p]),
        "mrx_sorted_search_dev": (C.c_int, [H, C.c_uint32, u8p, i64p, C.c_int64, i64p, i64p, C.c_void_p]),
        "mrx_sorted_search_strided_dev": (C.c_int, [H, C.c_uint32, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i64p,
                                                    C.c_void_p]),
        "mrx_sorted_search_batch": (C.c_int, [u8p, i64p, C.c_int64, C.c_uint32, u8p, i64p, C.c_int64, i64p, i64p]),
        "mrx_debug_sorted_grid": (None, [C.c_int]),
        "mrx_debug_sorted_aids": (C.c_int, [C.c_int]),
        # sort: the batch | (order, rank, d_totals, stream); take: the batch | (index, k, out_offsets, out_data, out_cap,
        # d_totals, totals, stream)
        "mrx_sort_dev": (C.c_int, [u8p, i64p, C.c_int64, i64p, i64p, i64p, C.c_void_p]),
        "mrx_sort_known_dev": (C.c_int, [u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i64p, i64p, C.c_void_p]),
        "mrx_sort_strided_dev": (C.c_int, [u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i64p, i64p, C.c_void_p]),
        "mrx_sort_batch": (C.c_int, [u8p, i64p, C.c_int64, i64p, i64p, C.c_void_p]),
        "mrx_take_dev": (C.c_int, [u8p, i64p, C.c_int64, i64p, C.c_int64, i64p, u8p, C.c_int64, i64p, C.c_void_p,
                                   C.c_void_p]),
        "mrx_take_known_dev": (C.c_int, [u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, C.c_int64, i64p, u8p, C.c_int64,
                                         i64p, C.c_void_p, C.c_void_p]),
        "mrx_take_strided_dev": (C.c_int, [u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, C.c_int64, i64p, u8p, C.c_int64,
                                           i64p, C.c_void_p, C.c_void_p]),
        "mrx_take_batch": (C.c_int, [u8p, i64p, C.c_int64, i64p, C.c_int64, i64p, u8p, C.c_int64, C.c_void_p]),
        "mrx_debug_sort_small": (None, [C.c_int]),
        "mrx_debug_sort_grid": (None, [C.c_int]),
        "mrx_debug_sort_rounds": (C.c_int, []),
        # numbers: the batch | (kind, fill, values, status, stream); with spans: the batch | (prefix, spans, row_pairs,
        # pair, kind, fill, row_cap, values, status, owner, d_totals, totals, stream)
        "mrx_parse_dev": (C.c_int, [u8p, i64p, C.c_int64, C.c_int32, C.c_int64, i64p, u8p, C.c_void_p]),
        "mrx_parse_strided_dev": (C.c_int, [u8p, C.c_int64, i32p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, i64p, u8p,
                                            C.c_void_p]),
        "mrx_parse_spans_dev": (C.c_int, [u8p, i64p, C.c_int64, i64p, i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                          C.c_int64, i64p, u8p, i64p, i64p, C.c_void_p, C.c_void_p]),
        "mrx_parse_spans_strided_dev": (C.c_int, [u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i32p, C.c_int32,
                                                  C.c_int32, C.c_int32, C.c_int64, C.c_int64, i64p, u8p, i64p, i64p,
                                                  C.c_void_p, C.c_void_p]),
        "mrx_parse_batch": (C.c_int, [u8p, i64p, C.c_int64, C.c_int32, C.c_int64, i64p, u8p]),
        "mrx_debug_parse_grid": (None, [C.c_int]),
        # format: (tpl, tpl_len, cols, ncols, n, out_offsets, out_data, out_cap, row_status, d_totals, totals, stream); on
        # host buffers without d_totals and stream
        "mrx_format_dev": (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_int32, C.c_int64, i64p, u8p, C.c_int64, u8p, i64p,
                                     C.c_void_p, C.c_void_p]),
        "mrx_format_batch": (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_int32, C.c_int64, i64p, u8p, C.c_int64, u8p,
                                       C.c_void_p]),
        "mrx_debug_format_grid": (None, [C.c_int]),
        "mrx_testing_format_one": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_void_p]),
        # keywords: the handle | the batch | (flag / count, stream); findall: ... | (text_prefix, entries, spans, span_cap,
        # total, stream); filter as mrx_filter
        "mrx_kw_build": (C.c_int, [u8p, i64p, C.c_int64, C.c_uint32, C.c_void_p, C.POINTER(H)]),
        "mrx_kw_build_dev": (C.c_int, [u8p, i64p, C.c_int64, C.c_uint32, C.c_void_p, C.POINTER(H)]),
        "mrx_kw_free": (None, [H]),
        "mrx_kw_size": (C.c_int64, [H]),
        "mrx_kw_distinct": (C.c_int64, [H]),
        "mrx_kw_describe": (C.c_size_t, [H, C.c_char_p, C.c_size_t]),
        "mrx_kw_contains_dev": (C.c_int, [H, u8p, i64p, C.c_int64, u8p, C.c_void_p]),
        "mrx_kw_contains_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, u8p, C.c_void_p]),
        "mrx_kw_count_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i64p, C.c_void_p]),
        "mrx_kw_count_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, C.c_void_p]),
        "mrx_kw_findall_dev": (C.c_int, [H, u8p, i64p, C.c_int64, i64p, i32p, i32p, C.c_int64, C.POINTER(C.c_int64),
                                         C.c_void_p]),
        "mrx_kw_findall_known_dev": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i32p, i32p, C.c_int64,
                                               C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_kw_findall_strided_dev": (C.c_int, [H, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i32p, i32p, C.c_int64,
                                                 C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_kw_filter_dev": (C.c_int, [H, C.c_uint32, u8p, i64p, C.c_int64, i64p, i64p, u8p, C.c_int64, i64p, C.c_void_p,
                                        C.c_void_p]),
        "mrx_kw_filter_known_dev": (C.c_int, [H, C.c_uint32, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i64p, u8p,
                                              C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_kw_filter_strided_dev": (C.c_int, [H, C.c_uint32, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i64p, u8p,
                                                C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_kw_findall_batch": (C.c_int, [H, u8p, i64p, C.c_int64, i64p, i32p, i32p, C.c_int64, C.POINTER(C.c_int64)]),
        # leftmost: the handle, count | the batch | findall's tail; sub: the handle, (repl data, offsets, r), count | the
        # batch | (out_offsets, out_data, out_cap, nsub, d_totals, totals, stream)
        "mrx_kw_leftmost_dev": (C.c_int, [H, C.c_int64, u8p, i64p, C.c_int64, i64p, i32p, i32p, C.c_int64,
                                          C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_kw_leftmost_known_dev": (C.c_int, [H, C.c_int64, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i32p, i32p,
                                                C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_kw_leftmost_strided_dev": (C.c_int, [H, C.c_int64, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i32p, i32p,
                                                  C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
        "mrx_kw_leftmost_batch": (C.c_int, [H, C.c_int64, u8p, i64p, C.c_int64, i64p, i32p, i32p, C.c_int64,
                                            C.POINTER(C.c_int64)]),
        "mrx_kw_sub_dev": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int64, u8p, i64p, C.c_int64, i64p, u8p, C.c_int64, i32p,
                                     i64p, C.c_void_p, C.c_void_p]),
        "mrx_kw_sub_known_dev": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int64, u8p, i64p, C.c_int64, C.c_int64, C.c_int64,
                                           i64p, u8p, C.c_int64, i32p, i64p, C.c_void_p, C.c_void_p]),
        "mrx_kw_sub_strided_dev": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int64, u8p, C.c_int64, i32p, C.c_int32, C.c_int64,
                                             i64p, u8p, C.c_int64, i32p, i64p, C.c_void_p, C.c_void_p]),
        "mrx_kw_sub_batch": (C.c_int, [H, u8p, i64p, C.c_int64, C.c_int64, u8p, i64p, C.c_int64, i64p, u8p, C.c_int64, i32p,
                                       C.c_void_p]),
        "mrx_debug_kw_host_leftmost": (C.c_int, [u8p, i64p, C.c_int64, C.c_uint32, C.c_int64, u8p, i64p, C.c_int64, i64p,
                                                 i32p, i32p, C.c_int64, C.POINTER(C.c_int64)]),
        "mrx_debug_kw_host_sub": (C.c_int, [u8p, i64p, C.c_int64, C.c_uint32, u8p, i64p, C.c_int64, C.c_int64, u8p, i64p,
                                            C.c_int64, i64p, u8p, C.c_int64, i32p, C.c_void_p]),
        "mrx_debug_kw_piece": (None, [C.c_int64]),
        "mrx_debug_kw_tier": (None, [C.c_int]),
        "mrx_debug_kw_host_findall": (C.c_int, [u8p, i64p, C.c_int64, C.c_uint32, u8p, i64p, C.c_int64, i64p, i32p, i32p,
                                                C.c_int64, C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]),
        "mrx_lines_dev": (C.c_int, [C.c_uint32, C.c_uint8, u8p, i64p, C.c_int64, i64p, i64p, i64p, C.c_int64, u8p, C.c_int64,
                                    i64p, C.c_void_p, C.c_void_p]),
        "mrx_lines_known_dev": (C.c_int, [C.c_uint32, C.c_uint8, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i64p, i64p,
                                          C.c_int64, u8p, C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_lines_strided_dev": (C.c_int, [C.c_uint32, C.c_uint8, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i64p, i64p,
                                            i64p, C.c_int64, u8p, C.c_int64, i64p, C.c_void_p, C.c_void_p]),
        "mrx_lines_batch": (C.c_int, [C.c_uint32, C.c_uint8, u8p, i64p, C.c_int64, i64p, i64p, i64p, C.c_int64, u8p,
                                      C.c_int64, C.c_void_p]),
        "mrx_debug_lines_piece": (C.c_int64, [C.c_int64]),
        "mrx_debug_lines_syncs": (C.c_int64, []),
        "mrx_debug_lines_host": (C.c_int, [C.c_uint32, C.c_uint8, u8p, i64p, C.c_int64, i64p, i64p, i64p, C.c_int64, u8p,
                                           C.c_int64, C.c_void_p]),
        "mrx_fields_dev": (C.c_int, [C.c_uint32, C.c_uint8, i32p, C.c_int32, u8p, i64p, C.c_int64, i32p, i32p, i64p,
                                     C.c_void_p]),
        "mrx_fields_known_dev": (C.c_int, [C.c_uint32, C.c_uint8, i32p, C.c_int32, u8p, i64p, C.c_int64, C.c_int64,
                                           C.c_int64, i32p, i32p, i64p, C.c_void_p]),
        "mrx_fields_strided_dev": (C.c_int, [C.c_uint32, C.c_uint8, i32p, C.c_int32, u8p, C.c_int64, i32p, C.c_int32,
                                             C.c_int64, i32p, i32p, i64p, C.c_void_p]),
        "mrx_fields_batch": (C.c_int, [C.c_uint32, C.c_uint8, i32p, C.c_int32, u8p, i64p, C.c_int64, i32p, i32p, i64p]),
        "mrx_fields_quoted_dev": (C.c_int, [C.c_uint32, C.c_uint8, C.c_uint8, i32p, C.c_int32, u8p, i64p, C.c_int64, i32p,
                                            i32p, u8p, i64p, C.c_void_p]),
        "mrx_fields_quoted_strided_dev": (C.c_int, [C.c_uint32, C.c_uint8, C.c_uint8, i32p, C.c_int32, u8p, C.c_int64, i32p,
                                                    C.c_int32, C.c_int64, i32p, i32p, u8p, i64p, C.c_void_p]),
        "mrx_fields_quoted_batch": (C.c_int, [C.c_uint32, C.c_uint8, C.c_uint8, i32p, C.c_int32, u8p, i64p, C.c_int64, i32p,
                                              i32p, u8p, i64p]),
        "mrx_debug_fields_quoted_host": (C.c_int, [C.c_uint32, C.c_uint8, C.c_uint8, i32p, C.c_int32, u8p, i64p, C.c_int64,
                                                   i32p, i32p, u8p, i64p]),
        "mrx_debug_fields_group": (C.c_int, [C.c_int]),
        "mrx_debug_fields_last_group": (C.c_int, []),
        "mrx_debug_fields_grid": (None, [C.c_int]),
        "mrx_debug_fields_host": (C.c_int, [C.c_uint32, C.c_uint8, i32p, C.c_int32, u8p, i64p, C.c_int64, i32p, i32p,
                                            i64p]),
        "mrx_translate_dev": (C.c_int, [u8p, u8p, u8p, u8p, i64p, C.c_int64, u8p, C.c_int64, i64p, i64p, C.c_void_p,
                                        C.c_void_p]),
        "mrx_translate_known_dev": (C.c_int, [u8p, u8p, u8p, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, u8p, C.c_int64,
                                              i64p, i64p, C.c_void_p, C.c_void_p]),
        "mrx_translate_strided_dev": (C.c_int, [u8p, u8p, u8p, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, u8p, C.c_int64,
                                                i64p, i64p, C.c_void_p, C.c_void_p]),
        "mrx_translate_batch": (C.c_int, [u8p, u8p, u8p, u8p, i64p, C.c_int64, i64p, u8p, C.c_int64, C.c_void_p]),
        "mrx_strip_dev": (C.c_int, [u8p, C.c_uint32, u8p, i64p, C.c_int64, i32p, i64p, C.c_void_p]),
        "mrx_strip_known_dev": (C.c_int, [u8p, C.c_uint32, u8p, i64p, C.c_int64, C.c_int64, C.c_int64, i32p, i64p,
                                          C.c_void_p]),
        "mrx_strip_strided_dev": (C.c_int, [u8p, C.c_uint32, u8p, C.c_int64, i32p, C.c_int32, C.c_int64, i32p, i64p,
                                            C.c_void_p]),
        "mrx_strip_batch": (C.c_int, [u8p, C.c_uint32, u8p, i64p, C.c_int64, i32p, i64p]),
        "mrx_debug_translate_piece": (C.c_int64, [C.c_int64]),
        "mrx_debug_translate_syncs": (C.c_int64, []),
        "mrx_debug_translate_host": (C.c_int, [u8p, u8p, u8p, u8p, i64p, C.c_int64, i64p, u8p, C.c_int64, C.c_void_p]),
        "mrx_debug_strip_host": (C.c_int, [u8p, C.c_uint32, u8p, i64p, C.c_int64, i32p, i64p]),
        "mrx_debug_set_route": (None, [C.c_int]),
        "mrx_testing_set_run": (C.c_int, [H, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int32)]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


# include/mrx.h (the drop-in boundary) and include/mrx_testing.h (measurement / testing hooks)
EXPORTED_SYMBOLS = [
    "mrx_compile", "mrx_compile_ex", "mrx_free", "mrx_last_error", "mrx_engine_type", "mrx_stats", "mrx_describe",
    "mrx_num_groups", "mrx_match_first_dev", "mrx_search_dev", "mrx_match_first_strided_dev",
    "mrx_search_strided_dev", "mrx_is_match_dev", "mrx_is_match_strided_dev",
    "mrx_findall_dev", "mrx_findall_known_dev", "mrx_findall_strided_dev", "mrx_count_dev", "mrx_count_strided_dev",
    "mrx_captures_strided_dev", "mrx_captures_dev",
    "mrx_captures_all_dev", "mrx_captures_all_strided_dev", "mrx_captures_all_batch",
    "mrx_match_first_at_dev", "mrx_search_at_dev", "mrx_is_match_at_dev", "mrx_match_first_at_strided_dev",
    "mrx_search_at_strided_dev", "mrx_is_match_at_strided_dev",
    "mrx_sub_dev", "mrx_sub_known_dev", "mrx_sub_strided_dev", "mrx_split_dev", "mrx_split_strided_dev", "mrx_split_batch", "mrx_match_first_batch", "mrx_search_batch", "mrx_is_match_batch",
    "mrx_findall_batch", "mrx_captures_batch", "mrx_sub_batch", "mrx_version", "mrx_release_scratch",
    "mrx_set_compile", "mrx_set_free", "mrx_set_size", "mrx_set_describe", "mrx_set_search_dev",
    "mrx_set_search_strided_dev", "mrx_set_count_dev", "mrx_set_count_strided_dev", "mrx_set_matches_dev",
    "mrx_set_matches_strided_dev", "mrx_set_findall_dev", "mrx_set_findall_known_dev", "mrx_set_findall_strided_dev",
    "mrx_set_findall_batch", "mrx_set_sub_dev", "mrx_set_sub_known_dev", "mrx_set_sub_strided_dev", "mrx_set_sub_batch",
    "mrx_filter_dev", "mrx_filter_known_dev", "mrx_filter_strided_dev", "mrx_filter_batch",
    "mrx_set_filter_dev", "mrx_set_filter_known_dev", "mrx_set_filter_strided_dev", "mrx_set_filter_batch",
    "mrx_gather_spans_dev", "mrx_gather_spans_strided_dev", "mrx_gather_spans_batch",
    "mrx_extract_dev", "mrx_extract_known_dev", "mrx_extract_strided_dev", "mrx_extract_batch",
    "mrx_expand_spans_dev", "mrx_expand_spans_strided_dev", "mrx_expand_spans_batch",
    "mrx_expand_dev", "mrx_expand_strided_dev", "mrx_expand_batch",
    "mrx_distinct_dev", "mrx_distinct_known_dev", "mrx_distinct_strided_dev", "mrx_distinct_batch",
    "mrx_dict_build_dev", "mrx_dict_build_strided_dev", "mrx_dict_free", "mrx_dict_size", "mrx_dict_distinct",
    "mrx_dict_lookup_dev", "mrx_dict_lookup_strided_dev", "mrx_dict_filter_dev", "mrx_dict_filter_known_dev",
    "mrx_dict_filter_strided_dev", "mrx_dict_lookup_batch",
    "mrx_sort_dev", "mrx_sort_known_dev", "mrx_sort_strided_dev", "mrx_sort_batch",
    "mrx_take_dev", "mrx_take_known_dev", "mrx_take_strided_dev", "mrx_take_batch",
    "mrx_sorted_build_dev", "mrx_sorted_build_strided_dev", "mrx_sorted_free", "mrx_sorted_size", "mrx_sorted_distinct",
    "mrx_sorted_order_dev", "mrx_sorted_search_dev", "mrx_sorted_search_strided_dev", "mrx_sorted_search_batch",
    "mrx_parse_dev", "mrx_parse_strided_dev", "mrx_parse_spans_dev", "mrx_parse_spans_strided_dev", "mrx_parse_batch",
    "mrx_format_dev", "mrx_format_batch",
    "mrx_kw_build", "mrx_kw_build_dev", "mrx_kw_free", "mrx_kw_size", "mrx_kw_distinct", "mrx_kw_describe",
    "mrx_kw_contains_dev", "mrx_kw_contains_strided_dev", "mrx_kw_count_dev", "mrx_kw_count_strided_dev",
    "mrx_kw_findall_dev", "mrx_kw_findall_known_dev", "mrx_kw_findall_strided_dev", "mrx_kw_filter_dev",
    "mrx_kw_filter_known_dev", "mrx_kw_filter_strided_dev", "mrx_kw_findall_batch",
    "mrx_kw_leftmost_dev", "mrx_kw_leftmost_known_dev", "mrx_kw_leftmost_strided_dev", "mrx_kw_leftmost_batch",
    "mrx_kw_sub_dev", "mrx_kw_sub_known_dev", "mrx_kw_sub_strided_dev", "mrx_kw_sub_batch",
    "mrx_lines_dev", "mrx_lines_known_dev", "mrx_lines_strided_dev", "mrx_lines_batch",
    "mrx_fields_dev", "mrx_fields_known_dev", "mrx_fields_strided_dev", "mrx_fields_batch",
    "mrx_fields_quoted_dev", "mrx_fields_quoted_strided_dev", "mrx_fields_quoted_batch",
    "mrx_translate_dev", "mrx_translate_known_dev", "mrx_translate_strided_dev", "mrx_translate_batch",
    "mrx_strip_dev", "mrx_strip_known_dev", "mrx_strip_strided_dev", "mrx_strip_batch",
]
TESTING_SYMBOLS = [
    "mrx_timing_reset", "mrx_timing_enable", "mrx_timing_scan_ms", "mrx_last_kernel_name",
    "mrx_debug_force_generic", "mrx_debug_long_text_kernels", "mrx_debug_scratch_bytes",
    "mrx_debug_scratch_in_use",
    "mrx_debug_fused_findall", "mrx_debug_stream_bits", "mrx_debug_stream_bits_trace", "mrx_debug_dynamic_texts", "mrx_debug_subs_group",
    "mrx_debug_split_findall", "mrx_debug_dense_rows", "mrx_debug_tries_always", "mrx_debug_chain_sub_general", "mrx_testing_emptywalk_findall", "mrx_debug_litscan_pieces", "mrx_debug_multiwalk", "mrx_debug_rec_skew", "mrx_testing_comm_shift", "mrx_testing_comm_compact",
    "mrx_debug_set_route", "mrx_testing_set_run", "mrx_debug_filter_form", "mrx_debug_extract_grid",
    "mrx_debug_expand_grid", "mrx_debug_distinct_hash_mask", "mrx_debug_distinct_grid",
    "mrx_debug_sort_small", "mrx_debug_sort_grid", "mrx_debug_sort_rounds", "mrx_debug_parse_grid",
    "mrx_debug_sorted_grid", "mrx_debug_sorted_aids",
    "mrx_debug_decode_lean", "mrx_debug_last_decode_lean", "mrx_testing_decode_expand",
    "mrx_testing_decode_store_plan",
    "mrx_debug_format_grid", "mrx_testing_format_one",
    "mrx_debug_kw_piece", "mrx_debug_kw_tier", "mrx_debug_kw_host_findall",
    "mrx_debug_kw_host_leftmost", "mrx_debug_kw_host_sub",
    "mrx_debug_lines_piece", "mrx_debug_lines_syncs", "mrx_debug_lines_host",
    "mrx_debug_fields_group", "mrx_debug_fields_last_group", "mrx_debug_fields_grid", "mrx_debug_fields_host",
    "mrx_debug_fields_quoted_host",
    "mrx_debug_translate_piece", "mrx_debug_translate_syncs", "mrx_debug_translate_host",
    "mrx_debug_strip_host",
]
# (hooks with a digit in their name, listed apart: the header scan of tests/test_host_tables.py reads [a-z_] names)
TESTING_SYMBOLS_NUMBERED = ["mrx_debug_rec12", "mrx_testing_rec12_roundtrip", "mrx_debug_decode_store16",
                            "mrx_debug_last_decode_store16"]
COMM_SYMBOLS = [
    "mrx_comm_unique_id", "mrx_comm_init", "mrx_comm_free", "mrx_comm_rank", "mrx_comm_size",
    "mrx_comm_spans_staging_bytes", "mrx_comm_reserve",
    "mrx_allgather_fixed", "mrx_allgatherv_rows", "mrx_allgatherv_spans",
]


def _b(x) -> bytes:
    if isinstance(x, str):
        return x.encode("utf-8")
    return bytes(x)


def _check(rc: int):
    if rc == MRX_OK:
        return
    msg = load_library().mrx_last_error().decode("utf-8", "replace")
    if rc == MRX_E_SYNTAX:
        raise RegexSyntaxError(msg)
    if rc == MRX_E_UNSUPPORTED:
        raise UnsupportedPattern(msg)
    raise MrxError("mrx error %d: %s" % (rc, msg))


def pack_texts(texts: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """Pack texts back to back: (data uint8[total], offsets int64[n+1])."""
    bs = [_b(t) for t in texts]
    offsets = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(x) for x in bs], out=offsets[1:])
    data = np.frombuffer(b"".join(bs), dtype=np.uint8).copy() if offsets[-1] else np.zeros(0, np.uint8)
    return data, offsets


class DeviceBatch:
    """Texts already resident in HBM (torch tensors on a cuda device).

    CSR form:      DeviceBatch(data_u8, offsets_i64)
    strided form:  DeviceBatch.strided(data_u8[n*stride], stride, length or lens_i32)
    """

    def __init__(self, data, offsets=None, *, stride: int = 0, length: int = 0, lens=None, n=None):
        import torch
        if data.dtype != torch.uint8 or not data.is_contiguous():
            raise MrxError("batch data must be a contiguous uint8 tensor")
        self.data, self.offsets, self.stride, self.length, self.lens = data, offsets, stride, length, lens
        # CSR batches whose offsets were built on the host: offsets[n] and the longest text, so that findall does not
        # have to read them back from the device (mrx_findall_known_dev); None = not known.  Private: set by
        # from_texts / from_arrow only, from the very offsets they upload -- the C side sizes its record scratch from
        # them ("neither may be too small"), so a stale or hand-set value would be an out-of-bounds write, not an error
        self._end_offset: Optional[int] = None
        self._max_len: Optional[int] = None
        # from_lines only: the byte count of the source buffer's unterminated tail (include/mrx.h, "lines")
        self.tail: Optional[int] = None
        if offsets is not None:
            if offsets.dtype != torch.int64 or not offsets.is_contiguous() or offsets.device != data.device:
                raise MrxError("offsets must be a contiguous int64 tensor on the data's device")
            if offsets.numel() < 1:
                raise MrxError("offsets needs n + 1 entries")
            self.n = int(offsets.numel()) - 1
        else:
            self.n = int(n)

    @classmethod
    def csr_known(cls, data, offsets, end_offset: int, max_len: int):
        """A CSR batch whose builder knows offsets[n] and the longest text (it produced the offsets, or holds an Arrow
        array's): findall and sub then need no look at the device before their first kernel (mrx_findall_known_dev,
        mrx_sub_known_dev).  Upper bounds are fine; neither may be too small -- the C side sizes scratch from them that
        its kernels index with the real offsets."""
        b = cls(data, offsets)
        if int(end_offset) < 0 or int(max_len) < 0:
            raise MrxError("end_offset and max_len must not be negative")
        b._end_offset, b._max_len = int(end_offset), int(max_len)
        return b

    @classmethod
    def strided(cls, data, stride: int, length: Optional[int] = None, lens=None):
        """Texts at a fixed pitch: text i = data[i*stride : i*stride + (lens[i] | length)].  `length`
        (common to all texts) or `lens` (int32[n] on the data's device; takes precedence) must be given;
        lens[i] <= stride is the caller's contract (the kernels read lens[i] bytes of row i)."""
        import torch
        stride = int(stride)
        if stride <= 0 or data.numel() % stride:
            raise MrxError("data size %d is not a multiple of the stride %d" % (data.numel(), stride))
        n = data.numel() // stride
        if length is None and lens is None:
            raise MrxError("give length= (common to all texts) or lens= (per text; it takes precedence)")
        if lens is not None:
            if lens.dtype != torch.int32 or not lens.is_contiguous() or lens.device != data.device or lens.numel() != n:
                raise MrxError("lens must be a contiguous int32[n] tensor on the data's device")
            length = 0
        elif not 0 <= int(length) <= stride:
            raise MrxError("length must be in [0, stride]")
        return cls(data, None, stride=stride, length=int(length), lens=lens, n=n)

    @classmethod
    def from_texts(cls, texts: Sequence, device="cuda"):
        import torch
        data, offsets = pack_texts(texts)
        d = torch.from_numpy(data).to(device) if data.size else torch.zeros(0, dtype=torch.uint8, device=device)
        b = cls(d, torch.from_numpy(offsets).to(device))
        b._end_offset = int(offsets[-1])
        b._max_len = int(np.diff(offsets).max()) if len(offsets) > 1 else 0
        return b

    @classmethod
    def from_arrow(cls, arr, device="cuda"):
        """Batch from a pyarrow LargeBinary / LargeString array: the array's
        two buffers ARE the packed form of the C ABI -- text bytes back to back and int64
        offsets[n+1] -- so they are uploaded as they stand (a sliced array keeps its offsets; the
        data buffer is cut to the referenced range).  Nulls are treated as empty texts."""
        import numpy as np
        import pyarrow as pa
        import torch
        if isinstance(arr, pa.ChunkedArray):
            arr = arr.combine_chunks()
        if pa.types.is_binary(arr.type) or pa.types.is_string(arr.type):
            arr = arr.cast(pa.large_binary())
        if not (pa.types.is_large_binary(arr.type) or pa.types.is_large_string(arr.type)):
            raise MrxError("from_arrow needs a (large_)binary or (large_)string array")
        if arr.null_count:
            arr = arr.fill_null(b"")
        bufs = arr.buffers()   # [validity, offsets, data]
        n = len(arr)
        offs = np.frombuffer(bufs[1], dtype=np.int64, count=n + 1, offset=arr.offset * 8).copy()
        lo, hi = int(offs[0]), int(offs[-1])
        data = np.frombuffer(bufs[2], dtype=np.uint8, count=hi - lo, offset=lo) if hi > lo else np.zeros(0, np.uint8)
        offs -= lo
        d = torch.from_numpy(data.copy()).to(device) if data.size else torch.zeros(0, dtype=torch.uint8, device=device)
        b = cls(d, torch.from_numpy(offs).to(device))
        b._end_offset = int(offs[-1])
        b._max_len = int(np.diff(offs).max()) if n > 0 else 0
        return b

    _entry_points = {}   # call(): an operation's entry points, resolved once per stem

    def call(self, lib, op, head, tail):
        """One C call on this batch: op is an operation's stem ("mrx_findall", "mrx_set_sub", ...) or the pair
        (fn_csr, fn_strided).  Picks <stem>_strided_dev for a fixed pitch, <stem>_known_dev where the library has it and
        the batch knows its bounds, else <stem>_dev, and lays the batch out as the ABI does between the arguments in
        front of it (`head`) and those behind it (`tail`).  Returns the return code."""
        if isinstance(op, str):
            fns = self._entry_points.get(op)
            if fns is None:
                fns = self._entry_points[op] = (getattr(lib, op + "_dev"), getattr(lib, op + "_known_dev", None),
                                                getattr(lib, op + "_strided_dev"))
            fn_csr, fn_known, fn_strided = fns
        else:
            (fn_csr, fn_strided), fn_known = op, None
        # texts without a byte: a tensor of no elements has no address, and some entry points refuse a null d_data when
        # n > 0 (sets, captures_all) where others take it -- every batch passes a pointer, as format's text columns do
        data = _ptr(self.data) or _ptr(_no_bytes(self.data.device))
        if self.offsets is None:
            return fn_strided(*head, data, self.stride, _ptr(self.lens), self.length, self.n, *tail)
        if fn_known is not None and self._end_offset is not None:
            return fn_known(*head, data, _ptr(self.offsets), self.n, self._end_offset, self._max_len, *tail)
        return fn_csr(*head, data, _ptr(self.offsets), self.n, *tail)

    def csr_offsets(self):
        """CSR offsets for the generic kernels (built on device for strided batches)."""
        import torch
        if self.offsets is not None:
            return self.offsets
        if self.lens is None and self.length == self.stride:
            return torch.arange(0, (self.n + 1) * self.stride, self.stride, dtype=torch.int64,
                                device=self.data.device)
        raise MrxError("this operation needs a CSR batch (strided batch with padding given)")

    def longest(self) -> Optional[int]:
        """An upper bound of the longest text where the host knows one (a fixed pitch, known CSR bounds), else None:
        the known bound that filter's and extract's results carry on."""
        if self.offsets is not None:
            return self._max_len
        return self.stride if self.lens is not None else self.length

    def lines(self, sep=b"\n", keepends: bool = False, crlf: bool = False, partial: bool = True,
              piece_cap: Optional[int] = None, out_cap: Optional[int] = None):
        """This batch's texts cut at the byte `sep` into a new packed batch (include/mrx.h, mrx_lines_dev): (lines
        DeviceBatch, prefix int64[n + 1], owner int64[lines]), shaped as extract's result.  The lines of a text are
        text.split(sep) with the last piece dropped when it is empty: every separator ends a line, an unterminated
        tail is a line too, and no line crosses a text boundary.  keepends leaves every terminated line its separator;
        crlf (sep b"\\n" only, not with keepends) also drops one b"\\r" directly in front of a dropped b"\\n";
        partial=False leaves every text's unterminated tail out.  `lines.tail` is the byte count of the last text's
        unterminated tail, whatever `partial` says.  Without piece_cap / out_cap the call grows them as extract does
        (the default holds a line per 32 bytes; more lines cost one more pass).  `lines` is a CSR batch with known
        bounds, both exact: its bytes and its longest line, so findall on it reads nothing back and routes by the real
        line length.  A CSR input without known bounds pays one read-back of its first and last offset; one with them
        and a strided one do not."""
        return self._lines_call(_lines_flags(sep, keepends, crlf, partial), piece_cap, out_cap, True)

    def _lines_call(self, flags_sep, piece_cap: Optional[int], out_cap: Optional[int], move: bool):
        """lines() with extract's grow-and-retry over the four totals of mrx_lines_*: first the lines, then the bytes,
        each unless it is the caller's own.  move=False (from_lines with keepends: one text, whose lines with their
        separators are its own bytes) asks for the offsets alone with an output capacity of 0, takes the capacity code
        that the missing bytes give for success, and returns the input's data under the new offsets."""
        import torch
        dev, nbytes = self.data.device, int(self.data.numel())
        prefix = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
        d_totals = torch.empty(4, dtype=torch.int64, device=dev)
        totals = (C.c_int64 * 4)()
        lib = load_library()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        pcap = nbytes // 32 + self.n + 64 if piece_cap is None else int(piece_cap)
        ocap = 0 if not move else nbytes if out_cap is None else int(out_cap)
        pb = out = None
        while True:
            if pb is None:
                pb = (torch.empty(max(pcap, 1), dtype=torch.int64, device=dev), torch.empty(pcap + 1, dtype=torch.int64, device=dev))
            if out is None and ocap > 0:
                out = torch.empty(ocap, dtype=torch.uint8, device=dev)
            rc = self.call(lib, "mrx_lines", flags_sep,
                           (_ptr(prefix), _ptr(pb[0]), _ptr(pb[1]), pcap, _ptr(out), ocap, _ptr(d_totals),
                            C.cast(totals, C.c_void_p), stream))
            nlines, nb = int(totals[0]), int(totals[1])
            if rc == MRX_E_CAPACITY and piece_cap is None and nlines > pcap:
                pcap, pb = nlines, None
                continue
            if rc == MRX_E_CAPACITY and nlines <= pcap and nb > ocap:
                if not move:
                    break
                if out_cap is None:
                    ocap, out = nb, None
                    continue
            _check(rc)
            break
        trim_p = (lambda t, m: t[:m].clone()) if 4 * nlines < pcap else (lambda t, m: t[:m])
        trim_b = (lambda t, m: t[:m].clone()) if 4 * nb < ocap else (lambda t, m: t[:m])
        if not move:
            data = self.data
        else:
            data = trim_b(out, nb) if out is not None else torch.empty(0, dtype=torch.uint8, device=dev)
        res = DeviceBatch(data, trim_p(pb[1], nlines + 1))
        res._end_offset, res._max_len, res.tail = nb, int(totals[2]), int(totals[3])
        return res, prefix, trim_p(pb[0], nlines)

    @classmethod
    def from_lines(cls, data, sep=b"\n", keepends: bool = False, crlf: bool = False, partial: bool = True,
                   piece_cap: Optional[int] = None, out_cap: Optional[int] = None):
        """The lines of one buffer on the device (a file's bytes as a contiguous uint8 tensor) as a batch: lines() of
        the batch whose one text is the buffer, with `.tail` set for reading in chunks -- with partial=False carry
        data[len - tail:] in front of the next chunk.  Below 2^31 bytes the buffer is taken as a strided batch of one
        text (nothing is uploaded and nothing read back before the kernels), at and above that as a CSR batch of two
        offsets.  With keepends=True no byte moves: the result's `data` is the caller's tensor and only the offsets are
        computed."""
        import torch
        if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
            raise MrxError("from_lines needs a contiguous one-dimensional uint8 tensor")
        nbytes = int(data.numel())
        if 0 < nbytes < (1 << 31):
            src = cls.strided(data, nbytes, length=nbytes)
        else:
            src = cls(data, torch.tensor([0, nbytes], dtype=torch.int64, device=data.device))
        return src._lines_call(_lines_flags(sep, keepends, crlf, partial), piece_cap, out_cap, not keepends)[0]

    def lines_async(self, out, sep=b"\n", keepends: bool = False, crlf: bool = False, partial: bool = True):
        """Enqueue lines() on the current stream without reading its result back.  out = (line_prefix int64[n + 1],
        owner int64[piece_cap], out_offsets int64[piece_cap + 1], out_data uint8[out_cap], totals int64[4]) device
        tensors of the caller; totals = {lines, bytes, longest line, tail} once the stream has drained.  No byte is
        written when lines > piece_cap or bytes > out_cap (check totals against both).  A CSR batch without known
        bounds still pays the read-back of its first and last offset before the first kernel."""
        import torch
        flags, sep_byte = _lines_flags(sep, keepends, crlf, partial)
        prefix, owner, out_offsets, out_data, totals = out
        if prefix.numel() < self.n + 1 or out_offsets.numel() < owner.numel() + 1 or totals.numel() < 4:
            raise MrxError("out needs line_prefix int64[n + 1], owner int64[cap], out_offsets int64[cap + 1], "
                           "out_data uint8[out_cap], totals int64[4]")
        for t in (prefix, owner, out_offsets, totals):
            if t.dtype != torch.int64 or not t.is_contiguous():
                raise MrxError("line_prefix, owner, out_offsets and totals must be contiguous int64 tensors")
        if out_data.dtype != torch.uint8 or not out_data.is_contiguous():
            raise MrxError("out_data must be a contiguous uint8 tensor")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(self.call(load_library(), "mrx_lines", (flags, sep_byte),
                         (_ptr(prefix), _ptr(owner), _ptr(out_offsets), int(owner.numel()), _ptr(out_data),
                          int(out_data.numel()), _ptr(totals), None, stream)))

    def fields(self, columns, delim=None, rest: bool = False, counts: bool = True, quote=None):
        """The columns of every text as span rows (include/mrx.h, mrx_fields_dev): (prefix int64[n + 1], rows
        int32[n, f, 2], nf int32[n]), device tensors.  delim=None is whitespace mode, bytes.split() of every text; delim
        one byte is t.split(delim).  columns count from 1 as cut and awk do, or from -1 at the end ($NF); rest=True
        makes the largest column run to the end of the text.  rows[i, j] is (start, end) of column columns[j] in text i,
        (-1, -1) where the text has no such part; nf[i] is the field count (None with counts=False, which lets the
        kernel stop reading a text behind its largest column).  prefix is the identity CSR 0 .. n: prefix and rows go
        to gather_spans(pair=j), parse_spans(pair=j) and expand_spans as they stand.  A batch with known bounds passes
        them on.  The call enqueues on the current stream and reads nothing back.
        With quote (one byte, include/mrx.h, mrx_fields_quoted_dev) a delimiter or whitespace byte between quotes
        separates nothing, a part that begins and ends with the quote is given without both, and the result has a
        fourth value: (prefix, rows, nf, quoted uint8[n, f]), quoted[i, j] = 1 where the outer quotes were taken off.
        Doubled quotes stay in the content; csv_columns(batch, ...) takes them out."""
        import torch
        dev, f = self.data.device, len(columns)
        rows = torch.empty((self.n, f, 2), dtype=torch.int32, device=dev)
        nf = torch.empty(self.n, dtype=torch.int32, device=dev) if counts else None
        # n == 0 enqueues nothing: the one entry of the prefix is the host's to write
        prefix = torch.empty(self.n + 1, dtype=torch.int64, device=dev) if self.n else torch.zeros(1, dtype=torch.int64, device=dev)
        if quote is not None:
            quoted = torch.empty((self.n, f), dtype=torch.uint8, device=dev)
            self.fields_async((prefix, rows, nf, quoted), columns, delim, rest, quote)
            return prefix, rows, nf, quoted
        self.fields_async((prefix, rows, nf), columns, delim, rest)
        return prefix, rows, nf

    def fields_async(self, out, columns, delim=None, rest: bool = False, quote=None):
        """fields() on the caller's tensors out = (prefix int64[n + 1] or None, rows int32[n, f, 2], nf int32[n] or
        None), with quote out = (prefix, rows, nf, quoted uint8[n, f] or None): enqueues on the current stream and
        returns.  Nothing is written for a batch without texts."""
        import torch
        flags, delim_byte, cols = _fields_args(columns, delim, rest)
        quoted = None
        if quote is not None:
            quote_byte = _quote_byte(quote)
            prefix, rows, nf, quoted = out
            if quoted is not None and (quoted.dtype != torch.uint8 or not quoted.is_contiguous() or quoted.numel() < self.n * len(cols)):
                raise MrxError("quoted must be a contiguous uint8[n, f] tensor")
        else:
            prefix, rows, nf = out
        if rows is None or rows.dtype != torch.int32 or not rows.is_contiguous() or rows.numel() < self.n * len(cols) * 2:
            raise MrxError("rows must be a contiguous int32[n, f, 2] tensor")
        if nf is not None and (nf.dtype != torch.int32 or not nf.is_contiguous() or nf.numel() < self.n):
            raise MrxError("nf must be a contiguous int32[n] tensor")
        if prefix is not None and (prefix.dtype != torch.int64 or not prefix.is_contiguous() or prefix.numel() < self.n + 1):
            raise MrxError("prefix must be a contiguous int64[n + 1] tensor")
        if self.n == 0:   # nothing is enqueued, but the columns are still the C side's to refuse (no rows: no address)
            rows = torch.empty(2, dtype=torch.int32, device=self.data.device)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if quote is not None:
            _check(self.call(load_library(), "mrx_fields_quoted", (flags, delim_byte, quote_byte, cols.ctypes.data, len(cols)),
                             (_ptr(rows), _ptr(nf), _ptr(quoted), _ptr(prefix), stream)))
            return
        _check(self.call(load_library(), "mrx_fields", (flags, delim_byte, cols.ctypes.data, len(cols)),
                         (_ptr(rows), _ptr(nf), _ptr(prefix), stream)))

    def translate(self, table=None, delete=b"", squeeze=b""):
        """bytes.translate(table, delete) of every text, then tr -s over the bytes of `squeeze`, as a new batch
        (include/mrx.h, mrx_translate_dev).  table is 256 bytes or None, the identity.  Without delete and squeeze the
        result has this batch's layout -- the same offsets tensor, or the same pitch, length and lens -- and its known
        bounds, and nothing is read back (a CSR batch without known bounds pays the read-back of its first and last
        offset; the padding of fixed-pitch rows is unspecified in the result).  With delete or squeeze the result is a
        packed CSR batch with exact known bounds, its bytes and its longest text: this batch's byte count is capacity
        enough, so the call never retries and reads the two totals back once.  delete together with squeeze is
        refused: call twice."""
        import torch
        dev = self.data.device
        args = _translate_args(table, delete, squeeze)
        if not (delete or squeeze):
            out = torch.empty_like(self.data)
            self.translate_async((out, None, None), table)
            if self.offsets is not None:
                res = DeviceBatch(out, self.offsets)
                res._end_offset, res._max_len = self._end_offset, self._max_len
                return res
            return DeviceBatch(out, None, stride=self.stride, length=self.length, lens=self.lens, n=self.n)
        cap = int(self.data.numel())
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        out_offsets = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
        d_totals = torch.empty(2, dtype=torch.int64, device=dev)
        totals = (C.c_int64 * 2)()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(self.call(load_library(), "mrx_translate", args,
                         (_ptr(out), cap, _ptr(out_offsets), _ptr(d_totals), C.cast(totals, C.c_void_p), stream)))
        nb = int(totals[0])
        res = DeviceBatch(out[:nb].clone() if 4 * nb < cap else out[:nb], out_offsets)
        res._end_offset, res._max_len = nb, int(totals[1])
        return res

    def translate_async(self, out, table=None, delete=b"", squeeze=b""):
        """Enqueue translate() on the current stream without reading its result back.  out = (out_data uint8[out_cap],
        out_offsets int64[n + 1], totals int64[2]) device tensors of the caller; totals = {bytes, longest text} once
        the stream has drained, and no byte is written when bytes > out_cap.  Without delete and squeeze out_offsets
        and totals may be None and are not written: byte p of this batch's data goes to byte p of out_data.  A CSR
        batch without known bounds still pays the read-back of its first and last offset."""
        import torch
        args = _translate_args(table, delete, squeeze)
        out_data, out_offsets, totals = out
        if out_data is None or out_data.dtype != torch.uint8 or not out_data.is_contiguous():
            raise MrxError("out_data must be a contiguous uint8 tensor")
        for t, need in ((out_offsets, self.n + 1), (totals, 2)):
            if t is None and not (delete or squeeze):
                continue
            if t is None or t.dtype != torch.int64 or not t.is_contiguous() or t.numel() < need:
                raise MrxError("out needs out_data uint8[out_cap], out_offsets int64[n + 1], totals int64[2]")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        src = self
        if not (delete or squeeze) and self.offsets is not None and (self._end_offset or 0) > self.data.numel():
            # The same-length form tells from end_offset whether the region fits out_data (include/mrx.h), so a loose
            # bound would be refused as a capacity; offsets[n] never exceeds the data's size, which is a bound as good.
            src = DeviceBatch.csr_known(self.data, self.offsets, int(self.data.numel()), self._max_len)
        _check(src.call(load_library(), "mrx_translate", args,
                        (_ptr(out_data), int(out_data.numel()), _ptr(out_offsets), _ptr(totals), None, stream)))

    def lower(self):
        """bytes.lower() of every text: the ASCII letters, as Python's (translate with its table)."""
        return self.translate(_LOWER)

    def upper(self):
        """bytes.upper() of every text: the ASCII letters, as Python's."""
        return self.translate(_UPPER)

    def strip(self, chars=None, left: bool = True, right: bool = True, spans: bool = False):
        """bytes.strip(chars) of every text (lstrip with right=False, rstrip with left=False) as a new packed batch:
        strip's rows (include/mrx.h, mrx_strip_dev), then gather_spans.  chars=None strips the six whitespace bytes.
        spans=True returns (prefix int64[n + 1], rows int32[n, 1, 2]) instead, device tensors that go to gather_spans,
        parse_spans and expand_spans as they stand; that form enqueues and reads nothing back."""
        import torch
        dev = self.data.device
        rows = torch.empty((self.n, 1, 2), dtype=torch.int32, device=dev)
        # n == 0 enqueues nothing: the one entry of the prefix is the host's to write
        prefix = torch.empty(self.n + 1, dtype=torch.int64, device=dev) if self.n else torch.zeros(1, dtype=torch.int64, device=dev)
        self.strip_async((prefix, rows), chars, left, right)
        if spans:
            return prefix, rows
        return self.gather_spans(prefix, rows)[0]

    def strip_async(self, out, chars=None, left: bool = True, right: bool = True):
        """strip(spans=True) on the caller's tensors out = (prefix int64[n + 1] or None, rows int32[n, 1, 2]): enqueues
        on the current stream and returns.  Nothing is written for a batch without texts."""
        import torch
        prefix, rows = out
        if rows is None or rows.dtype != torch.int32 or not rows.is_contiguous() or rows.numel() < self.n * 2:
            raise MrxError("rows must be a contiguous int32[n, 1, 2] tensor")
        if prefix is not None and (prefix.dtype != torch.int64 or not prefix.is_contiguous() or prefix.numel() < self.n + 1):
            raise MrxError("prefix must be a contiguous int64[n + 1] tensor")
        if self.n == 0:   # nothing is enqueued, but the flags are still the C side's to refuse (no rows: no address)
            rows = torch.empty(2, dtype=torch.int32, device=self.data.device)
        chars_set = None if chars is None else _byte_set(chars)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(self.call(load_library(), "mrx_strip", (chars_set, _strip_flags(left, right)), (_ptr(rows), _ptr(prefix), stream)))

    def cut(self, columns, delim=None, out_delim=None, end=b"\n", quote=None):
        """cut -d<delim> -f<columns>, or awk '{print $a, $b}' with delim=None: one record per text, the named columns
        joined by out_delim (default: delim, or one space in whitespace mode) and closed by `end`, as a new packed
        batch: (records DeviceBatch, owner int64[n]).  This is fields() followed by expand_spans() with the template
        \\1<out_delim>\\2...<end>, so a column that a text does not have contributes nothing, and at most 9 columns
        can be named: expand's templates know \\1 .. \\9 only.  With quote the columns are those of fields(quote=)
        and the records hold their contents: outer quotes taken off, doubled quotes as they stand."""
        if len(columns) > 9:
            raise MrxError("cut takes at most 9 columns: it runs expand_spans, whose templates know \\1 .. \\9 only "
                           "(fields() itself takes %d)" % MRX_FIELDS_MAX_COLUMNS)
        sep = _b(out_delim) if out_delim is not None else (_b(delim) if delim is not None else b" ")
        template = sep.join(b"\\" + str(j + 1).encode() for j in range(len(columns))) + _b(end)
        # expand takes a row's last pair for the whole match, which no reference names: one more pair stands there
        prefix, rows = self.fields(list(columns) + [1], delim, counts=False, quote=quote)[:2]
        return self.expand_spans(template, prefix, rows)

    def gather_spans(self, prefix, spans, pair: int = 0, piece_cap: Optional[int] = None, out_cap: Optional[int] = None):
        """The bytes under spans of this batch's texts as a new packed batch (include/mrx.h, mrx_gather_spans_dev):
        (pieces DeviceBatch, owner int64[pieces]).  prefix int64[n + 1] is the CSR of the rows over the texts, spans
        int32[m, 2] (findall, split_dev, a set's findall) or int32[m, g + 1, 2] (captures_all; `pair` picks the pair of
        each row: group j is pair j - 1, the whole match pair g), both device tensors; m = prefix[n].  A pair is clamped
        to its text, so an unset group gives an empty piece.  The result is a CSR batch with known bounds where this
        batch knows its longest text, trimmed as filter's; owner[r] is the text index of piece r.  Without piece_cap /
        out_cap the call grows them as needed (the input's byte count is no bound: overlapping spans are each copied)."""
        import torch
        if spans.dtype != torch.int32 or not spans.is_contiguous() or spans.dim() not in (2, 3) or spans.shape[-1] != 2:
            raise MrxError("spans must be a contiguous int32[m, 2] or int32[m, g + 1, 2] tensor")
        if prefix.dtype != torch.int64 or not prefix.is_contiguous() or prefix.numel() != self.n + 1:
            raise MrxError("prefix must be a contiguous int64[n + 1] tensor")
        row_pairs = int(spans.shape[1]) if spans.dim() == 3 else 1
        lib = load_library()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return _extract_result(self, _grow_call2(
            int(spans.shape[0]) if piece_cap is None else int(piece_cap),
            int(self.data.numel()) if out_cap is None else int(out_cap), self.data.device,
            lambda pb, pcap, out, ocap, d_totals, totals: self.call(
                lib, "mrx_gather_spans", (),
                (_ptr(prefix), _ptr(spans), row_pairs, int(pair), pcap, _ptr(pb[0]), _ptr(pb[1]), _ptr(out), ocap,
                 _ptr(d_totals), totals, stream)),
            grow_pieces=piece_cap is None, grow_out=out_cap is None))

    def expand_spans(self, template, prefix, rows, piece_cap: Optional[int] = None, out_cap: Optional[int] = None):
        """One record per row of captures_all as a new packed batch (include/mrx.h, mrx_expand_spans_dev): (records
        DeviceBatch, owner int64[records]).  `template` is sub's template grammar (only \\1..\\9 are references; every
        other byte is literal); record r is the template with each \\j replaced by group j of row r, clamped to its text
        as gather_spans clamps a pair -- an unset group and a group the rows do not hold contribute nothing.  prefix
        int64[n + 1] is the CSR of the rows over the texts and rows int32[m, g + 1, 2] captures_all's rows (groups 1..g,
        then the match), both device tensors.  Without piece_cap / out_cap the call grows them as needed.  The result
        is a CSR batch, trimmed as filter's, with known bounds where this batch knows its longest text -- and the bound
        on a record is len(template) + references x longest, NOT the input's longest text: that is what the result's
        longest() says."""
        import torch
        template = _b(template)
        if rows.dtype != torch.int32 or not rows.is_contiguous() or rows.dim() != 3 or rows.shape[-1] != 2:
            raise MrxError("rows must be a contiguous int32[m, g + 1, 2] tensor")
        if prefix.dtype != torch.int64 or not prefix.is_contiguous() or prefix.numel() != self.n + 1:
            raise MrxError("prefix must be a contiguous int64[n + 1] tensor")
        lib = load_library()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        m = int(rows.shape[0])
        return _expand_result(self, template, _grow_call2(
            m if piece_cap is None else int(piece_cap),
            max(64, int(self.data.numel()) + m * len(template)) if out_cap is None else int(out_cap), self.data.device,
            lambda pb, pcap, out, ocap, d_totals, totals: self.call(
                lib, "mrx_expand_spans", (),
                (_ptr(prefix), _ptr(rows), int(rows.shape[1]), template, len(template), pcap, _ptr(pb[0]), _ptr(pb[1]),
                 _ptr(out), ocap, _ptr(d_totals), totals, stream)),
            grow_pieces=piece_cap is None, grow_out=out_cap is None))

    def distinct(self, out_cap: Optional[int] = None):
        """The unique texts of this batch and how often each occurs (include/mrx.h, mrx_distinct_dev): (values
        DeviceBatch, counts int64[u], group_of int64[n], first int64[u]), device tensors.  Texts are equal when their
        lengths and bytes are; the groups are numbered by first occurrence, the order of dict.fromkeys(texts) and of
        collections.Counter(texts).  Value g is text first[g], counts[g] texts equal it, and group_of[i] is the group
        of text i.  `values` is a CSR batch, trimmed by filter's quarter rule as counts and first are, with known bounds
        where this batch knows its longest text.  out_cap defaults to this batch's bytes, which always suffice; a
        smaller one of the caller's that does not hold the values raises MrxError (MRX_E_CAPACITY)."""
        import torch
        dev, n = self.data.device, self.n
        cap = int(self.data.numel()) if out_cap is None else int(out_cap)
        group_of = torch.empty(n, dtype=torch.int64, device=dev)
        first, counts = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        d_totals = torch.empty(2, dtype=torch.int64, device=dev)
        totals = (C.c_int64 * 2)()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(self.call(load_library(), "mrx_distinct", (),
                         (_ptr(group_of), _ptr(first), _ptr(counts), _ptr(out_off), _ptr(out), cap, _ptr(d_totals),
                          C.cast(totals, C.c_void_p), stream)))
        u, nbytes = int(totals[0]), int(totals[1])
        trim_u = (lambda t, m: t[:m].clone()) if 4 * u < n else (lambda t, m: t[:m])
        trim_b = (lambda t, m: t[:m].clone()) if 4 * nbytes < cap else (lambda t, m: t[:m])
        values = DeviceBatch(trim_b(out, nbytes), trim_u(out_off, u + 1))
        longest = self.longest()
        if longest is not None:   # known bounds, as filter's result: a value is one of the texts
            values._end_offset, values._max_len = nbytes, int(longest)
        return values, trim_u(counts, u), group_of, trim_u(first, u)

    def distinct_async(self, out):
        """Enqueue distinct on the current stream without reading anything back.  out = (group_of int64[n], first
        int64[n], counts int64[n], out_offsets int64[n + 1], out_data uint8[cap], totals int64[2]) device tensors of the
        caller; totals = {u, bytes} once the stream has drained.  No byte is written when bytes > cap (check totals[1]);
        cap = this batch's bytes always fits."""
        import torch
        group_of, first, counts, out_offsets, out_data, totals = out
        if (min(group_of.numel(), first.numel(), counts.numel()) < self.n or out_offsets.numel() < self.n + 1
                or totals.numel() < 2):
            raise MrxError("out needs group_of, first and counts int64[n], out_offsets int64[n + 1], out_data uint8[cap], "
                           "totals int64[2]")
        for t in (group_of, first, counts, out_offsets, totals):
            if t.dtype != torch.int64 or not t.is_contiguous():
                raise MrxError("group_of, first, counts, out_offsets and totals must be contiguous int64 tensors")
        if out_data.dtype != torch.uint8 or not out_data.is_contiguous():
            raise MrxError("out_data must be a contiguous uint8 tensor")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(self.call(load_library(), "mrx_distinct", (),
                         (_ptr(group_of), _ptr(first), _ptr(counts), _ptr(out_offsets), _ptr(out_data),
                          int(out_data.numel()), _ptr(totals), None, stream)))

    def argsort(self, rank: bool = False):
        """The stable ascending order of this batch's texts (include/mrx.h, mrx_sort_dev): order int64[n], a device
        tensor with order[p] the index of the text at sorted position p -- sorted(range(n), key=texts.__getitem__).
        Texts compare as Python's bytes do: bytewise and unsigned, a proper prefix first, equal texts in index order.
        With rank=True the result is (order, rank int64[n], distinct_count): rank[i] is the number of different texts
        smaller than text i, the inverse of numpy.unique(texts, return_inverse=True).  The call synchronises the
        stream once per 8-byte refinement round (one or two for typical batches)."""
        import torch
        dev, n = self.data.device, self.n
        order = torch.empty(n, dtype=torch.int64, device=dev)
        ranks = torch.empty(n, dtype=torch.int64, device=dev) if rank else None
        d_totals = torch.empty(1, dtype=torch.int64, device=dev) if rank else None
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(self.call(load_library(), "mrx_sort", (), (_ptr(order), _ptr(ranks), _ptr(d_totals), stream)))
        if not rank:
            return order
        return order, ranks, int(d_totals.item())

    def _check_index(self, index):
        import torch
        if index.dtype != torch.int64 or not index.is_contiguous() or index.dim() != 1 or index.device != self.data.device:
            raise MrxError("index must be a contiguous int64[k] tensor on the data's device")

    def take(self, index, out_cap: Optional[int] = None):
        """The texts at `index` (int64[k], a device tensor; any order, repeats allowed, k may exceed n) as a new packed
        batch (include/mrx.h, mrx_take_dev): text j of the result is text index[j] of this batch.  The result is a CSR
        DeviceBatch with known bounds: its byte count and, where this batch knows it, this batch's longest text.
        Without out_cap the output starts at this batch's byte count and grows when repeats need more; an out_cap of
        the caller's that does not hold the result, and an index outside [0, n), raise MrxError."""
        import torch
        self._check_index(index)
        dev, k = self.data.device, int(index.numel())
        out_off = torch.empty(k + 1, dtype=torch.int64, device=dev)
        d_totals = torch.empty(2, dtype=torch.int64, device=dev)
        totals = (C.c_int64 * 2)()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        lib = load_library()

        def run(out, cap, total):
            rc = self.call(lib, "mrx_take", (), (_ptr(index), k, _ptr(out_off), _ptr(out), cap, _ptr(d_totals),
                                                 C.cast(totals, C.c_void_p), stream))
            total._obj.value = int(totals[1])
            return rc
        out, nbytes = _grow_call(int(self.data.numel()) if out_cap is None else int(out_cap),
                                 lambda cap: torch.empty(max(cap, 1), dtype=torch.uint8, device=dev), run,
                                 grow=out_cap is None, only_larger=True)
        taken = DeviceBatch(out[:nbytes].clone() if 4 * nbytes < out.numel() else out[:nbytes], out_off)
        longest = self.longest()
        if longest is not None:   # known bounds, as filter's result: a taken text is one of the texts
            taken._end_offset, taken._max_len = nbytes, int(longest)
        return taken

    def take_async(self, index, out):
        """Enqueue take on the current stream without reading anything back.  out = (out_offsets int64[k + 1], out_data
        uint8[cap], totals int64[2]) device tensors of the caller; totals = {k, bytes} once the stream has drained, or
        {-1, -1} when an index lies outside [0, n).  No byte is written when bytes > cap (check totals[1])."""
        import torch
        self._check_index(index)
        out_offsets, out_data, totals = out
        k = int(index.numel())
        if out_offsets.numel() < k + 1 or totals.numel() < 2:
            raise MrxError("out needs out_offsets int64[k + 1], out_data uint8[cap], totals int64[2]")
        for t in (out_offsets, totals):
            if t.dtype != torch.int64 or not t.is_contiguous():
                raise MrxError("out_offsets and totals must be contiguous int64 tensors")
        if out_data.dtype != torch.uint8 or not out_data.is_contiguous():
            raise MrxError("out_data must be a contiguous uint8 tensor")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(self.call(load_library(), "mrx_take", (),
                         (_ptr(index), k, _ptr(out_offsets), _ptr(out_data), int(out_data.numel()), _ptr(totals), None,
                          stream)))

    def sort(self):
        """(sorted_batch, order): this batch's texts in ascending order as a new packed batch -- take(argsort()) -- and
        the permutation that made it."""
        order = self.argsort()
        return self.take(order), order

    def parse(self, kind: str = "int", fill=0):
        """Every text of this batch as a number (include/mrx.h, mrx_parse_dev): (values, status), device tensors.  kind
        is "int" ([+-]?[0-9]+), "hex" ([+-]?(0[xX])?[0-9a-fA-F]+) or "float" ([+-]?([0-9]+\\.?[0-9]*|\\.[0-9]+)
        ([eE][+-]?[0-9]+)?); a text is parsed as a whole.  values is int64[n], or float64[n] for "float"; status is
        uint8[n]: 0 = a number, 1 = an empty text, 2 = outside the grammar, 3 = well-formed but not answered (an integer
        outside int64; a float that the exact rule does not cover).  Rows that are not numbers hold `fill`.  Enqueues on
        the current stream and reads nothing back."""
        import torch
        k, word = _num_kind(kind), _num_fill(kind, fill)
        values = torch.empty(self.n, dtype=torch.int64, device=self.data.device)
        status = torch.empty(self.n, dtype=torch.uint8, device=self.data.device)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(self.call(load_library(), "mrx_parse", (), (k, word, _ptr(values), _ptr(status), stream)))
        return (values.view(torch.float64) if kind == "float" else values), status

    def parse_spans(self, prefix, spans, pair: int = 0, kind: str = "int", fill=0):
        """The bytes under spans of this batch's texts as numbers, read where they lie (include/mrx.h,
        mrx_parse_spans_dev): (values, status, owner), device tensors with one row per row of `spans`.  prefix, spans
        and pair are gather_spans' own -- prefix int64[n + 1] the CSR of the rows over the texts, spans int32[m, 2] or
        int32[m, g + 1, 2] with m = prefix[n] -- and a pair is clamped to its text in the same way, so an unset group is
        an empty piece (status 1).  kind, fill, values and status are parse's; owner int64[m] is the text index of each
        row.  The row count is the spans tensor's own: the call enqueues on the current stream and reads nothing back."""
        import torch
        if spans.dtype != torch.int32 or not spans.is_contiguous() or spans.dim() not in (2, 3) or spans.shape[-1] != 2:
            raise MrxError("spans must be a contiguous int32[m, 2] or int32[m, g + 1, 2] tensor")
        if prefix.dtype != torch.int64 or not prefix.is_contiguous() or prefix.numel() != self.n + 1:
            raise MrxError("prefix must be a contiguous int64[n + 1] tensor")
        k, word = _num_kind(kind), _num_fill(kind, fill)
        row_pairs = int(spans.shape[1]) if spans.dim() == 3 else 1
        dev, m = self.data.device, int(spans.shape[0])
        values = torch.empty(m, dtype=torch.int64, device=dev)
        status = torch.empty(m, dtype=torch.uint8, device=dev)
        owner = torch.empty(m, dtype=torch.int64, device=dev)
        d_totals = torch.empty(1, dtype=torch.int64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(self.call(load_library(), "mrx_parse_spans", (),
                         (_ptr(prefix), _ptr(spans), row_pairs, int(pair), k, word, m, _ptr(values), _ptr(status),
                          _ptr(owner), _ptr(d_totals), None, stream)))
        return (values.view(torch.float64) if kind == "float" else values), status, owner


MRX_NUM_INT10, MRX_NUM_INT16, MRX_NUM_FLOAT = range(3)
MRX_NUM_OK, MRX_NUM_EMPTY, MRX_NUM_MALFORMED, MRX_NUM_RANGE = range(4)
_NUM_KINDS = {"int": MRX_NUM_INT10, "hex": MRX_NUM_INT16, "float": MRX_NUM_FLOAT}


def _num_kind(kind: str) -> int:
    if kind not in _NUM_KINDS:
        raise MrxError("kind must be 'int', 'hex' or 'float'")
    return _NUM_KINDS[kind]


def _num_fill(kind: str, fill) -> int:
    """The 64-bit word stored in a row that is not a number: an int as it is, for "float" the bits of float(fill)."""
    if kind == "float":
        return int(np.array([fill], np.float64).view(np.int64)[0])
    fill = int(fill)
    if not -(1 << 63) <= fill < (1 << 63):
        raise MrxError("fill must fit an int64")
    return fill


def _num_lists(kind: str, values, status, prefix=None):
    """Host lists from values and status (device tensors): the number, or None where the status is not OK; with the
    CSR of the rows over the texts, one list per text."""
    conv = float if kind == "float" else int
    flat = [conv(v) if s == MRX_NUM_OK else None for v, s in zip(values.cpu().numpy().tolist(), status.cpu().numpy().tolist())]
    if prefix is None:
        return flat
    prefix = prefix.cpu().numpy()
    return [flat[prefix[i]:prefix[i + 1]] for i in range(len(prefix) - 1)]


def _sort_counts(values: "DeviceBatch", counts, sort: Optional[str], top: Optional[int]):
    """The rows (values, counts) of distinct in another order: None = as they are (first occurrence), "value" =
    ascending by value, "count" = descending by count with ties in first-occurrence order (Counter.most_common);
    top = k keeps the first k rows of that order."""
    order = _row_order(values, counts, sort, top)
    return (values, counts) if order is None else (values.take(order), counts[order])


def _row_order(values: "DeviceBatch", counts, sort: Optional[str], top: Optional[int]):
    """The rows of distinct that _sort_counts keeps, in its order, as an int64 device tensor; None = all, as they are."""
    import torch
    if sort not in (None, "value", "count"):
        raise MrxError("sort must be None, 'value' or 'count'")
    if top is not None and int(top) < 0:
        raise MrxError("top must be >= 0")
    if sort is None and (top is None or int(top) >= values.n):
        return None
    if sort == "value":
        order = values.argsort()
    elif sort == "count":
        order = torch.sort(counts, descending=True, stable=True)[1]
    else:
        order = torch.arange(values.n, dtype=torch.int64, device=counts.device)
    return order if top is None else order[:int(top)].contiguous()


def _ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


_NO_BYTES = {}


def _no_bytes(device):
    """16 zero bytes on `device`, allocated once: the data pointer of a batch whose texts hold no byte."""
    import torch
    if device not in _NO_BYTES:
        _NO_BYTES[device] = torch.zeros(16, dtype=torch.uint8, device=device)
    return _NO_BYTES[device]


def _grow_call(cap, alloc, call, grow=True, only_larger=False):
    """Allocate alloc(cap), rc = call(buffers, cap, byref(total)); on MRX_E_CAPACITY grow to the reported total and
    repeat -- if `grow` (a caller's own capacity is not outgrown) and, with only_larger, only when the total exceeds
    the capacity.  Returns (buffers, total)."""
    while True:
        bufs = alloc(cap)
        total = C.c_int64(0)
        rc = call(bufs, cap, C.byref(total))
        if rc == MRX_E_CAPACITY and grow and (not only_larger or int(total.value) > cap):
            cap = int(total.value)
            continue
        _check(rc)
        return bufs, int(total.value)


def _grow_call2(piece_cap, out_cap, dev, call, grow_pieces=True, grow_out=True):
    """_grow_call for the two capacities of extract: (owner int64[piece_cap], out_offsets int64[piece_cap + 1]) and
    out_data uint8[out_cap] on `dev`; rc = call(piece_bufs, piece_cap, out_data, out_cap, d_totals, totals).  On
    MRX_E_CAPACITY the short capacity grows to the reported need -- first the pieces (the bytes are not known before
    they fit), then the bytes, so at most two retries -- unless it is the caller's own.  Returns (owner, out_offsets,
    out_data, piece_cap, out_cap, pieces, bytes)."""
    import torch
    d_totals = torch.empty(2, dtype=torch.int64, device=dev)
    totals = (C.c_int64 * 2)()
    pb = out = None
    while True:
        if pb is None:
            pb = (torch.empty(max(piece_cap, 1), dtype=torch.int64, device=dev),
                  torch.empty(piece_cap + 1, dtype=torch.int64, device=dev))
        if out is None:
            out = torch.empty(max(out_cap, 1), dtype=torch.uint8, device=dev)
        rc = call(pb, piece_cap, out, out_cap, d_totals, C.cast(totals, C.c_void_p))
        if rc == MRX_E_CAPACITY and grow_pieces and int(totals[0]) > piece_cap:
            piece_cap, pb = int(totals[0]), None
            continue
        if rc == MRX_E_CAPACITY and grow_out and int(totals[0]) <= piece_cap and int(totals[1]) > out_cap:
            out_cap, out = int(totals[1]), None
            continue
        _check(rc)
        return pb[0], pb[1], out, piece_cap, out_cap, int(totals[0]), int(totals[1])


def _extract_result(batch: "DeviceBatch", grown):
    """(pieces DeviceBatch, owner) from _grow_call2's buffers, each trimmed by filter's quarter rule: a result that
    uses less than a quarter of its buffer is copied out, above that the views are returned as they are."""
    owner, out_off, out, piece_cap, out_cap, pieces, nbytes = grown
    trim_p = (lambda t, m: t[:m].clone()) if 4 * pieces < piece_cap else (lambda t, m: t[:m])
    trim_b = (lambda t, m: t[:m].clone()) if 4 * nbytes < out_cap else (lambda t, m: t[:m])
    res = DeviceBatch(trim_b(out, nbytes), trim_p(out_off, pieces + 1))
    longest = batch.longest()
    if longest is not None:   # known bounds, as filter's result: no piece is longer than its text
        res._end_offset, res._max_len = nbytes, int(longest)
    return res, trim_p(owner, pieces)


def _template_ref_list(template: bytes) -> List[int]:
    """The references of a template, in order: the j of each \\1..\\9 of sub's grammar (parse_repl_template scans left to
    right and passes both bytes of a reference)."""
    refs, i = [], 0
    while i + 1 < len(template):
        if template[i] == 0x5C and 0x31 <= template[i + 1] <= 0x39:
            refs.append(template[i + 1] - 0x30)
            i += 2
        else:
            i += 1
    return refs


def _template_refs(template: bytes) -> int:
    """How many references a template has."""
    return len(_template_ref_list(template))


def _expand_result(batch: "DeviceBatch", template: bytes, grown):
    """_extract_result for expand: a record is at most len(template) + references x the longest text long."""
    res, owner = _extract_result(batch, grown)
    if res._max_len is not None:
        res._max_len = len(template) + _template_refs(template) * res._max_len
    return res, owner


def _piece_lists(pieces: "DeviceBatch", prefix) -> List[List[bytes]]:
    """Host lists from a pieces batch and the CSR of the pieces over the texts (a device tensor or numpy)."""
    raw = pieces.data.cpu().numpy().tobytes()
    off = pieces.offsets.cpu().numpy()
    prefix = prefix if isinstance(prefix, np.ndarray) else prefix.cpu().numpy()
    return [[raw[off[r]:off[r + 1]] for r in range(prefix[i], prefix[i + 1])] for i in range(len(prefix) - 1)]


MRX_FILTER_INVERT, MRX_FILTER_ALL = 1, 2
MRX_LINES_KEEPENDS, MRX_LINES_CRLF, MRX_LINES_DROP_PARTIAL = 1, 2, 4


def _lines_flags(sep, keepends: bool, crlf: bool, partial: bool) -> Tuple[int, int]:
    """(flags, separator byte) of mrx_lines_*; which combinations are refused is the C side's to say."""
    sep = _b(sep)
    if len(sep) != 1:
        raise MrxError("sep must be a single byte: compile_regex(sep).split_batch cuts at longer separators")
    return ((MRX_LINES_KEEPENDS if keepends else 0) | (MRX_LINES_CRLF if crlf else 0) |
            (0 if partial else MRX_LINES_DROP_PARTIAL)), sep[0]


MRX_FIELDS_WHITESPACE, MRX_FIELDS_REST = 1, 2
MRX_FIELDS_MAX_COLUMNS = 32


MRX_STRIP_LEFT, MRX_STRIP_RIGHT = 1, 2
_LOWER = bytes(range(256)).lower()
_UPPER = bytes(range(256)).upper()


def _byte_set(members) -> bytes:
    """The 32-byte bitmap of include/mrx.h over the bytes of `members`."""
    bits = bytearray(32)
    for c in _b(members):
        bits[c >> 3] |= 1 << (c & 7)
    return bytes(bits)


def _translate_args(table=None, delete=b"", squeeze=b""):
    """(table, delete set, squeeze set) of mrx_translate_*, each None where empty.  What the C side refuses too is refused
    here first, so that the host-list forms say so before they upload."""
    table = None if table is None else _b(table)
    if table is not None and len(table) != 256:
        raise MrxError("table must be 256 bytes (or None, the identity)")
    if delete and squeeze:
        raise MrxError("delete and squeeze in one call: translate twice")
    return table, _byte_set(delete) if delete else None, _byte_set(squeeze) if squeeze else None


def _strip_flags(left: bool, right: bool) -> int:
    """flags of mrx_strip_*; neither side is the C side's to refuse."""
    return (MRX_STRIP_LEFT if left else 0) | (MRX_STRIP_RIGHT if right else 0)


def _fields_args(columns, delim, rest: bool):
    """(flags, delimiter byte, columns as int32 array) of mrx_fields_*; which columns are refused is the C side's to say."""
    flags = MRX_FIELDS_REST if rest else 0
    if delim is None:
        flags, delim_byte = flags | MRX_FIELDS_WHITESPACE, 0
    else:
        delim = _b(delim)
        if len(delim) != 1:
            raise MrxError("delim must be a single byte (or None for whitespace): compile_regex(delim).split_dev cuts "
                           "at longer delimiters")
        delim_byte = delim[0]
    cols = [int(c) for c in columns]
    if any(not -(1 << 31) <= c < (1 << 31) for c in cols):
        raise MrxError("a column must fit an int32")
    return flags, delim_byte, np.array(cols, dtype=np.int32)


def _quote_byte(quote) -> int:
    """The quote byte of mrx_fields_quoted_*; which bytes a mode refuses is the C side's to say."""
    quote = _b(quote)
    if len(quote) != 1:
        raise MrxError("quote must be a single byte")
    return quote[0]


def _filter_flags(mode: str = "any", invert: bool = False) -> int:
    if mode not in ("any", "all"):
        raise MrxError("mode must be 'any' or 'all'")
    return (MRX_FILTER_INVERT if invert else 0) | (MRX_FILTER_ALL if mode == "all" else 0)


def _filter(lib, stem: str, handle, flags: int, texts, extra=()):
    """filter of one pattern (stem "mrx_filter"), a set ("mrx_set_filter") or a dictionary ("mrx_dict_filter", a
    DeviceBatch only; `extra`: its d_index, in front of the outputs).  The capacity is the input's byte count, which
    always suffices, so there is no retry."""
    if isinstance(texts, DeviceBatch):
        import torch
        batch, dev, n = texts, texts.data.device, texts.n
        cap = int(batch.data.numel())
        out = (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev),
               torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(2, dtype=torch.int64, device=dev))
        totals = (C.c_int64 * 2)()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(batch.call(lib, stem, (handle, flags), extra + (_ptr(out[0]), _ptr(out[1]), _ptr(out[2]), cap, _ptr(out[3]),
                                                               C.cast(totals, C.c_void_p), stream)))
        kept, nbytes = int(totals[0]), int(totals[1])
        longest = batch.longest()
        # The outputs were allocated for the worst case (every text kept).  A result that uses less than a quarter
        # of them is copied out, so that a sparse filter does not pin the input's size for the result's lifetime;
        # above that the views are returned as they are (at most four times the result's own bytes stay allocated).
        trim = (lambda t, m: t[:m].clone()) if 4 * nbytes < cap else (lambda t, m: t[:m])
        kept_batch = DeviceBatch(trim(out[2], nbytes), trim(out[1], kept + 1))
        if longest is not None:   # known bounds: a following findall / sub / filter needs no read-back for them
            kept_batch._end_offset, kept_batch._max_len = nbytes, int(longest)
        return kept_batch, trim(out[0], kept)
    bs = [_b(t) for t in texts]
    data, offsets = pack_texts(bs)
    n = len(bs)
    idx = np.zeros(max(n, 1), np.int64)
    out_off = np.zeros(n + 1, np.int64)
    out = np.empty(max(int(offsets[-1]), 1), np.uint8)
    totals = (C.c_int64 * 2)()
    _check(getattr(lib, stem + "_batch")(handle, flags, data.ctypes.data, offsets.ctypes.data, n, idx.ctypes.data,
                                         out_off.ctypes.data, out.ctypes.data, int(offsets[-1]),
                                         C.cast(totals, C.c_void_p)))
    kept = int(totals[0])
    raw = out[:int(totals[1])].tobytes()
    return [raw[out_off[r]:out_off[r + 1]] for r in range(kept)], idx[:kept].copy()


def _filter_async(lib, stem: str, handle, flags: int, batch: "DeviceBatch", out, extra=()):
    import torch
    kept_idx, out_offsets, out_data, totals = out
    if kept_idx.numel() < batch.n or out_offsets.numel() < batch.n + 1 or totals.numel() < 2:
        raise MrxError("out needs kept_idx int64[n], out_offsets int64[n + 1], out_data uint8[cap], totals int64[2]")
    for t in (kept_idx, out_offsets, totals):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise MrxError("kept_idx, out_offsets and totals must be contiguous int64 tensors")
    if out_data.dtype != torch.uint8 or not out_data.is_contiguous():
        raise MrxError("out_data must be a contiguous uint8 tensor")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _check(batch.call(lib, stem, (handle, flags), extra + (_ptr(kept_idx), _ptr(out_offsets), _ptr(out_data),
                                                           int(out_data.numel()), _ptr(totals), None, stream)))


class Dictionary:
    """A fixed set of texts, the entries, built once on the device and probed by any number of batches (include/mrx.h,
    "dictionaries"): grep -F -x -f list, isin, vocab.index(token).  `entries` is a list of texts or a DeviceBatch; the
    handle keeps its own copy, so the batch may be dropped afterwards.  Texts are equal when their lengths and bytes are;
    duplicates among the entries are allowed and the lowest index stands for them.  len() is the number of entries."""

    def __init__(self, entries):
        import torch
        self._lib = load_library()
        batch = entries if isinstance(entries, DeviceBatch) else DeviceBatch.from_texts([_b(t) for t in entries])
        h = C.c_void_p()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(batch.call(self._lib, (self._lib.mrx_dict_build_dev, self._lib.mrx_dict_build_strided_dev), (),
                          (stream, C.byref(h))))
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.mrx_dict_free(self._h)
                self._h = None
        except Exception:
            pass

    def __len__(self) -> int:
        return int(self._lib.mrx_dict_size(self._h))

    @property
    def distinct_count(self) -> int:
        """How many of the entries are different."""
        return int(self._lib.mrx_dict_distinct(self._h))

    def lookup_async(self, batch: "DeviceBatch", out):
        """Enqueue the lookup on the current stream: out int64[n], a device tensor of the caller, receives for every
        text the lowest index of an entry equal to it, or -1.  Nothing is read back."""
        import torch
        if out.dtype != torch.int64 or not out.is_contiguous() or out.numel() < batch.n:
            raise MrxError("out must be a contiguous int64[n] tensor")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(batch.call(self._lib, (self._lib.mrx_dict_lookup_dev, self._lib.mrx_dict_lookup_strided_dev), (self._h,),
                          (_ptr(out), stream)))

    def lookup(self, texts):
        """For every text the lowest index of an entry equal to it, or -1: np.int64[n] for a list of texts, a device
        int64 tensor for a DeviceBatch (enqueued on the current stream, nothing read back)."""
        import torch
        if isinstance(texts, DeviceBatch):
            out = torch.empty(texts.n, dtype=torch.int64, device=texts.data.device)
            self.lookup_async(texts, out)
            return out
        batch = DeviceBatch.from_texts([_b(t) for t in texts])
        return self.lookup(batch).cpu().numpy()

    def isin(self, texts):
        """bool[n]: is text i an entry?  numpy for a list of texts, a device tensor for a DeviceBatch."""
        return self.lookup(texts) >= 0

    def filter(self, texts, invert: bool = False):
        """The texts that are entries (with invert, the others) as a new packed batch, in their order: what
        CompiledRegex.filter returns, with the same known bounds and the same trimming (include/mrx.h,
        mrx_dict_filter_dev).  A list of texts gives (kept List[bytes], idx numpy int64[kept]), a DeviceBatch gives
        (DeviceBatch, idx) with device tensors."""
        if isinstance(texts, DeviceBatch):
            return _filter(self._lib, "mrx_dict_filter", self._h, _filter_flags("any", invert), texts, extra=(None,))
        bs = [_b(t) for t in texts]
        kept, idx = self.filter(DeviceBatch.from_texts(bs), invert)
        idx = idx.cpu().numpy()
        return [bs[int(i)] for i in idx], idx

    def filter_async(self, batch: "DeviceBatch", out, invert: bool = False, index=None):
        """Enqueue the filter on the current stream without reading anything back: out as CompiledRegex.filter_async's
        (kept_idx int64[n], out_offsets int64[n + 1], out_data uint8[cap], totals int64[2]).  index int64[n] (optional,
        a device tensor) also receives the lookup result of every input text."""
        import torch
        if index is not None and (index.dtype != torch.int64 or not index.is_contiguous() or index.numel() < batch.n):
            raise MrxError("index must be a contiguous int64[n] tensor")
        _filter_async(self._lib, "mrx_dict_filter", self._h, _filter_flags("any", invert), batch, out, extra=(_ptr(index),))


MRX_SORTED_EQUAL = 0
MRX_SORTED_PREFIX = 1
MRX_SORTED_LONGEST = 2
_SORTED_MODES = {"equal": MRX_SORTED_EQUAL, "prefix": MRX_SORTED_PREFIX, "longest": MRX_SORTED_LONGEST}


class SortedIndex:
    """A batch of texts, the entries, kept in sorted order on the device and searched by any number of batches
    (include/mrx.h, "sorted index"): bisect.bisect_left / bisect_right, the range of entries that begin with a text, and
    the longest entry that is a prefix of a text.  `entries` is a list of texts or a DeviceBatch in any layout; the
    handle keeps its own sorted copy.  The order is sort's: bytewise, unsigned, a proper prefix first, equal entries in
    ascending original index.  Positions are positions 0..len() in that order; order[p] is the original index of the entry
    at position p.  A DeviceBatch of texts gives device tensors, a list gives numpy arrays."""

    def __init__(self, entries):
        import torch
        self._lib = load_library()
        batch = entries if isinstance(entries, DeviceBatch) else DeviceBatch.from_texts([_b(t) for t in entries])
        h = C.c_void_p()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(batch.call(self._lib, (self._lib.mrx_sorted_build_dev, self._lib.mrx_sorted_build_strided_dev), (),
                          (stream, C.byref(h))))
        self._h = h
        self._entries = batch   # for `values` only: the handle searches its own copy
        self._order = None
        self._values = None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.mrx_sorted_free(self._h)
                self._h = None
        except Exception:
            pass

    def __len__(self) -> int:
        return int(self._lib.mrx_sorted_size(self._h))

    @property
    def distinct_count(self) -> int:
        """How many of the entries are different."""
        return int(self._lib.mrx_sorted_distinct(self._h))

    @property
    def order(self):
        """int64[m], a device tensor: order[p] is the original index of the entry at sorted position p (fetched once)."""
        if self._order is None:
            import torch
            order = torch.empty(len(self), dtype=torch.int64, device=self._entries.data.device)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _check(self._lib.mrx_sorted_order_dev(self._h, _ptr(order), stream))
            self._order = order
        return self._order

    @property
    def values(self) -> "DeviceBatch":
        """The sorted entries as a DeviceBatch: entries.take(order), made on first use."""
        if self._values is None:
            self._values = self._entries.take(self.order)
        return self._values

    def search_async(self, batch: "DeviceBatch", mode, lo, hi):
        """Enqueue a search on the current stream: mode is "equal", "prefix" or "longest" (or its MRX_SORTED_ value), lo
        and hi int64[n] device tensors of the caller (either may be None, not both).  Nothing is read back."""
        import torch
        for t in (lo, hi):
            if t is not None and (t.dtype != torch.int64 or not t.is_contiguous() or t.numel() < batch.n):
                raise MrxError("lo and hi must be contiguous int64[n] tensors")
        if lo is None and hi is None:
            raise MrxError("give lo, hi or both")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(batch.call(self._lib, (self._lib.mrx_sorted_search_dev, self._lib.mrx_sorted_search_strided_dev),
                          (self._h, int(_SORTED_MODES.get(mode, mode))), (_ptr(lo), _ptr(hi), stream)))

    def _search(self, texts, mode: int, want_lo: bool = True, want_hi: bool = True):
        import torch
        if not isinstance(texts, DeviceBatch):
            got = self._search(DeviceBatch.from_texts([_b(t) for t in texts]), mode, want_lo, want_hi)
            return tuple(None if t is None else t.cpu().numpy() for t in got)
        lo = torch.empty(texts.n, dtype=torch.int64, device=texts.data.device) if want_lo else None
        hi = torch.empty(texts.n, dtype=torch.int64, device=texts.data.device) if want_hi else None
        self.search_async(texts, mode, lo, hi)
        return lo, hi

    def searchsorted(self, texts, side: str = "left"):
        """bisect.bisect_left (side="left") or bisect_right (side="right") of every text among the sorted entries:
        int64[n]."""
        if side not in ("left", "right"):
            raise MrxError("side must be 'left' or 'right'")
        return self._search(texts, MRX_SORTED_EQUAL, side == "left", side == "right")[side == "right"]

    def equal_range(self, texts):
        """(lo, hi): the entries equal to text i stand at positions [lo[i], hi[i]); lo == hi is the insertion point."""
        return self._search(texts, MRX_SORTED_EQUAL)

    def prefix_range(self, texts):
        """(lo, hi): exactly the positions [lo[i], hi[i]) hold the entries that begin with text i."""
        return self._search(texts, MRX_SORTED_PREFIX)

    def longest_prefix(self, texts, lengths: bool = False):
        """The lowest position of the longest entry that is a prefix of text i, or -1; with lengths=True, (positions,
        lengths of those entries or -1)."""
        pos, length = self._search(texts, MRX_SORTED_LONGEST, True, lengths)
        return (pos, length) if lengths else pos

    def index(self, texts):
        """The lowest original index of an entry equal to text i, or -1: what Dictionary.lookup answers."""
        import torch
        if not isinstance(texts, DeviceBatch):
            return self.index(DeviceBatch.from_texts([_b(t) for t in texts])).cpu().numpy()
        lo, hi = self.equal_range(texts)
        if len(self) == 0:
            return torch.full_like(lo, -1)
        return torch.where(lo < hi, self.order[lo.clamp(max=len(self) - 1)], torch.full_like(lo, -1))


MRX_KW_IGNORE_CASE = 1


class Keywords:
    """A fixed list of literals, the entries, searched for INSIDE every text in one pass (include/mrx.h, "keywords"):
    grep -F -f list, keyword tagging.  `entries` is a list of byte strings or a DeviceBatch; the handle keeps its own
    automaton, so the entries may be dropped afterwards.  Every occurrence is a hit, overlapping and nested ones
    included; equal entries share the lowest index among them; an empty entry is refused.  With ignore_case ASCII A-Z
    are folded onto a-z in the entries and in the texts.  len() is the number of entries."""

    def __init__(self, entries, ignore_case: bool = False):
        self._lib = load_library()
        flags = MRX_KW_IGNORE_CASE if ignore_case else 0
        h = C.c_void_p()
        if isinstance(entries, DeviceBatch) and entries.offsets is not None:
            import torch
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _check(self._lib.mrx_kw_build_dev(_ptr(entries.data), _ptr(entries.offsets), entries.n, flags, stream,
                                              C.byref(h)))
        else:
            if isinstance(entries, DeviceBatch):   # a fixed pitch: the build runs on the host anyway
                rows = entries.data.cpu().numpy().reshape(entries.n, entries.stride)
                lens = entries.lens.cpu().numpy() if entries.lens is not None else [entries.length] * entries.n
                entries = [rows[j, :int(lens[j])].tobytes() for j in range(entries.n)]
            data, offsets = pack_texts(entries)
            _check(self._lib.mrx_kw_build(data.ctypes.data, offsets.ctypes.data, len(offsets) - 1, flags, None,
                                          C.byref(h)))
        self._h = h
        self._hits_per_byte = 0.0

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.mrx_kw_free(self._h)
                self._h = None
        except Exception:
            pass

    def __len__(self) -> int:
        return int(self._lib.mrx_kw_size(self._h))

    @property
    def distinct_count(self) -> int:
        """How many of the entries are different (after folding, with ignore_case)."""
        return int(self._lib.mrx_kw_distinct(self._h))

    def describe(self) -> str:
        """m, distinct entries, states, byte classes, the longest entry and the table's bytes."""
        need = self._lib.mrx_kw_describe(self._h, None, 0)
        buf = C.create_string_buffer(need + 1)
        self._lib.mrx_kw_describe(self._h, buf, need + 1)
        return buf.value.decode("utf-8", "replace")

    def _per_text(self, op: str, dtype, texts):
        import torch
        host = not isinstance(texts, DeviceBatch)
        batch = DeviceBatch.from_texts([_b(t) for t in texts]) if host else texts
        out = torch.empty(batch.n, dtype=dtype, device=batch.data.device)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(batch.call(self._lib, (getattr(self._lib, op + "_dev"), getattr(self._lib, op + "_strided_dev")),
                          (self._h,), (_ptr(out), stream)))
        return out.cpu().numpy() if host else out

    def contains(self, texts):
        """bool[n]: does any entry occur in text i?  numpy for a list of texts, a device tensor for a DeviceBatch
        (enqueued on the current stream, nothing read back)."""
        import torch
        return self._per_text("mrx_kw_contains", torch.uint8, texts) != 0

    def count(self, texts):
        """int64[n]: the number of hits in text i; numpy for a list of texts, a device tensor for a DeviceBatch."""
        import torch
        return self._per_text("mrx_kw_count", torch.int64, texts)

    def _default_cap(self, nbytes: int, n: int) -> int:
        """Span capacity without a caller's cap: one hit per 8 bytes, or the density of the previous call (+1/8)."""
        return max(64, nbytes // 8 + n, int(nbytes * self._hits_per_byte * 1.125) + n + 64)

    def findall(self, texts, span_cap: Optional[int] = None):
        """Every hit of every entry, text-major (include/mrx.h, mrx_kw_findall_dev): (text_prefix int64[n+1], entries
        int32[total], spans int32[total, 2]).  Text i's hits are [text_prefix[i], text_prefix[i+1]) in ascending (end,
        start) order.  A list of bytes gives numpy arrays, a DeviceBatch device tensors.  Without span_cap the call
        retries once with the total it needs."""
        if isinstance(texts, DeviceBatch):
            import torch
            batch, dev, n = texts, texts.data.device, texts.n
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            prefix = torch.empty(n + 1, dtype=torch.int64, device=dev)
            nbytes = int(batch.data.numel())
            (ents, spans), total = _grow_call(
                int(span_cap) if span_cap is not None else self._default_cap(nbytes, n),
                lambda cap: (torch.empty(max(cap, 1), dtype=torch.int32, device=dev),
                             torch.empty((max(cap, 1), 2), dtype=torch.int32, device=dev)),
                lambda es, cap, total: batch.call(self._lib, "mrx_kw_findall", (self._h,),
                                                  (_ptr(prefix), _ptr(es[0]), _ptr(es[1]), cap, total, stream)),
                grow=span_cap is None, only_larger=True)
        else:
            data, offsets = pack_texts(texts)
            n, nbytes = len(offsets) - 1, int(offsets[-1])
            prefix = np.zeros(n + 1, np.int64)
            (ents, spans), total = _grow_call(
                int(span_cap) if span_cap is not None else self._default_cap(nbytes, n),
                lambda cap: (np.empty(max(cap, 1), np.int32), np.empty((max(cap, 1), 2), np.int32)),
                lambda es, cap, total: self._lib.mrx_kw_findall_batch(self._h, data.ctypes.data, offsets.ctypes.data, n,
                                                                      prefix.ctypes.data, es[0].ctypes.data,
                                                                      es[1].ctypes.data, cap, total),
                grow=span_cap is None, only_larger=True)
        self._hits_per_byte = total / max(1, nbytes)
        return prefix, ents[:total], spans[:total]

    def findall_lists(self, texts) -> List[List[Tuple[int, int, int]]]:
        """findall() as a list per text of (entry, start, end) tuples."""
        prefix, ents, spans = self.findall(texts)
        if not isinstance(prefix, np.ndarray):
            prefix, ents, spans = prefix.cpu().numpy(), ents.cpu().numpy(), spans.cpu().numpy()
        return [[(int(ents[q]), int(spans[q, 0]), int(spans[q, 1])) for q in range(prefix[i], prefix[i + 1])]
                for i in range(len(prefix) - 1)]

    def filter(self, texts, invert: bool = False):
        """The texts in which some entry occurs (with invert, the others) as a new packed batch, in their order: what
        CompiledRegex.filter returns (include/mrx.h, mrx_kw_filter_dev).  A list of texts gives (kept List[bytes], idx
        numpy int64[kept]), a DeviceBatch gives (DeviceBatch, idx) with device tensors."""
        if isinstance(texts, DeviceBatch):
            return _filter(self._lib, "mrx_kw_filter", self._h, _filter_flags("any", invert), texts)
        bs = [_b(t) for t in texts]
        kept, idx = self.filter(DeviceBatch.from_texts(bs), invert)
        idx = idx.cpu().numpy()
        return [bs[int(i)] for i in idx], idx

    def filter_async(self, batch: "DeviceBatch", out, invert: bool = False):
        """filter() enqueued on the current stream without a read-back, as CompiledRegex.filter_async."""
        _filter_async(self._lib, "mrx_kw_filter", self._h, _filter_flags("any", invert), batch, out)

    def leftmost(self, texts, count: int = 0, span_cap: Optional[int] = None):
        """The leftmost-longest matches of every text (include/mrx.h, mrx_kw_leftmost_dev): the non-overlapping matches
        that sub replaces, with count > 0 the first `count` of each text.  (text_prefix int64[n+1], entries
        int32[total], spans int32[total, 2]) in findall's shape, a text's matches in ascending start order; numpy arrays
        for a list of bytes, device tensors for a DeviceBatch.  Without span_cap the call retries once with the total it
        needs."""
        count = int(count)
        if isinstance(texts, DeviceBatch):
            import torch
            batch, dev, n = texts, texts.data.device, texts.n
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            prefix = torch.empty(n + 1, dtype=torch.int64, device=dev)
            nbytes = int(batch.data.numel())
            (ents, spans), total = _grow_call(
                int(span_cap) if span_cap is not None else self._default_cap(nbytes, n),
                lambda cap: (torch.empty(max(cap, 1), dtype=torch.int32, device=dev),
                             torch.empty((max(cap, 1), 2), dtype=torch.int32, device=dev)),
                lambda es, cap, total: batch.call(self._lib, "mrx_kw_leftmost", (self._h, count),
                                                  (_ptr(prefix), _ptr(es[0]), _ptr(es[1]), cap, total, stream)),
                grow=span_cap is None, only_larger=True)
        else:
            data, offsets = pack_texts(texts)
            n, nbytes = len(offsets) - 1, int(offsets[-1])
            prefix = np.zeros(n + 1, np.int64)
            (ents, spans), total = _grow_call(
                int(span_cap) if span_cap is not None else self._default_cap(nbytes, n),
                lambda cap: (np.empty(max(cap, 1), np.int32), np.empty((max(cap, 1), 2), np.int32)),
                lambda es, cap, total: self._lib.mrx_kw_leftmost_batch(self._h, count, data.ctypes.data,
                                                                       offsets.ctypes.data, n, prefix.ctypes.data,
                                                                       es[0].ctypes.data, es[1].ctypes.data, cap, total),
                grow=span_cap is None, only_larger=True)
        return prefix, ents[:total], spans[:total]

    def leftmost_lists(self, texts, count: int = 0) -> List[List[Tuple[int, int, int]]]:
        """leftmost() as a list per text of (entry, start, end) tuples."""
        prefix, ents, spans = self.leftmost(texts, count)
        if not isinstance(prefix, np.ndarray):
            prefix, ents, spans = prefix.cpu().numpy(), ents.cpu().numpy(), spans.cpu().numpy()
        return [[(int(ents[q]), int(spans[q, 0]), int(spans[q, 1])) for q in range(prefix[i], prefix[i + 1])]
                for i in range(len(prefix) - 1)]

    def _repl_batch(self, repl, device) -> "DeviceBatch":
        """The replacements as a CSR batch on the device with 1 or len(self) rows; a wrong length raises before any
        call."""
        m = len(self)
        if isinstance(repl, DeviceBatch):
            if repl.offsets is None:
                raise MrxError("the replacements must be a CSR DeviceBatch")
            rows = repl
        else:
            reps = [_b(repl)] if isinstance(repl, (bytes, bytearray, memoryview, str)) else [_b(r) for r in repl]
            rows = None
        k = rows.n if rows is not None else len(reps)
        if k != 1 and k != m:
            raise MrxError("sub needs one replacement or one per entry (%d), not %d" % (m, k))
        if rows is None:
            import torch
            data, offsets = pack_texts(reps)
            d = torch.zeros(len(data) + 16, dtype=torch.uint8, device=device)   # (a pointer even for b"")
            if len(data):
                d[:len(data)] = torch.from_numpy(data).to(device)
            rows = DeviceBatch(d, torch.from_numpy(offsets).to(device))
        return rows

    def sub(self, repl, texts, count: int = 0, out_cap: Optional[int] = None):
        """Every text with its leftmost-longest matches replaced (include/mrx.h, mrx_kw_sub_dev), with count > 0 the
        first `count` of each text; every other byte is copied unchanged.  `repl` is bytes / str (one for all), a
        sequence of len(self) of them (a match of entry j takes repl[j]) or a CSR DeviceBatch with 1 or len(self) texts;
        the bytes are taken verbatim.  A list of texts gives List[bytes]; a DeviceBatch gives a CSR DeviceBatch that
        knows its byte count and longest text, so it feeds the next call without a read-back.  Without out_cap the call
        retries once with the size it needs."""
        return self.subn(repl, texts, count, out_cap)[0]

    def subn(self, repl, texts, count: int = 0, out_cap: Optional[int] = None):
        """sub(), plus the number of replacements in every text: (List[bytes], numpy int32[n]) for a list of texts,
        (DeviceBatch, int32[n] device tensor) for a DeviceBatch."""
        import torch
        host = not isinstance(texts, DeviceBatch)
        batch = DeviceBatch.from_texts([_b(t) for t in texts]) if host else texts
        dev, n = batch.data.device, batch.n
        rows = self._repl_batch(repl, dev)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        nsub = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        totals = (C.c_int64 * 3)()
        cap = int(out_cap) if out_cap is not None else int(batch.data.numel()) + int(batch.data.numel()) // 4 + 64
        while True:
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            rc = batch.call(self._lib, "mrx_kw_sub", (self._h, _ptr(rows.data), _ptr(rows.offsets), rows.n, int(count)),
                            (_ptr(out_off), _ptr(out), cap, _ptr(nsub), None, C.cast(totals, C.c_void_p), stream))
            if rc == MRX_E_CAPACITY and out_cap is None and int(totals[0]) > cap:
                cap = int(totals[0])
                continue
            _check(rc)
            break
        nbytes = int(totals[0])
        data = out[:nbytes].clone() if 4 * nbytes < cap else out[:nbytes]
        res = DeviceBatch.csr_known(data, out_off, nbytes, int(totals[1]))
        if not host:
            return res, nsub[:n]
        raw, off = res.data.cpu().numpy().tobytes(), out_off.cpu().numpy()
        return [raw[off[i]:off[i + 1]] for i in range(n)], nsub[:n].cpu().numpy()


class CompiledRegex:
    """Compile once, match many batches (reference: matcher.mojo:929-1163)."""

    def __init__(self, pattern, lazydfa_semantics: bool = False, bitset_nfa: bool = False,
                 nfa_engine: bool = False, dfa_engine: bool = False):
        """lazydfa_semantics: MRX_COMPILE_LAZYDFA_SEMANTICS (include/mrx.h) -- NOT the
        reference's result for SIMPLE patterns; off by default.
        bitset_nfa: MRX_COMPILE_BITSET_NFA -- same results, LazyDFA walks run on the bitset NFA.
        nfa_engine: MRX_COMPILE_NFA_ENGINE -- NFAEngine itself as the Engine (regex.nfa, nfa.mojo:66-143,
        1733-1769), no hybrid router in front.
        dfa_engine: MRX_COMPILE_DFA_ENGINE -- compile_dfa_pattern's DFAEngine as the Engine (comptime API)."""
        self._lib = load_library()
        self.pattern = _b(pattern)
        self.lazydfa_semantics = bool(lazydfa_semantics)
        h = C.c_void_p()
        _check(self._lib.mrx_compile_ex(self.pattern, len(self.pattern),
                                        (1 if lazydfa_semantics else 0) | (2 if bitset_nfa else 0)
                                        | (4 if nfa_engine else 0) | (8 if dfa_engine else 0),
                                        C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.mrx_free(self._h)
                self._h = None
        except Exception:
            pass

    # -- introspection (get_engine_type :900-918, get_stats :1139-1163) ------------
    def get_engine_type(self) -> str:
        return self._lib.mrx_engine_type(self._h).decode()

    def get_stats(self) -> str:
        return self._lib.mrx_stats(self._h).decode("utf-8", "replace")

    def describe(self) -> str:
        need = self._lib.mrx_describe(self._h, None, 0)
        buf = C.create_string_buffer(need + 1)
        self._lib.mrx_describe(self._h, buf, need + 1)
        return buf.value.decode("utf-8", "replace")

    @property
    def num_groups(self) -> int:
        return self._lib.mrx_num_groups(self._h)

    # -- host-buffer batches --------------------------------------------------------
    def _spans_call(self, fn, texts):
        data, offsets = pack_texts(texts)
        n = len(offsets) - 1
        s = np.empty(n, np.int32)
        e = np.empty(n, np.int32)
        _check(fn(self._h, data.ctypes.data, offsets.ctypes.data, n, s.ctypes.data, e.ctypes.data))
        return s, e

    def match_first(self, texts) -> Tuple[np.ndarray, np.ndarray]:
        """regex.match_first per text: (start[n], end[n]), -1/-1 where none."""
        if isinstance(texts, DeviceBatch):
            return self._dev_spans(self._lib.mrx_match_first_dev, self._lib.mrx_match_first_strided_dev,
                                   texts)
        return self._spans_call(self._lib.mrx_match_first_batch, texts)

    def match_next(self, texts) -> Tuple[np.ndarray, np.ndarray]:
        """regex.search per text."""
        if isinstance(texts, DeviceBatch):
            return self._dev_spans(self._lib.mrx_search_dev, self._lib.mrx_search_strided_dev, texts)
        return self._spans_call(self._lib.mrx_search_batch, texts)

    search = match_next

    def is_match(self, texts):
        """CompiledRegex.is_match(text, 0): uint8[n] -- numpy for host texts, a device tensor for a
        DeviceBatch."""
        if isinstance(texts, DeviceBatch):   # device tensor uint8[n]
            import torch
            f = torch.empty(texts.n, dtype=torch.uint8, device=texts.data.device)
            _check(texts.call(self._lib, "mrx_is_match", (self._h,), (_ptr(f), self._stream_ptr())))
            return f
        data, offsets = pack_texts(texts)
        n = len(offsets) - 1
        f = np.empty(n, np.uint8)
        _check(self._lib.mrx_is_match_batch(self._h, data.ctypes.data, offsets.ctypes.data, n,
                                            f.ctypes.data))
        return f

    # -- the Engine / RegexMatcher seam with its `start` argument (engine.mojo:4-37) ------------------
    def _at(self, op: str, texts, start):
        """op in {"match_first", "search", "is_match"}; start: one int for all texts, or int32[n]
        (numpy / device tensor).  Host texts are uploaded; a DeviceBatch is used in place."""
        import torch
        batch = texts if isinstance(texts, DeviceBatch) else DeviceBatch.from_texts(texts)
        dev = batch.data.device
        d_starts = None
        s0 = 0
        if isinstance(start, (int, np.integer)):
            s0 = int(start)
        else:
            d_starts = start if isinstance(start, torch.Tensor) else torch.from_numpy(np.asarray(start, dtype=np.int32))
            d_starts = d_starts.to(device=dev, dtype=torch.int32).contiguous()
            if d_starts.numel() != batch.n:
                raise MrxError("starts needs one entry per text")
        if op == "is_match":
            f = torch.empty(batch.n, dtype=torch.uint8, device=dev)
            _check(batch.call(self._lib, "mrx_is_match_at", (self._h,), (s0, _ptr(d_starts), _ptr(f), self._stream_ptr())))
            return f if isinstance(texts, DeviceBatch) else f.cpu().numpy()
        s = torch.empty(batch.n, dtype=torch.int32, device=dev)
        e = torch.empty(batch.n, dtype=torch.int32, device=dev)
        _check(batch.call(self._lib, "mrx_match_first_at" if op == "match_first" else "mrx_search_at", (self._h,),
                          (s0, _ptr(d_starts), _ptr(s), _ptr(e), self._stream_ptr())))
        return (s, e) if isinstance(texts, DeviceBatch) else (s.cpu().numpy(), e.cpu().numpy())

    def match_first_at(self, texts, start):
        """CompiledRegex.match_first(text, start) (matcher.mojo:1049-1062): a match beginning at start."""
        return self._at("match_first", texts, start)

    def match_next_at(self, texts, start):
        """CompiledRegex.match_next(text, start) (matcher.mojo:1064-1077): leftmost match from start on."""
        return self._at("search", texts, start)

    def is_match_at(self, texts, start):
        """CompiledRegex.is_match(text, start) (matcher.mojo:1103-1115)."""
        return self._at("is_match", texts, start)

    def test(self, texts):
        """CompiledRegex.test (matcher.mojo:1091-1101): does search() match.  bool[n]: numpy for host
        texts, a device tensor for a DeviceBatch."""
        s, _ = self.match_next(texts)
        if isinstance(texts, DeviceBatch):
            return s >= 0
        return (np.asarray(s) >= 0)

    def filter(self, texts, invert: bool = False):
        """The texts in which search() matches (test(); with invert, the others) as a new packed batch, in their order
        (include/mrx.h, mrx_filter_dev).  A list of texts gives (kept List[bytes], idx numpy int64[kept]); a
        DeviceBatch gives (DeviceBatch, idx) with device tensors: a CSR batch trimmed to the kept texts and their bytes.
        It carries known bounds (its byte count, and the input's longest text as its own) when the input knows its
        longest text -- a fixed pitch, from_texts / from_arrow / csr_known -- so that a following findall, sub or filter
        needs no read-back for them; the result of a plain DeviceBatch(data, offsets) has none, as its input.  The
        tensors are views of buffers sized for the whole input unless the result uses less than a quarter of them (then
        they are copies of their own size).  idx holds the original indices."""
        return _filter(self._lib, "mrx_filter", self._h, _filter_flags("any", invert), texts)

    def filter_async(self, batch: "DeviceBatch", out, invert: bool = False):
        """Enqueue filter on the current stream without reading anything back.  out = (kept_idx int64[n], out_offsets
        int64[n + 1], out_data uint8[cap], totals int64[2]) device tensors of the caller; totals = {kept, bytes} once the
        stream has drained.  No byte is written when bytes > cap (check totals[1]); cap = the input's bytes always fits."""
        _filter_async(self._lib, "mrx_filter", self._h, _filter_flags("any", invert), batch, out)

    def extract(self, texts, group: Optional[int] = None, count: int = 0):
        """The matched bytes themselves (re.findall's strings; include/mrx.h, mrx_extract_dev).  group=None: findall's
        matches, in its order -- empty matches and the overlapping occurrences of an exact literal included; count must
        be 0.  group=j, 0 <= j <= num_groups: that group of every captures_all match (at most `count` per text, 0 =
        all), an unset group as an empty piece; j = 0 is the whole match of that loop, which is not always findall's
        list: captures_all's matches "are NOT findall's spans where the groups run on the backtracker: it is greedy and
        the first alternative wins, while findall takes the hybrid engines' leftmost-longest walk ... Exact literals
        differ too: findall returns overlapping occurrences, this loop does not" (include/mrx.h, mrx_captures_all_dev).
        A list of texts gives List[List[bytes]]; a DeviceBatch gives (pieces DeviceBatch, prefix int64[n + 1], owner
        int64[pieces]) on the device: text i's pieces are the texts [prefix[i], prefix[i + 1]) of `pieces`, and owner[r]
        = i for each of them.  `pieces` carries known bounds as filter's result does.
        Cost: the piece capacity is findall's default, a match per 8 bytes, and the sizes kernel and the scan run over
        the capacity, not over the pieces (profiles/extract.md); DeviceBatch.gather_spans on findall's own spans takes
        an exact capacity."""
        if not isinstance(texts, DeviceBatch):
            pieces, prefix, _ = self.extract(DeviceBatch.from_texts([_b(t) for t in texts]), group, count)
            return _piece_lists(pieces, prefix)
        if group is None:
            if count != 0:
                raise MrxError("count needs a group: findall has no limit")
            import torch
            prefix = torch.empty(texts.n + 1, dtype=torch.int64, device=texts.data.device)
            nbytes = int(texts.data.numel())
            res = _extract_result(texts, _grow_call2(
                max(64, nbytes // 8 + texts.n), nbytes, texts.data.device,
                lambda pb, pcap, out, ocap, d_totals, totals: texts.call(
                    self._lib, "mrx_extract", (self._h,),
                    (_ptr(prefix), _ptr(pb[0]), _ptr(pb[1]), pcap, _ptr(out), ocap, _ptr(d_totals), totals,
                     self._stream_ptr()))))
            return res[0], prefix, res[1]
        g = self.num_groups
        if not 0 <= int(group) <= g:
            raise MrxError("group must be in [0, %d]" % g)
        prefix, rows = self._captures_all_dev(texts, count)
        # rows hold groups 1..g, then group 0
        pieces, owner = texts.gather_spans(prefix, rows, pair=(int(group) - 1) % (g + 1))
        return pieces, prefix, owner

    def numbers(self, texts, kind: str = "int", group: Optional[int] = None, count: int = 0, fill=0):
        """The matches of this pattern as numbers, without gathering their bytes (include/mrx.h, "numbers"): extract
        followed by int() or float() on every piece.  group, count and the matches are extract's: group=None parses
        findall's matches (count must be 0), group=j that group of every captures_all match, an unset group as an empty
        piece.  kind and fill are DeviceBatch.parse's.  A DeviceBatch gives (values, status, prefix, owner) on the
        device: text i's rows are [prefix[i], prefix[i + 1]), owner[r] = i for each of them, values int64 (float64 for
        "float") and status uint8, 0 where the row is a number.  A list of texts gives List[List[Optional[int | float]]],
        None where the status is not 0."""
        if not isinstance(texts, DeviceBatch):
            values, status, prefix, _ = self.numbers(DeviceBatch.from_texts([_b(t) for t in texts]), kind, group, count, fill)
            return _num_lists(kind, values, status, prefix)
        _num_kind(kind)
        if group is None:
            if count != 0:
                raise MrxError("count needs a group: findall has no limit")
            prefix, spans, total = self._dev_findall(texts)
            rows, pair = spans[:total], 0
        else:
            g = self.num_groups
            if not 0 <= int(group) <= g:
                raise MrxError("group must be in [0, %d]" % g)
            prefix, rows = self._captures_all_dev(texts, count)
            pair = (int(group) - 1) % (g + 1)   # rows hold groups 1..g, then group 0
        values, status, owner = texts.parse_spans(prefix, rows, pair, kind, fill)
        return values, status, prefix, owner

    def expand(self, template, texts, count: int = 0):
        """One record per match, built from the match's groups and literal bytes: Python's [m.expand(t) for m in
        re.finditer(p, s)] (include/mrx.h, mrx_expand_dev).  `template` is sub's template: only \\1..\\9 are references,
        every other byte is literal; the record of a match is what sub(template, ...) puts in its place -- an unset
        group and a group the pattern lacks contribute nothing.  The matches are captures_all's (at most `count` per
        text, 0 = all), which is not always findall's list: captures_all's matches "are NOT findall's spans where the
        groups run on the backtracker: it is greedy and the first alternative wins, while findall takes the hybrid
        engines' leftmost-longest walk ... Exact literals differ too: findall returns overlapping occurrences, this loop
        does not" (include/mrx.h, mrx_captures_all_dev).
        A list of texts gives List[List[bytes]]; a DeviceBatch gives (records DeviceBatch, prefix int64[n + 1], owner
        int64[records]) on the device, shaped as extract's result; `records` carries known bounds where the input does,
        its longest record bounded by len(template) + references x the input's longest text."""
        template = _b(template)
        if not isinstance(texts, DeviceBatch):
            records, prefix, _ = self.expand(template, DeviceBatch.from_texts([_b(t) for t in texts]), count)
            return _piece_lists(records, prefix)
        import torch
        prefix = torch.empty(texts.n + 1, dtype=torch.int64, device=texts.data.device)
        nbytes = int(texts.data.numel())
        res = _expand_result(texts, template, _grow_call2(
            max(64, nbytes // 8 + texts.n), max(64, nbytes), texts.data.device,
            lambda pb, pcap, out, ocap, d_totals, totals: texts.call(
                self._lib, "mrx_expand", (self._h, template, len(template), int(count)),
                (_ptr(prefix), _ptr(pb[0]), _ptr(pb[1]), pcap, _ptr(out), ocap, _ptr(d_totals), totals,
                 self._stream_ptr()))))
        return res[0], prefix, res[1]

    def value_counts(self, texts, group: Optional[int] = None, count: int = 0, sort: Optional[str] = None,
                     top: Optional[int] = None):
        """Which strings this pattern matched in the batch, and how often each: extract(texts, group, count) followed by
        distinct over all its pieces (grep -o | sort | uniq -c without the sort).  A DeviceBatch gives (values
        DeviceBatch, counts int64[u]) on the device, in the order in which the values first occur in extract's pieces;
        a list of texts gives List[Tuple[bytes, int]] in that order, which equals
        list(collections.Counter(p for t in texts for p in rx.extract([t], group, count)[0]).items()).
        sort="value" orders the rows ascending by value (the sort of sort | uniq -c), sort="count" by descending count
        with ties in first-occurrence order (Counter.most_common(), sort | uniq -c | sort -rn); top=k keeps the first k
        rows of the chosen order (most_common(k), head -k).  The rows are reordered on the device: DeviceBatch.argsort
        or a stable torch.sort of the counts, then DeviceBatch.take."""
        if not isinstance(texts, DeviceBatch):
            values, counts = self.value_counts(DeviceBatch.from_texts([_b(t) for t in texts]), group, count, sort, top)
            raw = values.data.cpu().numpy().tobytes()
            off = values.offsets.cpu().numpy()
            return [(raw[off[g]:off[g + 1]], int(c)) for g, c in enumerate(counts.cpu().numpy())]
        pieces = self.extract(texts, group, count)[0]
        values, counts, _, _ = pieces.distinct()
        return _sort_counts(values, counts, sort, top)

    def extract_async(self, batch: "DeviceBatch", out):
        """Enqueue extract (findall's matches) on the current stream without reading anything back.  out =
        (piece_prefix int64[n + 1], owner int64[piece_cap], out_offsets int64[piece_cap + 1], out_data uint8[out_cap],
        totals int64[2]) device tensors of the caller; totals = {pieces, bytes} once the stream has drained.  No byte is
        written when pieces > piece_cap or bytes > out_cap (check totals against both).  A CSR batch without known bounds
        still pays findall's one read-back of them."""
        import torch
        prefix, owner, out_offsets, out_data, totals = out
        if prefix.numel() < batch.n + 1 or out_offsets.numel() < owner.numel() + 1 or totals.numel() < 2:
            raise MrxError("out needs piece_prefix int64[n + 1], owner int64[cap], out_offsets int64[cap + 1], "
                           "out_data uint8[out_cap], totals int64[2]")
        for t in (prefix, owner, out_offsets, totals):
            if t.dtype != torch.int64 or not t.is_contiguous():
                raise MrxError("piece_prefix, owner, out_offsets and totals must be contiguous int64 tensors")
        if out_data.dtype != torch.uint8 or not out_data.is_contiguous():
            raise MrxError("out_data must be a contiguous uint8 tensor")
        _check(batch.call(self._lib, "mrx_extract", (self._h,),
                          (_ptr(prefix), _ptr(owner), _ptr(out_offsets), int(owner.numel()), _ptr(out_data),
                           int(out_data.numel()), _ptr(totals), None, self._stream_ptr())))

    def split_batch(self, batch: "DeviceBatch", maxsplit: int = 0):
        """regex.split of a device-resident batch as bytes: split_dev's ranges gathered into a new packed batch,
        (pieces DeviceBatch, piece_prefix int64[n + 1], owner int64[pieces]), shaped as extract's result."""
        prefix, ranges, total = self.split_dev(batch, maxsplit)
        pieces, owner = batch.gather_spans(prefix, ranges[:total])
        return pieces, prefix, owner

    def match_all(self, texts):
        """regex.findall per text: (counts_prefix int64[n+1], spans int32[total, 2])."""
        if isinstance(texts, DeviceBatch):
            return self._dev_findall(texts)
        data, offsets = pack_texts(texts)
        n = len(offsets) - 1
        prefix = np.zeros(n + 1, np.int64)
        spans, total = _grow_call(
            max(64, int(offsets[-1]) // 4 + n), lambda cap: np.empty((cap, 2), np.int32),
            lambda spans, cap, total: self._lib.mrx_findall_batch(self._h, data.ctypes.data, offsets.ctypes.data, n,
                                                                  prefix.ctypes.data, spans.ctypes.data, cap, total))
        return prefix, spans[:total]

    findall = match_all

    def findall_lists(self, texts) -> List[List[Tuple[int, int]]]:
        prefix, spans = self.match_all(texts)
        out = []
        for i in range(len(prefix) - 1):
            out.append([(int(a), int(b)) for a, b in spans[prefix[i]:prefix[i + 1]]])
        return out

    def split(self, texts, maxsplit: int = 0) -> List[List[bytes]]:
        """regex.split per text: the pieces between successive matches (mrx_split_batch)."""
        bs = [_b(t) for t in texts]
        data, offsets = pack_texts(bs)
        n = len(bs)
        prefix = np.zeros(n + 1, dtype=np.int64)
        pieces, _ = _grow_call(
            max(16, 2 * n + len(data) // 8), lambda cap: np.empty((cap, 2), dtype=np.int32),
            lambda pieces, cap, total: self._lib.mrx_split_batch(self._h, data.ctypes.data, offsets.ctypes.data, n,
                                                                 int(maxsplit), prefix.ctypes.data, pieces.ctypes.data,
                                                                 cap, total), only_larger=True)
        out = []
        for i, t in enumerate(bs):
            out.append([t[int(a):int(b)] for a, b in pieces[prefix[i]:prefix[i + 1]]])
        return out

    def split_dev(self, batch: "DeviceBatch", maxsplit: int = 0, piece_cap: Optional[int] = None):
        """regex.split of a device-resident batch: (piece_prefix int64[n + 1], pieces int32[total, 2], total)."""
        import torch
        dev = batch.data.device
        n = batch.n
        prefix = torch.empty(n + 1, dtype=torch.int64, device=dev)
        pieces, total = _grow_call(
            piece_cap if piece_cap is not None else max(16, 2 * n + batch.data.numel() // 8),
            lambda cap: torch.empty((cap, 2), dtype=torch.int32, device=dev),
            lambda pieces, cap, total: batch.call(self._lib, "mrx_split", (self._h,),
                                                  (int(maxsplit), _ptr(prefix), _ptr(pieces), cap, total,
                                                   self._stream_ptr())),
            grow=piece_cap is None, only_larger=True)
        return prefix, pieces, total

    def captures(self, texts) -> np.ndarray:
        """search + capture groups, int32[n, g+1, 2] in the order the reference's
        NFAEngine._match_group appends them: groups 1..g, then group 0."""
        data, offsets = pack_texts(texts)
        n = len(offsets) - 1
        g = self.num_groups
        out = np.empty((n, g + 1, 2), np.int32)
        _check(self._lib.mrx_captures_batch(self._h, data.ctypes.data, offsets.ctypes.data, n,
                                            out.ctypes.data))
        return out

    def captures_all(self, texts, count: int = 0):
        """Capture groups of every match: the matches of sub()'s loop with a group template, at most `count` per text
        (0 = all; include/mrx.h, mrx_captures_all_dev).  (match_prefix int64[n+1], groups int32[total, g+1, 2]), rows in
        the order of captures(): groups 1..g, then group 0.  Host texts give numpy arrays, a DeviceBatch device tensors."""
        g = self.num_groups
        if isinstance(texts, DeviceBatch):
            return self._captures_all_dev(texts, count)
        data, offsets = pack_texts(texts)
        n = len(offsets) - 1
        prefix = np.zeros(n + 1, np.int64)
        groups, total = _grow_call(
            max(64, int(offsets[-1]) // 8 + n), lambda cap: np.empty((cap, g + 1, 2), np.int32),
            lambda groups, cap, total: self._lib.mrx_captures_all_batch(self._h, data.ctypes.data, offsets.ctypes.data, n,
                                                                        int(count), prefix.ctypes.data,
                                                                        groups.ctypes.data, cap, total),
            only_larger=True)
        return prefix, groups[:total]

    def _captures_all_dev(self, batch: "DeviceBatch", count: int = 0, match_cap: Optional[int] = None):
        import torch
        dev = batch.data.device
        g = self.num_groups
        prefix = torch.empty(batch.n + 1, dtype=torch.int64, device=dev)
        groups, total = _grow_call(
            int(match_cap) if match_cap is not None else max(64, batch.data.numel() // 8 + batch.n),
            lambda cap: torch.empty((cap, g + 1, 2), dtype=torch.int32, device=dev),
            lambda groups, cap, total: batch.call(self._lib, "mrx_captures_all", (self._h,),
                                                  (int(count), _ptr(prefix), _ptr(groups), cap, total,
                                                   self._stream_ptr())),
            grow=match_cap is None, only_larger=True)
        return prefix, groups[:total]

    def sub(self, repl, texts, count: int = 0) -> List[bytes]:
        repl = _b(repl)
        data, offsets = pack_texts(texts)
        n = len(offsets) - 1
        out_off = np.zeros(n + 1, np.int64)
        out, total = _grow_call(
            max(64, int(offsets[-1]) * 2 + 16 * n), lambda cap: np.empty(cap, np.uint8),
            lambda out, cap, total: self._lib.mrx_sub_batch(self._h, repl, len(repl), count, data.ctypes.data,
                                                            offsets.ctypes.data, n, out_off.ctypes.data, out.ctypes.data,
                                                            cap, total))
        raw = out[:total].tobytes()
        return [raw[out_off[i]:out_off[i + 1]] for i in range(n)]

    def captures_dev(self, batch: "DeviceBatch"):
        """search + capture groups on a device-resident batch: int32[n, g+1, 2] (device tensor)."""
        import torch
        g = self.num_groups
        out = torch.empty((batch.n, g + 1, 2), dtype=torch.int32, device=batch.data.device)
        _check(batch.call(self._lib, "mrx_captures", (self._h,), (_ptr(out), self._stream_ptr())))
        return out

    def sub_dev(self, repl, batch: "DeviceBatch", count: int = 0, out_cap: Optional[int] = None):
        """regex.sub on a device-resident batch (CSR, or fixed pitch, padded or not):
        (out_offsets int64[n+1], out_data uint8[total])."""
        import torch
        repl = _b(repl)
        dev = batch.data.device
        out_off = torch.empty(batch.n + 1, dtype=torch.int64, device=dev)
        out, total = _grow_call(
            int(out_cap) if out_cap else int(batch.data.numel()) * 2 + 16 * batch.n + 64,
            lambda cap: torch.empty(cap, dtype=torch.uint8, device=dev),
            lambda out, cap, total: batch.call(self._lib, "mrx_sub", (self._h, repl, len(repl), count),
                                               (_ptr(out_off), _ptr(out), cap, total, self._stream_ptr())))
        return out_off, out[:total]

    # -- device-resident batches (torch tensors) ------------------------------------
    def _stream_ptr(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _dev_spans(self, fn_csr, fn_strided, batch: DeviceBatch):
        import torch
        s = torch.empty(batch.n, dtype=torch.int32, device=batch.data.device)
        e = torch.empty(batch.n, dtype=torch.int32, device=batch.data.device)
        _check(batch.call(self._lib, (fn_csr, fn_strided), (self._h,), (_ptr(s), _ptr(e), self._stream_ptr())))
        return s, e

    def findall_async(self, batch: DeviceBatch, out):
        """Enqueue findall on the current stream without reading anything back.
        out = (counts_prefix int64[n+1], spans int32[cap, 2]) device tensors; the total
        is counts_prefix[n] once the stream has drained (check it against cap)."""
        prefix, spans = out
        _check(batch.call(self._lib, "mrx_findall", (self._h,),
                          (_ptr(prefix), _ptr(spans), spans.shape[0], None, self._stream_ptr())))

    def _dev_findall(self, batch: DeviceBatch, span_cap: Optional[int] = None, out=None):
        """Returns (counts_prefix int64[n+1], spans int32[cap, 2], total) on device."""
        import torch
        dev = batch.data.device
        if out is None:
            if span_cap is None:
                span_cap = max(64, batch.data.numel() // 8 + batch.n)
            prefix = torch.empty(batch.n + 1, dtype=torch.int64, device=dev)
            spans = torch.empty((span_cap, 2), dtype=torch.int32, device=dev)
        else:
            prefix, spans = out
            span_cap = spans.shape[0]
        ready = [spans]   # (the first call's buffer is there already)
        spans, total = _grow_call(
            span_cap, lambda cap: ready.pop() if ready else torch.empty((cap, 2), dtype=torch.int32, device=dev),
            lambda spans, cap, total: batch.call(self._lib, "mrx_findall", (self._h,),
                                                 (_ptr(prefix), _ptr(spans), cap, total, self._stream_ptr())),
            grow=out is None)
        return prefix, spans, total

    def count(self, batch: DeviceBatch):
        import torch
        counts = torch.empty(batch.n, dtype=torch.int32, device=batch.data.device)
        _check(batch.call(self._lib, "mrx_count", (self._h,), (_ptr(counts), self._stream_ptr())))
        return counts


class PatternSet:
    """k patterns answered together over one batch (include/mrx.h, "pattern sets"; Rust's RegexSet idea).

    Member j's answer for text i is exactly CompiledRegex(patterns[j]).match_next / count for that text.  `texts` is a
    DeviceBatch (results: device tensors [n, k]) or a list of bytes (copied in; results: numpy arrays [n, k])."""

    def __init__(self, patterns, *, lazydfa_semantics: bool = False, bitset_nfa: bool = False):
        self._lib = load_library()
        self._h = None
        self._hits_per_byte = 0.0   # findall: hits per input byte of the last call (sizes the next call's capacity)
        self.patterns = [_b(p) for p in patterns]
        k = len(self.patterns)
        arr = (C.c_char_p * max(k, 1))(*self.patterns)
        lens = (C.c_size_t * max(k, 1))(*[len(p) for p in self.patterns])
        h = C.c_void_p()
        _check(self._lib.mrx_set_compile(arr, lens, k, (1 if lazydfa_semantics else 0) | (2 if bitset_nfa else 0),
                                         C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h is not None:
                self._lib.mrx_set_free(self._h)
                self._h = None
        except Exception:
            pass

    def __len__(self) -> int:
        return int(self._lib.mrx_set_size(self._h))

    def describe(self) -> str:
        need = self._lib.mrx_set_describe(self._h, None, 0)
        buf = C.create_string_buffer(need + 1)
        self._lib.mrx_set_describe(self._h, buf, need + 1)
        return buf.value.decode("utf-8", "replace")

    def _run(self, op: str, texts):
        import torch
        host = not isinstance(texts, DeviceBatch)
        batch = DeviceBatch.from_texts(list(texts)) if host else texts
        k, n, dev = len(self), batch.n, batch.data.device
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if op == "search":
            s = torch.empty((n, k), dtype=torch.int32, device=dev)
            e = torch.empty((n, k), dtype=torch.int32, device=dev)
            _check(batch.call(self._lib, "mrx_set_search", (self._h,), (_ptr(s), _ptr(e), stream)))
            return (s.cpu().numpy(), e.cpu().numpy()) if host else (s, e)
        if op == "count":
            c = torch.empty((n, k), dtype=torch.int32, device=dev)
            _check(batch.call(self._lib, "mrx_set_count", (self._h,), (_ptr(c), stream)))
            return c.cpu().numpy() if host else c
        words = (k + 63) // 64
        w = torch.empty((n, words), dtype=torch.int64, device=dev)
        _check(batch.call(self._lib, "mrx_set_matches", (self._h,), (_ptr(w), stream)))
        if host:
            u = w.cpu().numpy().view(np.uint64)
            bits = (u[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
            return bits.reshape(n, words * 64)[:, :k].astype(bool)
        shifts = torch.arange(64, dtype=torch.int64, device=dev)
        bits = (w.unsqueeze(-1) >> shifts) & 1
        return bits.reshape(n, words * 64)[:, :k].bool()

    def search(self, texts):
        """(start, end) int32 [n, k] per member: regex.search, -1/-1 when member j finds nothing in text i."""
        return self._run("search", texts)

    def count(self, texts):
        """int32 [n, k]: len(findall(member j, text i))."""
        return self._run("count", texts)

    def matches(self, texts):
        """bool [n, k]: member j's search finds a match in text i (a search hit, not is_match)."""
        return self._run("matches", texts)

    def filter(self, texts, mode: str = "any", invert: bool = False):
        """The texts in which some member's search matches (mode="any") or every member's does (mode="all") -- with
        invert, the others, so any + invert is "none" -- as a new packed batch in their order (include/mrx.h,
        mrx_set_filter_dev).  Shapes as CompiledRegex.filter: (List[bytes], numpy idx) for a list of texts, (DeviceBatch,
        idx) device tensors for a DeviceBatch."""
        return _filter(self._lib, "mrx_set_filter", self._h, _filter_flags(mode, invert), texts)

    def filter_async(self, batch: "DeviceBatch", out, mode: str = "any", invert: bool = False):
        """filter() enqueued on the current stream without a read-back, as CompiledRegex.filter_async."""
        _filter_async(self._lib, "mrx_set_filter", self._h, _filter_flags(mode, invert), batch, out)

    def findall(self, texts, span_cap: Optional[int] = None):
        """Every member's findall, text-major (include/mrx.h, mrx_set_findall_dev): (text_prefix int64[n+1],
        members int32[total], spans int32[total, 2]).  Text i's hits are [text_prefix[i], text_prefix[i+1]): member
        0's findall spans of text i in match order, then member 1's, and so on.  A list of bytes gives numpy arrays, a
        DeviceBatch device tensors.  Without span_cap the call retries once with the total it needs."""
        if isinstance(texts, DeviceBatch):
            return self._findall_dev(texts, span_cap)
        data, offsets = pack_texts(texts)
        n = len(offsets) - 1
        prefix = np.zeros(n + 1, np.int64)
        (members, spans), total = _grow_call(
            int(span_cap) if span_cap is not None else self._default_cap(int(offsets[-1]), n),
            lambda cap: (np.empty(max(cap, 1), np.int32), np.empty((max(cap, 1), 2), np.int32)),
            lambda ms, cap, total: self._lib.mrx_set_findall_batch(self._h, data.ctypes.data, offsets.ctypes.data, n,
                                                                   prefix.ctypes.data, ms[0].ctypes.data,
                                                                   ms[1].ctypes.data, cap, total),
            grow=span_cap is None, only_larger=True)
        self._hits_per_byte = total / max(1, int(offsets[-1]))
        return prefix, members[:total], spans[:total]

    def extract(self, texts):
        """Every member's findall hits as bytes: findall()'s hits, text-major, gathered into a new packed batch
        (include/mrx.h, mrx_gather_spans_dev).  A DeviceBatch gives (pieces DeviceBatch, text_prefix int64[n + 1],
        members int32[pieces], owner int64[pieces]) on the device; a list of texts gives a list per text of (member,
        bytes) tuples."""
        host = not isinstance(texts, DeviceBatch)
        batch = DeviceBatch.from_texts([_b(t) for t in texts]) if host else texts
        prefix, members, spans = self._findall_dev(batch)
        pieces, owner = batch.gather_spans(prefix, spans)
        if not host:
            return pieces, prefix, members, owner
        members = members.cpu().numpy()
        prefix = prefix.cpu().numpy()
        return [[(int(members[prefix[i] + q]), p) for q, p in enumerate(row)]
                for i, row in enumerate(_piece_lists(pieces, prefix))]

    def _default_cap(self, nbytes: int, n: int) -> int:
        """Span capacity without a caller's cap: one hit per 8 bytes, or the density of this set's previous call (+1/8)
        where that was higher, so that a dense rule set does not pay the retry on every call."""
        by_last = int(nbytes * self._hits_per_byte * 1.125)
        return max(64, nbytes // 8 + n, by_last + n + 64)

    def _findall_dev(self, batch: "DeviceBatch", span_cap: Optional[int] = None):
        import torch
        dev = batch.data.device
        n = batch.n
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        prefix = torch.empty(n + 1, dtype=torch.int64, device=dev)
        (members, spans), total = _grow_call(
            int(span_cap) if span_cap is not None else self._default_cap(batch.data.numel(), n),
            lambda cap: (torch.empty(max(cap, 1), dtype=torch.int32, device=dev),
                         torch.empty((max(cap, 1), 2), dtype=torch.int32, device=dev)),
            lambda ms, cap, total: batch.call(self._lib, "mrx_set_findall", (self._h,),
                                              (_ptr(prefix), _ptr(ms[0]), _ptr(ms[1]), cap, total, stream)),
            grow=span_cap is None, only_larger=True)
        self._hits_per_byte = total / max(1, batch.data.numel())
        return prefix, members[:total], spans[:total]

    def findall_lists(self, texts) -> List[List[Tuple[int, int, int]]]:
        """findall() as a list per text of (member, start, end) tuples."""
        prefix, members, spans = self.findall(texts)
        if not isinstance(prefix, np.ndarray):
            prefix, members, spans = prefix.cpu().numpy(), members.cpu().numpy(), spans.cpu().numpy()
        return [[(int(members[q]), int(spans[q, 0]), int(spans[q, 1])) for q in range(prefix[i], prefix[i + 1])]
                for i in range(len(prefix) - 1)]

    def _repl_table(self, repl):
        """(repls, repl_lens, keep-alive) for the C call: one replacement for every member, or a sequence of k."""
        k = len(self)
        if isinstance(repl, (bytes, bytearray, memoryview, str)):
            reps = [_b(repl)] * k
        else:
            reps = [_b(r) for r in repl]
            if len(reps) != k:
                raise MrxError("repl: %d replacements for a set of %d members" % (len(reps), k))
        arr = (C.c_char_p * max(k, 1))(*reps)
        lens = (C.c_size_t * max(k, 1))(*[len(r) for r in reps])
        return C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p), (arr, lens, reps)

    def sub(self, repl, texts, count: int = 0, out_cap: Optional[int] = None):
        """Replace the hits of every member in one call (include/mrx.h, mrx_set_sub_dev): the candidates are the
        members' findall hits; in ascending (start, member) order a hit is selected when it starts at or after the end
        of the last selected one (an empty hit: one past it), and replaced by its member's replacement.  `repl` is
        bytes / str for every member or a sequence of k.  A list of texts gives List[bytes], a DeviceBatch
        (out_offsets int64[n+1], out_data uint8[total]) device tensors.  Without out_cap the call retries once with the
        size it needs."""
        return self._sub(repl, texts, count, out_cap)[:2] if isinstance(texts, DeviceBatch) else \
            self._sub(repl, texts, count, out_cap)[0]

    def subn(self, repl, texts, count: int = 0, out_cap: Optional[int] = None):
        """sub(), plus the number of replacements in each text, int32[n]: (List[bytes], numpy) for a list of texts,
        (out_offsets, out_data, nsub) device tensors for a DeviceBatch."""
        return self._sub(repl, texts, count, out_cap)

    def _sub(self, repl, texts, count: int, out_cap: Optional[int]):
        repls, lens, keep = self._repl_table(repl)   # (keep: the ctypes tables live until the call returns)
        longest = max((len(r) for r in keep[2]), default=0)
        if isinstance(texts, DeviceBatch):
            return self._sub_dev(repls, lens, longest, texts, count, out_cap)
        data, offsets = pack_texts(texts)
        n = len(offsets) - 1
        out_off = np.zeros(n + 1, np.int64)
        nsub = np.zeros(max(n, 1), np.int32)
        out, total = _grow_call(
            int(out_cap) if out_cap is not None else int(offsets[-1]) * 2 + (16 + longest) * n + 64,
            lambda cap: np.empty(max(cap, 1), np.uint8),
            lambda out, cap, total: self._lib.mrx_set_sub_batch(self._h, repls, lens, count, data.ctypes.data,
                                                                offsets.ctypes.data, n, out_off.ctypes.data,
                                                                out.ctypes.data, cap, nsub.ctypes.data, total),
            grow=out_cap is None, only_larger=True)
        raw = out[:total].tobytes()
        return [raw[out_off[i]:out_off[i + 1]] for i in range(n)], nsub[:n]

    def _sub_dev(self, repls, lens, longest: int, batch: "DeviceBatch", count: int, out_cap: Optional[int]):
        import torch
        dev = batch.data.device
        n = batch.n
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        nsub = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        out, total = _grow_call(
            int(out_cap) if out_cap is not None else int(batch.data.numel()) * 2 + (16 + longest) * n + 64,
            lambda cap: torch.empty(max(cap, 1), dtype=torch.uint8, device=dev),
            lambda out, cap, total: batch.call(self._lib, "mrx_set_sub", (self._h, repls, lens, count),
                                               (_ptr(out_off), _ptr(out), cap, _ptr(nsub), total, stream)),
            grow=out_cap is None, only_larger=True)
        return out_off, out[:total], nsub[:n]

    def _host_run(self, op: int, text: bytes):
        """Testing: the packed set tables walked on the CPU for one text (mrx_testing_set_run); -2 = not in a shared
        pass for that operation."""
        k = len(self)
        out = (C.c_int32 * (2 * k))()
        _check(self._lib.mrx_testing_set_run(self._h, op, bytes(text), len(text), out))
        return list(out)[: (2 * k if op == 1 else k)]


def compile_set(patterns, *, lazydfa_semantics: bool = False, bitset_nfa: bool = False) -> PatternSet:
    return PatternSet(patterns, lazydfa_semantics=lazydfa_semantics, bitset_nfa=bitset_nfa)


# ---------------------------------------------------------------------------------
# module-level API with the reference's process-wide cache (matcher.mojo:1166-1321)
# ---------------------------------------------------------------------------------
_CACHE = {}


def compile_regex(pattern, lazydfa_semantics: bool = False, bitset_nfa: bool = False,
                  nfa_engine: bool = False, dfa_engine: bool = False) -> CompiledRegex:
    key = (_b(pattern), bool(lazydfa_semantics), bool(bitset_nfa), bool(nfa_engine), bool(dfa_engine))
    c = _CACHE.get(key)
    if c is None:
        c = CompiledRegex(key[0], lazydfa_semantics, bitset_nfa, nfa_engine, dfa_engine)
        _CACHE[key] = c
    return c


def clear_regex_cache():
    _CACHE.clear()


def match_first(pattern, texts):
    return compile_regex(pattern).match_first(texts)


def search(pattern, texts):
    return compile_regex(pattern).match_next(texts)


def findall(pattern, texts):
    return compile_regex(pattern).match_all(texts)


def captures_all(pattern, texts, count: int = 0):
    """Capture groups of every match per text: (match_prefix int64[n+1], groups int32[total, g+1, 2])."""
    return compile_regex(pattern).captures_all(texts, count)


def sub(pattern, repl, texts, count: int = 0) -> List[bytes]:
    return compile_regex(pattern).sub(repl, texts, count)


def filter_texts(pattern, texts, invert: bool = False):
    """CompiledRegex.filter through the cache (the name leaves the builtin filter alone)."""
    return compile_regex(pattern).filter(texts, invert)


def findall_texts(pattern, texts):
    """CompiledRegex.extract through the cache: findall's matches as bytes (re.findall's strings)."""
    return compile_regex(pattern).extract(texts)


def distinct(texts, sort: Optional[str] = None, top: Optional[int] = None):
    """The unique texts of a list and how often each occurs, through mrx_distinct_batch: (values List[bytes], counts
    int64[u], group_of int64[n], first int64[u]) as numpy arrays, the values in the order of dict.fromkeys(texts).
    sort="value" / "count" and top=k reorder and cut the rows as CompiledRegex.value_counts does (on the device:
    DeviceBatch.distinct, argsort and take); group_of then holds the new row of every text, -1 for a text whose value
    top cut away."""
    lib = load_library()
    bs = [_b(t) for t in texts]
    if sort is not None or top is not None:
        import torch
        values, counts, group_of, first = DeviceBatch.from_texts(bs).distinct()
        order = _row_order(values, counts, sort, top)
        if order is not None:
            new_row = torch.full((values.n,), -1, dtype=torch.int64, device=order.device)
            new_row[order] = torch.arange(order.numel(), dtype=torch.int64, device=order.device)
            values, counts, first, group_of = values.take(order), counts[order], first[order], new_row[group_of]
        raw, off = values.data.cpu().numpy().tobytes(), values.offsets.cpu().numpy()
        return ([raw[off[g]:off[g + 1]] for g in range(values.n)], counts.cpu().numpy(), group_of.cpu().numpy(),
                first.cpu().numpy())
    data, offsets = pack_texts(bs)
    n, nbytes = len(bs), int(offsets[-1])
    group_of, first, counts = (np.zeros(max(n, 1), np.int64) for _ in range(3))
    out_off = np.zeros(n + 1, np.int64)
    out = np.empty(max(nbytes, 1), np.uint8)
    totals = (C.c_int64 * 2)()
    _check(lib.mrx_distinct_batch(data.ctypes.data, offsets.ctypes.data, n, group_of.ctypes.data, first.ctypes.data,
                                  counts.ctypes.data, out_off.ctypes.data, out.ctypes.data, nbytes,
                                  C.cast(totals, C.c_void_p)))
    u = int(totals[0])
    raw = out[:int(totals[1])].tobytes()
    return ([raw[out_off[g]:out_off[g + 1]] for g in range(u)], counts[:u].copy(), group_of[:n].copy(),
            first[:u].copy())


def lines_of(texts, sep=b"\n", keepends: bool = False, crlf: bool = False, partial: bool = True):
    """The lines of host texts (DeviceBatch.lines): a list of texts gives List[List[bytes]], one bytes object its
    List[bytes]."""
    single = isinstance(texts, (bytes, bytearray, memoryview, str))
    batch = DeviceBatch.from_texts([_b(texts)] if single else [_b(t) for t in texts])
    pieces, prefix, _ = batch.lines(sep, keepends, crlf, partial)
    out = _piece_lists(pieces, prefix)
    return out[0] if single else out


def fields_of(texts, columns, delim=None, rest: bool = False, quote=None):
    """The columns of host texts (DeviceBatch.fields): List[List[Optional[bytes]]], one list per text with the bytes of
    every requested column, None for a part that the text does not have.  With quote: the contents of quoted fields."""
    bs = [_b(t) for t in texts]
    _fields_args(columns, delim, rest)
    if quote is not None:
        _quote_byte(quote)
    if not bs:
        return []
    rows = DeviceBatch.from_texts(bs).fields(columns, delim, rest, counts=False, quote=quote)[1]
    rows = rows.cpu().numpy()
    return [[None if s < 0 else t[s:e] for s, e in rows[i].tolist()] for i, t in enumerate(bs)]


_unescape_keywords = {}   # csv_columns(): the one-entry keyword set QQ per quote byte, built once


def csv_columns(batch: "DeviceBatch", columns, delim=b",", quote=b'"', unescape: bool = True):
    """The cells of the named columns of every text of a DeviceBatch as CSV understands them: one packed DeviceBatch of
    n texts per column.  fields(quote=) gives the contents, gather_spans(pair=j) packs them (a column that a text does
    not have is an empty text), and with unescape every doubled quote becomes one: Keywords([QQ]).sub(Q, ...), leftmost
    and non-overlapping.  For rows that csv.writer wrote (QUOTE_MINIMAL or QUOTE_ALL, cells without \\r and \\n) these
    are csv.reader's cells; what malformed rows give is include/mrx.h's to say ("quoted fields")."""
    q = bytes([_quote_byte(quote)])
    prefix, rows, _, _ = batch.fields(columns, delim, counts=False, quote=q)
    out = []
    for j in range(len(columns)):
        cells = batch.gather_spans(prefix, rows, pair=j)[0]
        if unescape:
            kw = _unescape_keywords.get(q)
            if kw is None:
                kw = _unescape_keywords[q] = Keywords([q + q])
            cells = kw.sub(q, cells)
        out.append(cells)
    return out


def csv_of(texts, columns, delim=b",", quote=b'"') -> List[List[bytes]]:
    """csv_columns of host texts: one list per text with the decoded cell of every requested column, b""
    for a column that the text does not have."""
    bs = [_b(t) for t in texts]
    _fields_args(columns, delim, False)
    _quote_byte(quote)
    if not bs:
        return []
    cols = []
    for cells in csv_columns(DeviceBatch.from_texts(bs), columns, delim, quote):
        raw, off = cells.data.cpu().numpy().tobytes(), cells.offsets.cpu().numpy()
        cols.append([raw[off[i]:off[i + 1]] for i in range(len(bs))])
    return [list(cell) for cell in zip(*cols)]


def translate_texts(texts, table=None, delete=b"", squeeze=b"") -> List[bytes]:
    """DeviceBatch.translate of host texts: [t.translate(table, delete) for t in texts], then tr -s over `squeeze`."""
    bs = [_b(t) for t in texts]
    _translate_args(table, delete, squeeze)
    if not bs:
        return []
    res = DeviceBatch.from_texts(bs).translate(table, delete, squeeze)
    raw, off = res.data.cpu().numpy().tobytes(), res.offsets.cpu().numpy()
    return [raw[off[i]:off[i + 1]] for i in range(len(bs))]


def strip_texts(texts, chars=None, left: bool = True, right: bool = True) -> List[bytes]:
    """DeviceBatch.strip of host texts: [t.strip(chars) for t in texts] (lstrip / rstrip with one side off)."""
    bs = [_b(t) for t in texts]
    if not (left or right):
        raise MrxError("strip needs left, right or both")
    if not bs:
        return []
    _, rows = DeviceBatch.from_texts(bs).strip(chars, left, right, spans=True)
    return [t[int(a):int(b)] for t, (a, b) in zip(bs, rows.cpu().numpy().reshape(-1, 2))]


def build_dictionary(entries) -> Dictionary:
    """Dictionary(entries): a list of texts or a DeviceBatch."""
    return Dictionary(entries)


def build_sorted_index(entries) -> SortedIndex:
    """SortedIndex(entries): a list of texts or a DeviceBatch."""
    return SortedIndex(entries)


def searchsorted(entries, texts, side: str = "left"):
    """bisect.bisect_left (or, with side="right", bisect_right) of every text among sorted(entries), through
    mrx_sorted_search_batch: np.int64[n].  One index for one batch; build_sorted_index keeps it for many."""
    if side not in ("left", "right"):
        raise MrxError("side must be 'left' or 'right'")
    lib = load_library()
    es, bs = [_b(t) for t in entries], [_b(t) for t in texts]
    edata, eoff = pack_texts(es)
    data, off = pack_texts(bs)
    pos = np.zeros(max(len(bs), 1), np.int64)
    lo, hi = (pos.ctypes.data, None) if side == "left" else (None, pos.ctypes.data)
    _check(lib.mrx_sorted_search_batch(edata.ctypes.data, eoff.ctypes.data, len(es), MRX_SORTED_EQUAL, data.ctypes.data,
                                       off.ctypes.data, len(bs), lo, hi))
    return pos[:len(bs)].copy()


def build_keywords(entries, ignore_case: bool = False) -> Keywords:
    """Keywords(entries, ignore_case): a list of byte strings or a DeviceBatch."""
    return Keywords(entries, ignore_case)


def keywords_filter(entries, texts, invert: bool = False):
    """The texts in which some entry occurs (with invert, the others): one keyword set for one batch;
    build_keywords keeps it for many."""
    return Keywords(entries).filter(texts, invert)


def keywords_sub(entries, repl, texts, ignore_case: bool = False, count: int = 0):
    """Keywords(entries, ignore_case).sub(repl, texts, count): one keyword set for one batch; build_keywords keeps it for
    many."""
    return Keywords(entries, ignore_case).sub(repl, texts, count)


def lookup(entries, texts):
    """For every text the lowest index of an entry equal to it, or -1, through mrx_dict_lookup_batch: np.int64[n].
    One dictionary for one batch; build_dictionary keeps it for many."""
    lib = load_library()
    es, bs = [_b(t) for t in entries], [_b(t) for t in texts]
    edata, eoff = pack_texts(es)
    data, off = pack_texts(bs)
    index = np.zeros(max(len(bs), 1), np.int64)
    _check(lib.mrx_dict_lookup_batch(edata.ctypes.data, eoff.ctypes.data, len(es), data.ctypes.data, off.ctypes.data,
                                     len(bs), index.ctypes.data))
    return index[:len(bs)].copy()


def value_counts(pattern, texts, group: Optional[int] = None, count: int = 0, sort: Optional[str] = None,
                 top: Optional[int] = None):
    """compile_regex(pattern).value_counts(texts, group, count, sort, top)."""
    return compile_regex(pattern).value_counts(texts, group, count, sort, top)


def numbers(pattern, texts, kind: str = "int", group: Optional[int] = None, count: int = 0, fill=0):
    """compile_regex(pattern).numbers(texts, kind, group, count, fill): the pattern's matches as numbers."""
    return compile_regex(pattern).numbers(texts, kind, group, count, fill)


def parse_numbers(texts, kind: str = "int"):
    """int(t), int(t, 16) or float(t) for a list of texts, through mrx_parse_batch: List[Optional[int | float]], None
    where a text is not a number of that kind (include/mrx.h, "numbers": no whitespace, no underscores, no inf or nan)
    or is not answered (an integer outside int64; a float outside the exact rule)."""
    lib = load_library()
    k = _num_kind(kind)
    bs = [_b(t) for t in texts]
    data, offsets = pack_texts(bs)
    n = len(bs)
    values, status = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.uint8)
    _check(lib.mrx_parse_batch(data.ctypes.data, offsets.ctypes.data, n, k, 0, values.ctypes.data, status.ctypes.data))
    vals = (values.view(np.float64) if kind == "float" else values)[:n].tolist()
    return [v if s == MRX_NUM_OK else None for v, s in zip(vals, status[:n].tolist())]


MRX_COL_TEXT, MRX_COL_INT10, MRX_COL_INT16, MRX_COL_FIXED = range(4)
_FMT_CELL_MAX = 21   # the longest number cell: a sign and 20 digits
_FMT_BOUND_FIRST = 1 << 26   # a known bound of the output up to here is the first capacity: no retry is ever needed
_FMT_NUMBER_GUESS = 12       # ... beyond it a number cell is guessed at a sign and 11 digits, and the call may run twice


class _Column(C.Structure):
    """mrx_column of include/mrx.h."""
    _fields_ = [("kind", C.c_int32), ("arg", C.c_int32), ("d_values", C.c_void_p), ("d_offsets", C.c_void_p),
                ("stride", C.c_int64), ("d_lens", C.c_void_p), ("len", C.c_int32), ("pad_", C.c_int32),
                ("d_status", C.c_void_p)]


def _fmt_spec(spec) -> Tuple[int, int]:
    """(kind, arg) of a printf-like spec: "d", ".Kd", "x", ".Kx" (K = 0..20) or ".Pf" (P = 0..9)."""
    if not isinstance(spec, str) or not spec or spec[-1] not in "dxf":
        raise MrxError("a column's spec must be 'd', '.Kd', 'x', '.Kx' or '.Pf', not %r" % (spec,))
    letter, prec = spec[-1], spec[:-1]
    if prec == "" and letter != "f":
        return (MRX_COL_INT10 if letter == "d" else MRX_COL_INT16), 0
    if len(prec) < 2 or len(prec) > 3 or prec[0] != "." or not prec[1:].isdigit() or not prec[1:].isascii():
        raise MrxError("a column's spec must be 'd', '.Kd', 'x', '.Kx' or '.Pf', not %r" % (spec,))
    arg = int(prec[1:])
    if letter == "f":
        if arg > 9:
            raise MrxError("the precision P of '.Pf' must be in [0, 9]")
        return MRX_COL_FIXED, arg
    if arg > 20:
        raise MrxError("the digits K of '.K%s' must be in [0, 20]" % letter)
    return (MRX_COL_INT10 if letter == "d" else MRX_COL_INT16), arg


def _fmt_split(col):
    """(values, spec or None, status or None) of one entry of `columns`: a pair or triple is a tuple whose second
    element is the spec."""
    if isinstance(col, tuple) and len(col) in (2, 3) and isinstance(col[1], str):
        return col[0], col[1], (col[2] if len(col) == 3 else None)
    return col, None, None


def _fmt_device_columns(template: bytes, columns):
    """The columns of a device call: (mrx_column array, n, device, longest record or None, first capacity, what the
    array's pointers keep alive).  Every error of a spec, a dtype or a row count is raised here, before any device
    call."""
    import torch
    if not 1 <= len(columns) <= 9:
        raise MrxError("format takes 1 to 9 columns")
    arr = (_Column * len(columns))()
    refs = _template_ref_list(template)
    keep, n, dev, bounds, sizes = [], None, None, [], []
    for j, col in enumerate(columns):
        values, spec, status = _fmt_split(col)
        c = arr[j]
        if isinstance(values, DeviceBatch):
            if spec is not None or status is not None:
                raise MrxError("a text column takes no spec and no status")
            rows, where = values.n, values.data.device
            data = values.data
            if data.numel() == 0:   # (texts without a byte: the ABI still wants a pointer)
                data = torch.zeros(16, dtype=torch.uint8, device=where)
            c.kind, c.arg, c.d_values, c.d_offsets = MRX_COL_TEXT, 0, _ptr(data), _ptr(values.offsets)
            c.stride, c.d_lens, c.len = values.stride, _ptr(values.lens), values.length
            keep += [data, values]
            bounds.append(values.longest())
            sizes.append(int(values.data.numel()))
        elif isinstance(values, torch.Tensor):
            if values.dim() != 1 or not values.is_contiguous():
                raise MrxError("a number column must be a contiguous one-dimensional tensor")
            if spec is None:
                if values.dtype != torch.int64:
                    raise MrxError("a %s column needs a spec ('.Pf' for float64)" % values.dtype)
                spec = "d"
            kind, arg = _fmt_spec(spec)
            if values.dtype != (torch.float64 if kind == MRX_COL_FIXED else torch.int64):
                raise MrxError("spec %r does not fit a %s column" % (spec, values.dtype))
            rows, where = int(values.numel()), values.device
            if status is not None:
                if (not isinstance(status, torch.Tensor) or status.dtype != torch.uint8 or not status.is_contiguous()
                        or status.numel() != rows or status.device != where):
                    raise MrxError("a column's status must be a contiguous uint8[n] tensor on the values' device")
            c.kind, c.arg, c.d_values, c.d_status = kind, arg, _ptr(values) if rows else 0, _ptr(status)
            keep += [values, status]
            bounds.append(_FMT_CELL_MAX)
            sizes.append(_FMT_NUMBER_GUESS * rows)
        else:
            raise MrxError("a column must be a DeviceBatch, a tensor, (tensor, spec) or (tensor, spec, status)")
        if n is None:
            n, dev = rows, where
        elif rows != n:
            raise MrxError("columns of different row counts: %d and %d" % (n, rows))
        elif where != dev:
            raise MrxError("columns on different devices")
    used = [j for j in refs if j <= len(columns)]
    longest = None
    if all(bounds[j - 1] is not None for j in used):
        longest = len(template) + sum(int(bounds[j - 1]) for j in used)
    if longest is not None and n * longest <= _FMT_BOUND_FIRST:
        first = n * longest
    else:   # an estimate: every byte of a referenced text column once per reference, 12 bytes a number
        first = n * len(template) + sum(sizes[j - 1] for j in used)
    return arr, n, dev, longest, first, keep


def _fmt_host_column(values, spec):
    """One host list as numpy arrays: a list of texts for a text column (bytes; None = an empty text), or (values,
    spec, status) for a number column, whose None rows carry the status MRX_NUM_EMPTY.  Host work only."""
    values = list(values)
    some = next((v for v in values if v is not None), None)
    if spec is None and (some is None or isinstance(some, (bytes, bytearray, str))):
        return [b"" if v is None else _b(v) for v in values]
    if spec is None:
        if isinstance(some, float):
            raise MrxError("a float column needs a spec ('.Pf')")
        spec = "d"
    kind, _ = _fmt_spec(spec)
    try:
        if kind == MRX_COL_FIXED:
            host = np.array([0.0 if v is None else float(v) for v in values], np.float64)
        else:
            if any(v is not None and not isinstance(v, (int, np.integer)) for v in values):
                raise MrxError("spec %r does not fit a column of %s" % (spec, type(some).__name__))
            host = np.array([0 if v is None else int(v) for v in values], np.int64)
    except (OverflowError, TypeError, ValueError) as e:
        raise MrxError("spec %r does not fit the column: %s" % (spec, e))
    return host, spec, np.array([MRX_NUM_EMPTY if v is None else MRX_NUM_OK for v in values], np.uint8)


def format_records(template, columns, out_cap: Optional[int] = None, status: bool = False):
    """One record per row from a template, text columns and number columns, packed back to back on the device
    (include/mrx.h, mrx_format_dev): the inverse of numbers, shaped like expand.  template has sub's grammar -- \\1..\\9
    name the columns, every other byte is literal; a reference to a column that is not there contributes nothing.
    A column is a DeviceBatch (the row's text), an int64 tensor (spec "d"), (tensor, spec) or (tensor, spec, status):
    the cell is b"%<spec>" % value byte for byte, with spec "d" / ".Kd" / "x" / ".Kx" (K = 0..20) for int64 and ".Pf"
    (P = 0..9) for float64.  A ".Pf" cell is exact or refused: correctly rounded from the binary value, ties to even,
    where round(|v| * 10^P) is below 10^19; NaN, the infinities and larger values print nothing.  status is the uint8
    tensor that numbers / parse wrote beside the values: a cell whose byte is not 0 prints nothing.
    Returns the records as a CSR DeviceBatch with known bounds -- its data tensor is the report as it stands, and the
    batch feeds distinct, a Dictionary or any other call.  status=True also returns the row status, uint8[n]: 0 where
    every referenced cell was written, else the status of the lowest-numbered referenced column whose cell was not (its
    input byte, or 3 for a refused cell).  Without out_cap the output grows to what the records need; an out_cap of the
    caller's that does not hold them raises MrxError.
    When every column is a host list -- of bytes, of int, or of float with a spec; None = nothing -- the call uploads
    them, runs the same kernels and returns List[bytes] (and with status=True the row status as a numpy array)."""
    import torch
    template = _b(template)
    columns = list(columns)
    host = [not isinstance(_fmt_split(c)[0], (DeviceBatch, torch.Tensor)) for c in columns]
    if columns and all(host):
        if not 1 <= len(columns) <= 9:
            raise MrxError("format takes 1 to 9 columns")
        staged = [_fmt_host_column(v, spec) for v, spec, _ in map(_fmt_split, columns)]
        if len({len(c) if isinstance(c, list) else len(c[0]) for c in staged}) != 1:
            raise MrxError("columns of different row counts")
        up = lambda a: torch.from_numpy(a).to("cuda")   # noqa: E731
        res = format_records(template, [DeviceBatch.from_texts(c) if isinstance(c, list) else (up(c[0]), c[1], up(c[2]))
                                        for c in staged], out_cap, True)
        raw, off = res[0].data.cpu().numpy().tobytes(), res[0].offsets.cpu().numpy()
        records = [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        return (records, res[1].cpu().numpy()) if status else records
    if any(host):
        raise MrxError("columns must all be device columns or all be host lists")
    arr, n, dev, longest, first, keep = _fmt_device_columns(template, columns)
    out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    row_status = torch.empty(n, dtype=torch.uint8, device=dev) if status else None
    d_totals = torch.empty(2, dtype=torch.int64, device=dev)
    totals = (C.c_int64 * 2)()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib = load_library()

    def run(out, cap, total):
        rc = lib.mrx_format_dev(template, len(template), C.cast(arr, C.c_void_p), len(columns), n, _ptr(out_off), _ptr(out), cap,
                                _ptr(row_status), _ptr(d_totals), C.cast(totals, C.c_void_p), stream)
        total._obj.value = int(totals[1])
        return rc
    with torch.cuda.device(dev):
        out, nbytes = _grow_call(first if out_cap is None else int(out_cap),
                                 lambda cap: torch.empty(max(cap, 1), dtype=torch.uint8, device=dev), run,
                                 grow=out_cap is None, only_larger=True)
    del keep
    data = out[:nbytes].clone() if 4 * nbytes < out.numel() else out[:nbytes]
    records = DeviceBatch(data, out_off) if longest is None else DeviceBatch.csr_known(data, out_off, nbytes, longest)
    return (records, row_status) if status else records


def format_numbers(values, spec: str = "d", status=None):
    """One column under the template \\1, the inverse of parse: every value written as b"%<spec>" % value, as a
    DeviceBatch for a tensor and as List[bytes] for a host list (None = nothing).  status: the uint8 tensor that parse
    wrote beside the values; rows whose byte is not 0 become empty texts."""
    import torch
    if isinstance(values, torch.Tensor):
        return format_records(b"\\1", [(values, spec) if status is None else (values, spec, status)])
    if status is not None:
        values = [v if s == MRX_NUM_OK else None for v, s in zip(values, status)]
    return format_records(b"\\1", [(list(values), spec)])


def format_records_async(template, columns, out):
    """Enqueue format_records on the current stream without reading anything back.  columns are device columns; out =
    (out_offsets int64[n + 1], out_data uint8[cap], totals int64[2]) or, with a fourth entry, (..., row_status
    uint8[n]), device tensors of the caller; totals = {n, bytes} once the stream has drained.  No byte is written when
    bytes > cap (check totals[1])."""
    import torch
    template = _b(template)
    arr, n, dev, _, _, keep = _fmt_device_columns(template, list(columns))
    out_offsets, out_data, totals = out[:3]
    row_status = out[3] if len(out) > 3 else None
    if out_offsets.numel() < n + 1 or totals.numel() < 2:
        raise MrxError("out needs out_offsets int64[n + 1], out_data uint8[cap], totals int64[2]")
    for t in (out_offsets, totals):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise MrxError("out_offsets and totals must be contiguous int64 tensors")
    for t in (out_data, row_status):
        if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous()):
            raise MrxError("out_data and row_status must be contiguous uint8 tensors")
    if row_status is not None and row_status.numel() < n:
        raise MrxError("row_status needs n entries")
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _check(load_library().mrx_format_dev(template, len(template), C.cast(arr, C.c_void_p), len(arr), n, _ptr(out_offsets),
                                         _ptr(out_data), int(out_data.numel()), _ptr(row_status), _ptr(totals), None, stream))
    del keep


def sort_texts(texts):
    """sorted(texts) for a list of texts, through mrx_sort_batch: (List[bytes] in ascending order, order int64[n] as a
    numpy array with order[p] the index of the text at sorted position p).  Texts compare as Python's bytes do and equal
    texts keep their index order."""
    lib = load_library()
    bs = [_b(t) for t in texts]
    data, offsets = pack_texts(bs)
    n = len(bs)
    order = np.zeros(max(n, 1), np.int64)
    _check(lib.mrx_sort_batch(data.ctypes.data, offsets.ctypes.data, n, order.ctypes.data, None, None))
    order = order[:n].copy()
    return [bs[int(i)] for i in order], order


def expand(pattern, template, texts, count: int = 0):
    """CompiledRegex.expand through the cache: one templated record per match ([m.expand(t) for m in re.finditer])."""
    return compile_regex(pattern).expand(template, texts, count)


def split(pattern, texts, maxsplit: int = 0) -> List[List[bytes]]:
    """regex.split (matcher.mojo:1357-1393) through the C ABI (mrx_split_batch): pieces as byte ranges per text."""
    return compile_regex(pattern).split(texts, maxsplit)
