"""ctypes binding of libsparse_rx.so (C ABI declared in include/sparse_rx.h, include/sparse_rx_rescore.h,
include/sparse_rx_quant.h, include/sparse_rx_filter.h, include/sparse_rx_half.h, include/sparse_rx_mmr.h,
include/sparse_rx_terms.h, include/sparse_rx_maxsim.h, include/sparse_rx_fields.h, include/sparse_rx_collapse.h,
include/sparse_rx_facets.h, include/ext/sparse_rx_feedback.h, include/order/sparse_rx_order.h, include/boost/sparse_rx_boost.h,
include/ltr/sparse_rx_ltr.h, include/eval/sparse_rx_eval.h and include/binary/sparse_rx_binary.h).

The library is the product: there is no CPU fallback.  If it is missing or cannot be loaded every entry point
raises ``SparseRxUnavailable`` -- loudly, never a silent eager path.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from typing import Optional

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG_DIR)
LIB_PATH = os.path.join(_PKG_DIR, "libsparse_rx.so")
CSRC_DIR = os.path.join(_PKG_DIR, "csrc")
SOURCES = ["wave_kernel.hip", "tier2_kernel.hip", "merge.hip", "build.hip", "sparse_rx.hip", "dense.hip", "fuse.hip",
           "score_docs.hip", "dense_score.hip", "dense_quant.hip", "filter.hip", "tier2_filter.hip", "dense_half.hip", "mmr.hip",
           "terms.hip", "maxsim.hip", "fields.hip", "collapse.hip", "facets.hip", "feedback.hip", "order.hip", "boost.hip", "ltr.hip",
           "eval.hip", "dense_binary.hip"]  # one translation unit each, compiled in parallel
INCLUDED_SOURCES = {"tier2_filter.hip": ["tier2_kernel.hip"]}  # a unit that compiles another source file as part of itself
SRC_PATH = os.path.join(CSRC_DIR, "wave_kernel.hip")            # the dominant kernel's source (bench.py hashes it)
INCLUDE_DIR = os.path.join(_ROOT, "include")

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-std=c++17"]

SRX_VAL_F32, SRX_VAL_F16 = 0, 1
SRX_FUSE_WEIGHTED, SRX_FUSE_RRF = 0, 1
SRX_MAX_K = 1024  # rows per query list inside the engine (limits()["max_k"]; pinned to the library by tests/test_capi_cpu.py)


class SparseRxUnavailable(RuntimeError):
    """libsparse_rx.so is not built / not loadable (the HIP engine is mandatory)."""


class SparseRxError(RuntimeError):
    """A C-ABI call returned a negative status."""


class IndexDesc(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("val_type", ctypes.c_int32), ("n_docs", ctypes.c_int64),
                ("vocab", ctypes.c_int64), ("nnz", ctypes.c_int64), ("n_blocks", ctypes.c_int64), ("doc_base", ctypes.c_int64),
                ("tile_log2", ctypes.c_int32), ("n_tiles", ctypes.c_int32), ("unit_tiles", ctypes.c_int32),
                ("reserved0", ctypes.c_int32), ("term_ptr", ctypes.c_void_p), ("post", ctypes.c_void_p),
                ("tile_skip", ctypes.c_void_p), ("idf", ctypes.c_void_p), ("term_bound", ctypes.c_void_p),
                ("post16", ctypes.c_void_p)]


class SearchOpts(ctypes.Structure):
    _fields_ = [("supertile_log2", ctypes.c_int32), ("target_blocks", ctypes.c_int32), ("profile", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("unit_tiles", ctypes.c_int32)]


# every symbol include/sparse_rx.h declares: name -> (restype, argtypes)
_VP, _I32, _I64, _DBL = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
SYMBOLS = {
    "srx_version": (ctypes.c_int, []),
    "srx_last_error": (ctypes.c_char_p, []),
    "srx_limits": (ctypes.c_int, [ctypes.POINTER(_I32)]),
    "srx_device_count": (ctypes.c_int, []),
    "srx_index_create": (ctypes.c_int, [ctypes.POINTER(IndexDesc), ctypes.POINTER(_VP)]),
    "srx_index_destroy": (None, [_VP]),
    "srx_index_set_opts": (ctypes.c_int, [_VP, ctypes.POINTER(SearchOpts)]),
    "srx_search_workspace_bytes": (_I64, [_VP, _I32, _I32]),
    "srx_search": (ctypes.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_search_after": (ctypes.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_search_after_packed": (ctypes.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_merge_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    "srx_merge_topk": (ctypes.c_int, [_I32, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_merge_topk_packed": (ctypes.c_int, [_I32, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_search_packed": (ctypes.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _VP, _I64, _VP]),
    "srx_merge_topk_packed_out": (ctypes.c_int, [_I32, _VP, _I32, _I32, _I32, _VP, _VP, _I64, _VP]),
    "srx_dense_workspace_bytes": (_I64, [_I32, _I64, _I32]),
    "srx_dense_search_i8": (ctypes.c_int, [_I32, _VP, _VP, _I64, _I32, _VP, _VP, _I32, _I32, _I64, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_dense_packed_bytes": (_I64, [_I64, _I32]),
    "srx_dense_pack_i8": (ctypes.c_int, [_I32, _VP, _I64, _I32, _VP, _VP]),
    "srx_dense_search_i8_packed": (ctypes.c_int, [_I32, _VP, _VP, _I64, _I32, _VP, _VP, _I32, _I32, _I64, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_dense_f32_workspace_bytes": (_I64, [_I32, _I64, _I32]),
    "srx_dense_search_f32": (ctypes.c_int, [_I32, _VP, _I64, _I32, _VP, _I32, _I32, _I64, _VP, _VP, _VP, _VP, _I64, _VP, ctypes.c_float]),
    "srx_dense_search_u8": (ctypes.c_int, [_I32, _VP, _VP, _I64, _I32, _VP, _I32, _I32, _I64, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_fuse_topk": (ctypes.c_int, [_I32, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _I32, _I32, _I32, _I32, ctypes.c_float, ctypes.c_float,
                                     ctypes.c_float, _VP, _VP, _VP, _VP]),
    "srx_score_docs": (ctypes.c_int, [ctypes.POINTER(IndexDesc), _VP, _VP, _VP, _I32, _VP, _VP, _I32, _VP, _VP]),
    "srx_build_impacts": (ctypes.c_int, [_I32, _VP, _VP, _VP, _I64, _DBL, _DBL, _DBL, _VP, _VP]),
    "srx_build_tile_skip": (ctypes.c_int, [_I32, _VP, _VP, _I64, _I32, _I32, _VP, _VP]),
    "srx_memcpy_async": (ctypes.c_int, [_VP, _VP, _I64, _VP]),
    "srx_auto_unit_tiles": (_I32, [_I64, _I64, _I64, _I32]),
    "srx_build_blocks": (ctypes.c_int, [_I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I64, _I32, _I32, _I32, _VP, _VP, _VP, _I64, _VP]),
    "srx_build_compact": (ctypes.c_int, [_I32, _I32, _VP, _I64, _I32, _I32, _VP, _VP]),
    "srx_build_term_bounds": (ctypes.c_int, [_I32, _I32, _VP, _VP, _I64, _VP, _I32, _VP, _VP, _VP]),
    "srx_build_sum_duplicates": (ctypes.c_int, [_I32, _VP, _I64, _VP, _VP, _VP]),
    "srx_profile_read": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_float)]),
}

# every symbol include/sparse_rx_rescore.h declares (the second header of the same library)
_F32 = ctypes.c_float
RESCORE_SYMBOLS = {
    "srx_dense_score_docs_f32": (ctypes.c_int, [_I32, _VP, _I64, _I32, _VP, _I32, _I64, _VP, _VP, _I32, _VP, _VP]),
    "srx_dense_score_docs_u8": (ctypes.c_int, [_I32, _VP, _VP, _I64, _I32, _VP, _I32, _I64, _VP, _VP, _I32, _VP, _VP]),
    "srx_dense_score_docs_i8": (ctypes.c_int, [_I32, _VP, _I32, _VP, _I64, _I32, _VP, _VP, _I32, _I64, _VP, _VP, _I32, _VP, _VP]),
    "srx_fuse_topk_scored": (ctypes.c_int, [_I32, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _F32, _F32,
                                            _VP, _VP, _VP, _VP]),
}

# every symbol include/sparse_rx_quant.h declares (the third header of the same library)
QUANT_SYMBOLS = {
    "srx_dense_quantize_i8": (ctypes.c_int, [_I32, _VP, _I64, _I64, _I32, _I32, _I64, _I64, _I32, _VP, _VP, _VP, _VP]),
    "srx_dense_quantize_u8": (ctypes.c_int, [_I32, _VP, _I64, _I64, _I32, _I32, _I64, _I64, _VP, _VP, _VP, _VP]),
    "srx_dense_quantize_queries_i8": (ctypes.c_int, [_I32, _VP, _I64, _I32, _I32, _I32, _VP, _VP, _VP, _VP]),
    "srx_dense_quantize_queries_u8": (ctypes.c_int, [_I32, _VP, _I64, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
}
SRX_QUANT_NONFINITE, SRX_QUANT_DEGENERATE = 1, 2  # bits of the quantisers' flag word


class DocFilterDesc(ctypes.Structure):
    """``srx_doc_filter`` (include/sparse_rx_filter.h): a host struct of device pointers"""
    _fields_ = [("bits", ctypes.c_void_p), ("n_filters", ctypes.c_int32), ("q_filter", ctypes.c_void_p)]


# every symbol include/sparse_rx_filter.h declares (the fourth header of the same library)
_FP = ctypes.POINTER(DocFilterDesc)
FILTER_SYMBOLS = {
    "srx_filter_words": (_I64, [_I64]),
    "srx_filter_fill": (ctypes.c_int, [_I32, _VP, _I32, _I64, _I32, _VP]),
    "srx_filter_set_docs": (ctypes.c_int, [_I32, _VP, _I64, _I64, _VP, _I64, _I32, _VP]),
    "srx_filter_count": (ctypes.c_int, [_I32, _VP, _I32, _I64, _VP, _VP]),
    "srx_search_filtered": (ctypes.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _FP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_search_filtered_packed": (ctypes.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _FP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_dense_search_f32_filtered": (ctypes.c_int, [_I32, _VP, _I64, _I32, _VP, _I32, _I32, _I64, _FP, _VP, _VP, _VP, _VP, _I64, _VP,
                                                     ctypes.c_float]),
    "srx_dense_search_u8_filtered": (ctypes.c_int, [_I32, _VP, _VP, _I64, _I32, _VP, _I32, _I32, _I64, _FP, _VP, _VP, _VP, _VP, _I64, _VP]),
}

# every symbol include/sparse_rx_half.h declares (the fifth header of the same library)
HALF_SYMBOLS = {
    "srx_dense_half_bytes": (_I64, [_I64, _I32]),
    "srx_dense_convert_half": (ctypes.c_int, [_I32, _I32, _VP, _I64, _I64, _I32, _I32, _I64, _I64, _VP, _VP, _VP]),
    "srx_dense_half_workspace_bytes": (_I64, [_I32, _I64, _I32]),
    "srx_dense_search_half": (ctypes.c_int, [_I32, _I32, _VP, _I64, _I32, _VP, _I32, _I32, _I64, _FP, _VP, _VP, _VP, _VP, _I64, _VP, ctypes.c_float]),
    "srx_dense_score_docs_half": (ctypes.c_int, [_I32, _I32, _VP, _I64, _I32, _VP, _I32, _I64, _VP, _VP, _I32, _VP, _VP]),
}
SRX_HALF_F16, SRX_HALF_BF16 = 0, 1  # srx_half_type

# every symbol include/sparse_rx_mmr.h declares (the sixth header of the same library)
_MMR_TAIL = [_I64, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, _F32, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP]  # doc_base .. stream
MMR_SYMBOLS = {
    "srx_mmr_workspace_bytes": (_I64, [_I32, _I32]),
    "srx_mmr_select_f32": (ctypes.c_int, [_I32, _VP, _I64, _I32, *_MMR_TAIL]),
    "srx_mmr_select_half": (ctypes.c_int, [_I32, _I32, _VP, _I64, _I32, *_MMR_TAIL]),
}
SRX_MMR_DOT, SRX_MMR_COSINE = 0, 1  # srx_mmr_sim
SRX_MMR_MAX_M = 256                 # candidates per list (pinned to the header by tests/test_mmr_cpu.py)

# every symbol include/sparse_rx_terms.h declares (the seventh header of the same library)
TERMS_SYMBOLS = {
    "srx_filter_from_terms_bytes": (_I64, [_I64, _I64]),
    "srx_filter_from_terms": (ctypes.c_int, [ctypes.POINTER(IndexDesc), _I32, _VP, _VP, _VP, _VP, _VP, _VP, _FP, _VP, _VP]),
}

# every symbol include/sparse_rx_maxsim.h declares (the eighth header of the same library)
_MAXSIM_HEAD = [_I32, _I32, _VP, _I64, _I32, _VP, _I64, _I64, _VP, _VP, _I32, _I32, _VP, _VP, _I32]  # device .. m
MAXSIM_SYMBOLS = {
    "srx_maxsim_workspace_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "srx_maxsim_score_docs_half": (ctypes.c_int, [*_MAXSIM_HEAD, _VP, _VP, _I64, _VP]),
    "srx_maxsim_rerank_half": (ctypes.c_int, [*_MAXSIM_HEAD, _I32, _VP, _VP, _VP, _VP, _I64, _VP]),
}
SRX_MAXSIM_MAX_QT = 128  # query tokens per query (pinned to the header by tests/test_late_cpu.py)


class FieldColDesc(ctypes.Structure):
    """``srx_field_col`` (include/sparse_rx_fields.h): a host struct of device pointers"""
    _fields_ = [("data", ctypes.c_void_p), ("valid", ctypes.c_void_p), ("type", ctypes.c_int32)]


# every symbol include/sparse_rx_fields.h declares (the ninth header of the same library)
FIELDS_SYMBOLS = {
    "srx_filter_from_fields": (ctypes.c_int, [_I32, _I64, ctypes.POINTER(FieldColDesc), _I32, _VP, _I32, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP,
                                              _FP, _VP, _VP]),
}
SRX_FIELD_I32, SRX_FIELD_I64, SRX_FIELD_F32, SRX_FIELD_SET64 = 0, 1, 2, 3         # column types
SRX_FOP_RANGE, SRX_FOP_IN, SRX_FOP_MASK_ANY, SRX_FOP_MASK_ALL = 0, 1, 2, 3        # clause ops
SRX_FIELDS_MAX_COLS = 32                                                          # columns one call takes

# every symbol include/sparse_rx_collapse.h declares (the tenth header of the same library)
COLLAPSE_SYMBOLS = {
    "srx_collapse_topk": (ctypes.c_int, [_I32, ctypes.POINTER(FieldColDesc), _I64, _I64, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP,
                                         _VP, _VP, _VP]),
}
SRX_COLLAPSE_NULL_OWN, SRX_COLLAPSE_NULL_ONE, SRX_COLLAPSE_NULL_DROP = 0, 1, 2    # what a doc without a key is
SRX_COLLAPSE_MAX_M = 2048                                                         # positions per list (pinned to the header by tests/test_collapse_cpu.py)


class FacetBins(ctypes.Structure):
    """``srx_facet_bins`` (include/sparse_rx_facets.h): a host struct; ``edges`` is a device pointer"""
    _fields_ = [("mode", ctypes.c_int32), ("n_bins", ctypes.c_int32), ("origin", ctypes.c_int64), ("edges", ctypes.c_void_p)]


# every symbol include/sparse_rx_facets.h declares (the eleventh header of the same library)
_CP, _BP = ctypes.POINTER(FieldColDesc), ctypes.POINTER(FacetBins)
FACET_SYMBOLS = {
    "srx_facet_counts": (ctypes.c_int, [_I32, _CP, _I64, _BP, _FP, _I32, _VP, _VP, _VP]),
    "srx_facet_counts_lists": (ctypes.c_int, [_I32, _CP, _I64, _I64, _BP, _VP, _VP, _I32, _I32, _VP, _VP, _VP]),
}
SRX_FACET_CODES, SRX_FACET_LABELS, SRX_FACET_EDGES = 0, 1, 2                      # srx_facet_bins.mode
SRX_FACET_MAX_BINS = 8192                                                         # bins per facet (pinned to the header by tests/test_facets_cpu.py)



class ForwardDesc(ctypes.Structure):
    """``srx_forward_desc`` (include/ext/sparse_rx_feedback.h): a host struct of device pointers"""
    _fields_ = [("device", ctypes.c_int32), ("reserved", ctypes.c_int32), ("n_docs", ctypes.c_int64), ("vocab", ctypes.c_int64),
                ("doc_base", ctypes.c_int64), ("row_ptr", ctypes.c_void_p), ("term", ctypes.c_void_p), ("value", ctypes.c_void_p),
                ("doc_len", ctypes.c_void_p)]


class FeedbackParams(ctypes.Structure):
    """``srx_feedback_params`` (include/ext/sparse_rx_feedback.h): a host struct"""
    _fields_ = [("fb_docs", ctypes.c_int32), ("row_cap", ctypes.c_int32), ("n_terms", ctypes.c_int32), ("doc_weight", ctypes.c_int32),
                ("term_weight", ctypes.c_int32), ("alpha", ctypes.c_float), ("beta", ctypes.c_float)]


# every symbol include/ext/sparse_rx_feedback.h declares (the twelfth header of the same library)
FEEDBACK_SYMBOLS = {
    "srx_feedback_workspace_bytes": (_I64, [_I32]),
    "srx_feedback_expand": (ctypes.c_int, [ctypes.POINTER(ForwardDesc), ctypes.POINTER(FeedbackParams), _VP, _VP, _VP, _VP, _I32, _I64, _VP, _VP, _VP,
                                           _I32, _VP, _VP, _VP, _I64, _VP, _VP, _I64, _VP]),
}
SRX_FB_BY_SCORE, SRX_FB_UNIFORM = 0, 1                                            # srx_feedback_params.doc_weight
SRX_FB_RM, SRX_FB_RAW = 0, 1                                                      # srx_feedback_params.term_weight
SRX_FEEDBACK_MAX_DOCS, SRX_FEEDBACK_MAX_ENTRIES = 32, 4096                        # pinned to the header by tests/test_feedback_cpu.py
SRX_FEEDBACK_MAX_TERMS, SRX_FEEDBACK_MAX_QTERMS = 128, 128

# every symbol include/order/sparse_rx_order.h declares (the thirteenth header of the same library)
ORDER_SYMBOLS = {
    "srx_order_workspace_bytes": (_I64, [_I64, _I32, _I32]),
    "srx_order_topk": (ctypes.c_int, [_I32, _CP, _I64, _I64, _I32, _I32, _FP, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_order_lists": (ctypes.c_int, [_I32, _CP, _I64, _I64, _I32, _I32, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP]),
}
SRX_ORDER_ASC, SRX_ORDER_DESC = 0, 1                                              # order
SRX_ORDER_NULLS_LAST, SRX_ORDER_NULLS_FIRST, SRX_ORDER_NULLS_DROP = 0, 1, 2       # where the docs without a value go
SRX_ORDER_MAX_M = 2048                                                            # positions per list (pinned to the header by tests/test_order_cpu.py)
SRX_ORDER_MIN_SEG, SRX_ORDER_CHUNK = 32768, 8192                                  # the scan's segment rule (order_plan)


class BoostClause(ctypes.Structure):
    """``srx_boost_clause`` (include/boost/sparse_rx_boost.h): a DEVICE array element of 40 bytes"""
    _fields_ = [("col", ctypes.c_int32), ("flags", ctypes.c_int32), ("origin", ctypes.c_int64), ("inv_step", ctypes.c_float),
                ("weight", ctypes.c_float), ("missing", ctypes.c_float), ("knot0", ctypes.c_int32), ("n_seg", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


# every symbol include/boost/sparse_rx_boost.h declares (the fourteenth header of the same library)
BOOST_SYMBOLS = {
    "srx_boost_topk": (ctypes.c_int, [_I32, _CP, _I32, _I64, _I64, _VP, _I32, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32,
                                      _VP, _VP, _VP, _VP, _VP]),
}
SRX_BOOST_SCORE_MULTIPLY, SRX_BOOST_SCORE_SUM, SRX_BOOST_SCORE_MAX, SRX_BOOST_SCORE_MIN = 0, 1, 2, 3  # score_mode
SRX_BOOST_MULTIPLY, SRX_BOOST_SUM, SRX_BOOST_REPLACE = 0, 1, 2                                        # boost_mode
SRX_BOOST_ABS = 1                                                                                     # clause flags
SRX_BOOST_MAX_M, SRX_BOOST_MAX_CLAUSES, SRX_BOOST_MAX_COLS = 2048, 8, 8                               # pinned to the header by tests/test_boost_cpu.py
SRX_BOOST_MAX_KNOTS = 1 << 24


class LtrFeature(ctypes.Structure):
    """``srx_ltr_feature`` (include/ltr/sparse_rx_ltr.h): a HOST array element of 8 bytes"""
    _fields_ = [("kind", ctypes.c_int32), ("index", ctypes.c_int32)]


class LtrNode(ctypes.Structure):
    """``srx_ltr_node`` (include/ltr/sparse_rx_ltr.h): a DEVICE array element of 16 bytes"""
    _fields_ = [("feature", ctypes.c_int32), ("value", ctypes.c_float), ("left", ctypes.c_int32), ("right", ctypes.c_int32)]


# every symbol include/ltr/sparse_rx_ltr.h declares (the fifteenth header of the same library)
_LTR_HEAD = [_I32, _CP, _I32, _I64, _I64, ctypes.POINTER(LtrFeature), _I32, _VP, _I32, _VP, _I32, _VP, _I32, _F32, _I32, _I32, _VP, _VP, _VP]  # device .. cand_count
LTR_SYMBOLS = {
    "srx_ltr_topk": (ctypes.c_int, [*_LTR_HEAD, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
    "srx_ltr_score": (ctypes.c_int, [*_LTR_HEAD, _I32, _I32, _VP, _VP]),
}
SRX_LTR_F_SCORE, SRX_LTR_F_RANK, SRX_LTR_F_COLUMN, SRX_LTR_F_EXTRA = 0, 1, 2, 3                       # srx_ltr_feature.kind
SRX_LTR_LE, SRX_LTR_LT = 0, 1                                                                         # cmp
SRX_LTR_REPLACE, SRX_LTR_SUM = 0, 1                                                                   # mode
SRX_LTR_MISSING_LEFT = 1 << 30                                                                        # bit 30 of srx_ltr_node.feature
SRX_LTR_MAX_M, SRX_LTR_MAX_COLS, SRX_LTR_MAX_FEATURES, SRX_LTR_MAX_EXTRA = 2048, 8, 32, 32            # pinned to the header by tests/test_ltr_cpu.py
SRX_LTR_MAX_TREES, SRX_LTR_MAX_NODES = 4096, 1 << 22

# every symbol include/eval/sparse_rx_eval.h declares (the sixteenth header of the same library)
EVAL_SYMBOLS = {
    "srx_eval_workspace_bytes": (_I64, [_I32, _I32]),
    "srx_eval_lists": (ctypes.c_int, [_I32, _VP, _VP, _VP, _VP, _I32, _I64, _VP, _I32, _VP, _I32, _VP, _VP, _VP, _I32, _I32, ctypes.POINTER(_I32), _I32,
                                      _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
}
SRX_EVAL_NDCG, SRX_EVAL_AP, SRX_EVAL_RECALL, SRX_EVAL_P, SRX_EVAL_RR, SRX_EVAL_SUCCESS, SRX_EVAL_DCG, SRX_EVAL_IDCG = range(8)  # the last axis of out
SRX_EVAL_METRICS, SRX_EVAL_MAX_M, SRX_EVAL_MAX_K, SRX_EVAL_MAX_GAIN = 8, 2048, 8, 32                  # pinned to the header by tests/test_eval_cpu.py
SRX_EVAL_WAVE_M, SRX_EVAL_LDS_ROW, SRX_EVAL_MEAN_CHUNK = 256, 1024, 1024                              # the kernel's size constants, and the means' chunk

# every symbol include/binary/sparse_rx_binary.h declares (the seventeenth header of the same library)
BINARY_SYMBOLS = {
    "srx_binary_bytes": (_I64, [_I64, _I32, _I32]),
    "srx_binary_encode": (ctypes.c_int, [_I32, _VP, _I64, _I64, _I32, _I32, _I64, _I64, _VP, _I32, _VP, _VP]),
    "srx_binary_workspace_bytes": (_I64, [_I32, _I64, _I32]),
    "srx_binary_search": (ctypes.c_int, [_I32, _VP, _I64, _I32, _VP, _I32, _I32, _I64, _FP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "srx_binary_dist_docs": (ctypes.c_int, [_I32, _VP, _I64, _I32, _VP, _I32, _I64, _VP, _VP, _I32, _VP, _VP]),
}
SRX_BINARY_TILE, SRX_BINARY_QTILE, SRX_BINARY_PASS = 64, 128, 1024                                    # rows per tile, queries per wave walk and per pass
SRX_BINARY_RANK_CHUNK, SRX_BINARY_SPLIT_DOCS, SRX_BINARY_BLOCK_DOCS = 4096, 16384, 256                # the rank kernel's step, docs per row split, docs per workgroup


def order_plan(n_docs: int, n_rows: int, k: int):
    """``(segments, workspace bytes)`` of ``srx_order_topk``: the formula of include/order/sparse_rx_order.h restated (pinned to
    ``srx_order_workspace_bytes`` by tests/test_order_cpu.py).  A segment is what one workgroup scans for one row."""
    seg_docs = -(-max(SRX_ORDER_MIN_SEG, 64 * int(k)) // SRX_ORDER_CHUNK) * SRX_ORDER_CHUNK
    segments = -(-int(n_docs) // seg_docs)
    return segments, int(n_rows) * segments * (12 * int(k) + 8)

_lib: Optional[ctypes.CDLL] = None


def kernel_sources_sha256() -> str:
    """sha256 over the sources of the kernels a sparse search launches (wave_kernel.hip, tier2_kernel.hip, merge.hip and
    srx_common.h): identifies the build a profile was taken from.  The driver (sparse_rx.hip) and the index build
    (build.hip) are not part of it: an edit there does not change what a search runs on the GPU."""
    import hashlib
    h = hashlib.sha256()
    for f in ["wave_kernel.hip", "tier2_kernel.hip", "merge.hip", "srx_common.h"]:
        with open(os.path.join(CSRC_DIR, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _deps():
    return [os.path.join(CSRC_DIR, f) for f in SOURCES] + [os.path.join(CSRC_DIR, "srx_common.h"), os.path.join(CSRC_DIR, "filter_common.h"),
                                                            os.path.join(CSRC_DIR, "desc_check.h"),
                                                            os.path.join(CSRC_DIR, "field_common.h"),
                                                            os.path.join(CSRC_DIR, "half_common.h"),
                                                            os.path.join(CSRC_DIR, "mmr_common.h"),
                                                            os.path.join(INCLUDE_DIR, "sparse_rx.h"),
                                                            os.path.join(INCLUDE_DIR, "sparse_rx_rescore.h"),
                                                            os.path.join(INCLUDE_DIR, "sparse_rx_quant.h"),
                                                            os.path.join(INCLUDE_DIR, "sparse_rx_filter.h"),
                                                            os.path.join(INCLUDE_DIR, "sparse_rx_half.h"),
                                                            os.path.join(INCLUDE_DIR, "sparse_rx_mmr.h"),
                                                            os.path.join(INCLUDE_DIR, "sparse_rx_terms.h"),
                                                            os.path.join(INCLUDE_DIR, "sparse_rx_maxsim.h"),
                                                            os.path.join(INCLUDE_DIR, "sparse_rx_fields.h"),
                                                            os.path.join(INCLUDE_DIR, "sparse_rx_collapse.h"),
                                                            os.path.join(INCLUDE_DIR, "sparse_rx_facets.h"),
                                                            os.path.join(INCLUDE_DIR, "ext", "sparse_rx_feedback.h"),
                                                            os.path.join(INCLUDE_DIR, "order", "sparse_rx_order.h"),
                                                            os.path.join(INCLUDE_DIR, "boost", "sparse_rx_boost.h"),
                                                            os.path.join(INCLUDE_DIR, "ltr", "sparse_rx_ltr.h"),
                                                            os.path.join(INCLUDE_DIR, "eval", "sparse_rx_eval.h"),
                                                            os.path.join(INCLUDE_DIR, "binary", "sparse_rx_binary.h")]


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 with hipcc (one object per source, in parallel) and link them into
    <package>/libsparse_rx.so (in-tree)."""
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(p) for p in _deps()):
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise SparseRxUnavailable("hipcc not found: cannot build libsparse_rx.so")
    objdir = os.path.join(CSRC_DIR, "build")
    os.makedirs(objdir, exist_ok=True)
    newest_hdr = max(os.path.getmtime(p) for p in _deps()[len(SOURCES):])
    procs, objs = [], []
    for f in SOURCES:
        src, obj = os.path.join(CSRC_DIR, f), os.path.join(objdir, f.replace(".hip", ".o"))
        objs.append(obj)
        newest_src = max(os.path.getmtime(os.path.join(CSRC_DIR, x)) for x in [f, *INCLUDED_SOURCES.get(f, [])])
        if not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(newest_src, newest_hdr):
            continue
        cmd = [hipcc, *HIPCC_FLAGS, f"-I{INCLUDE_DIR}", f"-I{CSRC_DIR}", "-c", "-o", obj, src]
        if verbose:
            print(" ".join(cmd))
        procs.append((f, subprocess.Popen(cmd)))
    for f, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, f"hipcc -c {f}")
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-fvisibility=hidden", "-o", LIB_PATH, *objs]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """The loaded library (symbols typed).  Raises SparseRxUnavailable if it was never built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SparseRxUnavailable(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise SparseRxUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in {**SYMBOLS, **RESCORE_SYMBOLS, **QUANT_SYMBOLS, **FILTER_SYMBOLS, **HALF_SYMBOLS, **MMR_SYMBOLS,
                                   **TERMS_SYMBOLS, **MAXSIM_SYMBOLS, **FIELDS_SYMBOLS, **COLLAPSE_SYMBOLS, **FACET_SYMBOLS, **FEEDBACK_SYMBOLS,
                                   **ORDER_SYMBOLS, **BOOST_SYMBOLS, **LTR_SYMBOLS, **EVAL_SYMBOLS, **BINARY_SYMBOLS}.items():
        try:
            f = getattr(L, name)
        except AttributeError as e:
            raise SparseRxUnavailable(f"{LIB_PATH} does not export {name}") from e
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def check(rc: int, what: str) -> int:
    if rc < 0:
        msg = lib().srx_last_error()
        text = msg.decode("utf-8", "replace") if msg else ""
        if rc == -1:
            raise ValueError(f"{what}: {text}")
        raise SparseRxError(f"{what} failed ({rc}): {text}")
    return rc


def limits():
    out = (ctypes.c_int32 * 4)()
    check(lib().srx_limits(out), "srx_limits")
    return {"max_k": out[0], "max_tile_log2": out[1], "hash_cap": out[2], "threads": out[3]}
