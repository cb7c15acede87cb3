"""sparse-rx: MI355X-native batched BM25 / learned-sparse scoring + top-k behind the reference's
``RetrievalService.build_bm25_index()`` / ``search_bm25()`` API.  Import as ``sparse_rx``."""
from . import _capi
from ._capi import SparseRxError, SparseRxUnavailable, build_library
from .index import DeviceIndex, HostBatchPipeline, HostIndex, build_host_index, encode_queries, fuse_scored_device, fuse_topk_device, merge_topk_device, mmr_pool_depth, parse_operators, tokenize, validate_candidates
from .service import RetrievalService
from .registry import HybridRetriever, OptimizedBM25Retriever, OptimizedRetriever, QuantizedEmbeddingRetriever, RetrieverRegistry, load_index_npz, save_index_npz
from .dense import (DenseF32Index, DenseHalfIndex, DenseInt8Index, DenseUint8Index, QuantizedEmbeddingIndex, check_mmr_args, quantize_asymmetric,
                    quantize_asymmetric_device, quantize_queries_asymmetric_device, quantize_queries_symmetric_device,
                    quantize_query_asymmetric, quantize_query_symmetric, quantize_symmetric, quantize_symmetric_device)
from .distributed import (ShardedSearcher, shard_range, global_df, global_avgdl, global_term_bounds, bm25_idf_from_df,
                          build_sharded_host_index)
from .backend import SparseBackend, collapse_deep, collapse_pool_depth
from .filter import DocFilter
from .late import TokenIndex, check_late_shape, late_pool_depth
from .fields import FieldTable, columns_from_metadata
from .feedback import ForwardIndex
from . import boost
from .boost import BoostFn, BoostResolver, boost_deep
from . import ltr
from .ltr import ForestModel, RankFn
from . import evaluate
from .evaluate import Judgments
from . import binary
from .binary import DenseBinaryIndex, ScreenedDenseIndex

__all__ = ["RetrievalService", "DeviceIndex", "HostBatchPipeline", "HostIndex", "build_host_index", "encode_queries", "merge_topk_device", "fuse_topk_device", "fuse_scored_device", "validate_candidates", "HybridRetriever",
           "tokenize", "build_library", "SparseRxError", "SparseRxUnavailable", "_capi", "ShardedSearcher", "shard_range",
           "global_df", "global_avgdl", "global_term_bounds", "bm25_idf_from_df", "build_sharded_host_index", "SparseBackend", "DocFilter", "OptimizedBM25Retriever", "OptimizedRetriever", "QuantizedEmbeddingRetriever", "RetrieverRegistry",
           "load_index_npz", "save_index_npz", "DenseF32Index", "DenseHalfIndex", "DenseInt8Index", "DenseUint8Index", "QuantizedEmbeddingIndex", "quantize_symmetric",
           "quantize_asymmetric", "quantize_query_asymmetric",
           "quantize_query_symmetric", "quantize_symmetric_device", "quantize_asymmetric_device", "quantize_queries_symmetric_device",
           "quantize_queries_asymmetric_device", "check_mmr_args", "mmr_pool_depth", "parse_operators", "TokenIndex", "check_late_shape",
           "late_pool_depth", "FieldTable", "columns_from_metadata", "collapse_deep", "collapse_pool_depth", "ForwardIndex",
           "boost", "BoostFn", "BoostResolver", "boost_deep", "ltr", "ForestModel", "RankFn", "evaluate", "Judgments",
           "binary", "DenseBinaryIndex", "ScreenedDenseIndex"]
