"""Registry / pipeline adapters and the .npz index cache (row f2).

Mirrors, on the HIP engine, the two other call sites of the reference's hot path:
  * ``OptimizedBM25Retriever`` + ``RetrieverRegistry``  -- /root/reference/rag_system/core/retriever_registry.py:120-356, 562-599
  * ``OptimizedRetriever``                              -- /root/reference/rag_system/pipeline/evaluate_rag_pipeline.py:162-479
    (``bm25*`` types score with ``simd_bm25_score``, every other type with ``simd_tfidf_score`` and
    idf = log(N/(df+1)), :257-278, :378-399; index cache ``.rag_cache/{method}_index_{hash}.npz``, :189-200, :280-312)
so that the YAML experiments and ``benchmark_efficiency`` (objects with ``build_index_from_corpus`` + ``search``) run
unmodified.  The registry's dense types (dpr / contriever / splade) go to the ``QuantizedEmbeddingRetriever`` mirror, and
the ``hybrid`` type the reference configures without implementing it to ``HybridRetriever`` (sparse + dense, fused on the GPU).

``top_k``: any value, like the reference (deep rankings are paged with ``srx_search_after``); ``top_k <= 0`` gives ``{}``.
"""
from __future__ import annotations

import hashlib
import threading
import time
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from .backend import SparseBackend, SparseIndexViews
from .index import HostIndex, check_fuse_args, check_rescore_args, encode_queries, hybrid_depths, hybrid_search, rows_to_dict

_BM25_TYPES = ("bm25", "bm25_retriever", "bm25_custom")


class _SparseRetrieverBase(SparseIndexViews):
    """Shared batched search: cache semantics of the reference call sites, one srx_search per call."""

    # mode, term_order, strip_cache_key, blank, the body of search and the doors that only hand on to the backend: backend.SparseIndexViews

    def __init__(self, k1: float, b: float, device: Optional[str], tile_log2: int, use_cache: bool = True, group=None,
                 shard_searcher_factory=None, sharded: Optional[bool] = None, one_copy: bool = True):
        self.k1, self.b = k1, b
        # one GPU, or -- inside an initialised torch.distributed group -- doc-range shards (backend.SparseBackend)
        self._be = SparseBackend(device, tile_log2, group=group, searcher_factory=shard_searcher_factory, sharded=sharded, one_copy=one_copy)
        self.device, self.tile_log2 = self._be.device, tile_log2
        self.query_cache: Optional[Dict[str, Tuple[np.ndarray, np.ndarray]]] = {} if use_cache else None
        self.cache_lock = threading.RLock()

    def _upload(self):
        self._be.upload(self.mode, self.k1, self.b)

    def search(self, queries: Dict[str, str], top_k: int = 10, *, allowed_docs=None, excluded_docs=None, must_terms=None, any_terms=None,
               must_not_terms=None, operators: bool = False, where=None, collapse_by: Optional[str] = None, per_group: int = 1,
               collapse_nulls: str = "own", collapse_depth: Optional[int] = None, expand_docs: Optional[int] = None, expand_terms: int = 10,
               expand_weight: float = 0.5, expand_by: str = "score", boost=None, boost_depth: Optional[int] = None, rank_model: bool = False,
               rank_pool: Optional[int] = None) -> Dict[str, Dict[str, float]]:
        """``allowed_docs`` / ``excluded_docs`` (no reference counterpart): as ``RetrievalService.search_bm25`` -- the top
        ``top_k`` of the allowed docs, exact; both given or an unknown doc id raise ValueError; no cache for a filtered call.
        ``must_terms`` / ``any_terms`` / ``must_not_terms`` / ``operators``: term constraints, as ``RetrievalService.search_bm25``
        (rows built on the GPU from the posting lists, n_docs / 8 bytes per distinct constraint; scores unchanged; no cache).
        ``where``: a field predicate over the columns of :meth:`set_doc_fields`, as ``RetrievalService.search_bm25``.
        ``collapse_by`` / ``per_group`` / ``collapse_nulls`` / ``collapse_depth``: the top ``top_k`` of the ranking collapsed by a
        column of :meth:`set_doc_fields`, exact, as ``RetrievalService.search_bm25`` (``top_k`` <= 1024; no cache).
        ``expand_docs`` / ``expand_terms`` / ``expand_weight`` / ``expand_by``: pseudo-relevance feedback as
        ``RetrievalService.search_bm25`` (needs :meth:`enable_feedback`; no cache): the search of the query expanded on the GPU from
        its own first ``expand_docs`` results.  In dot mode a contribution is the doc's raw value and every term's gain is 1
        (Rocchio-style); in BM25 mode tf / doc_len and max(idf, 0).  The scores are those of the expanded query, whose weights
        sum to at most 1: not comparable to the scores of a plain search.
        ``boost`` / ``boost_depth``: the top ``top_k`` of the ranking boosted by field values, exact, with the boosted scores, as
        ``RetrievalService.search_bm25`` (needs raw scores > 0, which the search guarantees; not with ``collapse_by``; no cache).
        ``rank_model`` / ``rank_pool``: the first ``rank_pool`` rows of this search re-scored by the model of :meth:`set_rank_model`
        and cut to ``top_k``, as ``RetrievalService.search_bm25`` (pool-relative; not with ``boost``)."""
        # blank = no text (retriever_registry.py:237-239): white space is searched as an empty row; the cache is optional
        return self._search(queries, top_k, (allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, operators, where),
                            (collapse_by, per_group, collapse_nulls, collapse_depth), (expand_docs, expand_terms, expand_weight, expand_by),
                            boost, boost_depth, rank_model, rank_pool)

    def score(self, queries: Dict[str, str], candidates: Dict[str, Any]) -> Dict[str, Dict[str, float]]:
        """The exact score of caller-named documents: ``{qid: {doc_id: score}}`` with every doc of ``candidates[qid]`` in
        the caller's order and the arithmetic of :meth:`search` (``srx_score_docs``; the accumulation order is this
        retriever's ``term_order``).  No ``score > 0`` filter: 0.0 where no query term matches and for a blank or
        all-OOV query; ``{}`` for a qid without candidates; ``ValueError`` for an unknown doc id.  One batch, no cache."""
        self._need_index()
        return self._be.score_dicts(queries, candidates, order=self.term_order)

    def close(self):
        self._be.close()


class OptimizedBM25Retriever(_SparseRetrieverBase):
    """retriever_registry.py:120-356 (``method='tfidf'`` is BM25 with k1=1000, b=0 there, :593-595)."""

    def __init__(self, method: str = "bm25", model: str = None, k1: float = 1.2, b: float = 0.75, device: Optional[str] = None,
                 tile_log2: int = 14, **kwargs):
        super().__init__(k1, b, device, tile_log2, use_cache=kwargs.get("cache_queries", True), group=kwargs.get("group"),
                         shard_searcher_factory=kwargs.get("shard_searcher_factory"), sharded=kwargs.get("sharded"),
                         one_copy=kwargs.get("one_copy", True))
        self.method = method.lower()
        self.model_name = model
        self.use_simd = kwargs.get("use_simd", True)  # accepted, meaningless here

    def build_index_from_corpus(self, corpus: Dict[str, Dict]) -> None:
        if not corpus:
            raise ValueError("Empty corpus provided")  # retriever_registry.py:155-156
        self._be.build(corpus, idf_kind="bm25")
        self._upload()


class OptimizedRetriever(_SparseRetrieverBase):
    """evaluate_rag_pipeline.py:162-479: config dict + hardware dict; non-BM25 types use the tf-idf dot product.

    ``accumulation``: the order in which a doc's per-term contributions are added.  The reference has two answers:
    its NumPy fallback ``_numpy_score_documents`` (:436-479, what runs wherever numba is absent -- and what the committed
    fixtures tests/golden/pipeline_small.* were produced with) walks ``relevant_terms`` in QUERY-TOKEN order; its Numba
    kernels (:57-121) walk the CSR row, i.e. ascending term id.  The two differ in the last fp32 bit on about a quarter
    of the fixture queries.  Default ``"token"`` reproduces the runnable reference bit for bit; ``"term"`` gives the
    Numba / ``RetrievalService`` order."""

    strip_cache_key = False  # its cache key is f"{query_text}:{top_k}" (:340)

    def __init__(self, config: Dict[str, Any], hardware_info: Optional[Dict[str, Any]] = None, device: Optional[str] = None,
                 tile_log2: int = 14, cache_dir: str = ".rag_cache", accumulation: str = "token", group=None,
                 shard_searcher_factory=None, sharded: Optional[bool] = None, one_copy: bool = True):
        if accumulation not in ("token", "term"):
            raise ValueError("accumulation must be 'token' or 'term'")
        self.term_order = accumulation
        params = config.get("params", {}) or {}
        hardware_info = hardware_info or {"memory_gb": 8, "cores": 4}
        super().__init__(params.get("k1", 1.2), params.get("b", 0.75), device, tile_log2,
                         use_cache=hardware_info.get("memory_gb", 8) > 4, group=group, shard_searcher_factory=shard_searcher_factory,
                         sharded=sharded, one_copy=one_copy)
        self.config, self.hardware = config, hardware_info
        self.method = config.get("type", "bm25").lower()
        self.mode = "bm25" if self.method in ("bm25", "bm25_custom") else "dot"  # :258-261, :378-399
        self.use_cache = hardware_info.get("memory_gb", 8) > 4
        self.cache_dir = Path(cache_dir)

    def build_index_from_corpus(self, corpus: Dict[str, Dict]) -> None:
        corpus_hash = hashlib.md5(str(sorted(corpus.keys())[:1000]).encode()).hexdigest()[:8]  # :189
        cache_file = self.cache_dir / f"{self.method}_index_{corpus_hash}.npz"
        sharded = self._be.sharded()  # the .npz cache holds a whole-corpus index: shards are always built from the corpus
        if self.use_cache and cache_file.exists() and not sharded:
            self._be.set_host(load_index_npz(cache_file))
        else:
            self._be.build(corpus, idf_kind="bm25" if self.mode == "bm25" else "tfidf")
            if self.use_cache and not sharded:
                self.cache_dir.mkdir(exist_ok=True)
                save_index_npz(cache_file, self.host)
        self._upload()


def save_index_npz(path, h: HostIndex) -> None:
    """The reference's cache schema (evaluate_rag_pipeline.py:280-296): same keys and dtypes."""
    vocab_sorted = sorted(h.vocabulary, key=h.vocabulary.get)
    np.savez_compressed(path, tf_data=h.data, tf_indices=h.indices, tf_indptr=h.indptr,
                        tf_shape=np.array((h.n_docs, h.vocab_size), dtype=np.int64), doc_lengths=h.doc_lengths, idf=h.idf,
                        vocabulary=np.array(vocab_sorted), doc_ids=np.array(h.doc_ids), avgdl=np.float32(h.avgdl))


def load_index_npz(path) -> HostIndex:
    """Reads the schema above with ``allow_pickle=False`` (string arrays are plain ``<U`` arrays)."""
    z = np.load(path, allow_pickle=False)
    return HostIndex(indptr=z["tf_indptr"], indices=z["tf_indices"], data=z["tf_data"], doc_lengths=z["doc_lengths"],
                     idf=z["idf"], avgdl=float(z["avgdl"]), vocabulary={str(t): i for i, t in enumerate(z["vocabulary"])},
                     doc_ids=[str(d) for d in z["doc_ids"]])


class QuantizedEmbeddingRetriever:
    """Mirror of the reference's dense retriever (retriever_registry.py:358-559) on the HIP engine: the same simulated
    embeddings (clustered corpus vectors from ``np.random.seed(42)``, query vectors seeded by ``hash(query_text)``), the
    symmetric INT8 / asymmetric uint8 quantization and result dicts, with ``quantized_dot_product_batch`` + top-k replaced by
    ``srx_dense_search_i8`` (asymmetric: ``srx_dense_search_u8``; ``use_quantization=False``: ``np.dot`` + top-k replaced by
    ``srx_dense_search_f32``).  All
    queries of a ``search`` call go to the GPU as one batch."""

    def __init__(self, method: str, model: str, embedding_dim: int = 768, device: str = "cuda:0", **kwargs):
        self.method = method.lower()
        self.model_name = model
        self.embedding_dim = embedding_dim
        self.use_quantization = kwargs.get("use_quantization", True)
        self.quantization_method = kwargs.get("quantization_method", "symmetric")
        self.device = device
        from .dense import check_quantize_arg
        # "host": the NumPy quantisers (the reference's path); "device": the corpus and every query batch are quantised in
        # HIP (include/sparse_rx_quant.h) -- the same codes and scales bit for bit, no per-query host loop
        self.quantize = check_quantize_arg(kwargs.get("quantize", "host"))
        self.corpus_embeddings_int8 = None
        self.corpus_scales = None
        self.corpus_embeddings_fp32: Optional[np.ndarray] = None
        self.doc_ids: List[str] = []
        self._index = None

    # The reference keeps the quantised corpus as host arrays (:389-392).  With quantize="device" they exist on the device only
    # and are copied back on first access.
    @property
    def corpus_embeddings_int8(self) -> Optional[np.ndarray]:
        self._fetch_corpus()
        return self._corpus_codes

    @corpus_embeddings_int8.setter
    def corpus_embeddings_int8(self, value) -> None:
        self._corpus_codes = value

    @property
    def corpus_scales(self) -> Optional[np.ndarray]:
        self._fetch_corpus()
        return self._corpus_scales

    @corpus_scales.setter
    def corpus_scales(self, value) -> None:
        self._corpus_scales = value

    def _fetch_corpus(self) -> None:
        if getattr(self, "_corpus_codes", None) is None and self.quantize == "device" and self.use_quantization and self._index is not None:
            self._corpus_codes, self._corpus_scales = self._index.corpus_to_host()

    def _build_quantized(self, emb) -> None:
        """The quantised index of ``emb`` by the scheme and the ``quantize`` route this retriever is set to."""
        from .dense import DenseInt8Index, DenseUint8Index, quantize_asymmetric, quantize_symmetric
        symmetric = self.quantization_method == "symmetric"  # any other value is the asymmetric scheme, like the reference's else branch (:449)
        cls = DenseInt8Index if symmetric else DenseUint8Index
        if self.quantize == "device":
            self.corpus_embeddings_int8 = self.corpus_scales = None
            self._index = None
            self._index = cls.from_embeddings(emb, device=self.device)
        else:
            self.corpus_embeddings_int8, self.corpus_scales = (quantize_symmetric if symmetric else quantize_asymmetric)(emb)
            self._index = cls(self.corpus_embeddings_int8, self.corpus_scales, device=self.device)

    def _search_quantized(self, embs, k):
        """Host (doc, score, count) of the quantised search for a list of f32 query vectors."""
        from .dense import quantize_query_asymmetric, quantize_query_symmetric, stack_queries_f32
        symmetric = self.quantization_method == "symmetric"
        if self.quantize == "device":
            q = stack_queries_f32(self._index, embs)
            return self._index._host(self._index.search_f32_device(q, k) if symmetric else self._index.search_raw_device(q, k))
        if symmetric:
            qq = [quantize_query_symmetric(e) for e in embs]
            return self._index.search(np.stack([a for a, _ in qq]), np.array([b for _, b in qq], dtype=np.float32), k)
        qq = [quantize_query_asymmetric(e) for e in embs]
        return self._index.search(np.stack([a for a, _ in qq]), np.stack([b for _, b in qq]), k)

    def _score_quantized(self, embs, cand_doc, cand_count):
        """Host f32[nq, m] scores of the candidate block for a list of f32 query vectors."""
        from .dense import quantize_query_asymmetric, quantize_query_symmetric, stack_queries_f32
        symmetric = self.quantization_method == "symmetric"
        ix = self._index
        if self.quantize == "device":
            q = stack_queries_f32(ix, embs)
            fn = ix.score_docs_f32_device if symmetric else ix.score_docs_raw_device
            return ix._score_docs(cand_doc, cand_count, len(embs), lambda cd, cc: fn(q, cd, cc))
        if symmetric:
            qq = [quantize_query_symmetric(e) for e in embs]
            return ix.score_docs(np.stack([a for a, _ in qq]), np.array([b for _, b in qq], dtype=np.float32), cand_doc, cand_count)
        qq = [quantize_query_asymmetric(e) for e in embs]
        return ix.score_docs(np.stack([a for a, _ in qq]), np.stack([b for _, b in qq]), cand_doc, cand_count)

    def synthetic_embeddings(self, num_docs: int) -> np.ndarray:
        """retriever_registry.py:409-433: cluster centres + 0.1 noise from the legacy NumPy stream seeded with 42, rows
        normalised; drawn in the reference's order (centres, assignments, then one noise row per document)."""
        np.random.seed(42)
        num_clusters = min(50, num_docs // 10)
        centers = np.random.randn(num_clusters, self.embedding_dim).astype(np.float32)
        assign = np.random.randint(0, num_clusters, num_docs)
        noise = np.random.randn(num_docs, self.embedding_dim) * 0.1       # row i = the i-th randn(dim) call of the reference
        emb = (centers[assign] + noise).astype(np.float32)                 # f32 + f64 -> f64, stored as f32 (:426)
        norms = np.linalg.norm(emb, axis=1, keepdims=True)
        return emb / np.maximum(norms, 1e-8)

    def query_embedding_from_seed(self, seed: int) -> np.ndarray:
        """retriever_registry.py:526-536 after the hash: randn(dim) from the legacy stream, as f32, normalised."""
        np.random.seed(seed)
        e = np.random.randn(self.embedding_dim).astype(np.float32)
        return e / np.linalg.norm(e)

    def _generate_query_embedding(self, query_text: str) -> np.ndarray:
        return self.query_embedding_from_seed(hash(query_text) % (2 ** 31))  # process-dependent, like the reference's

    def build_index_from_corpus(self, corpus: Dict[str, Dict]) -> None:
        from .dense import DenseF32Index
        self.doc_ids = list(corpus.keys())
        emb = self.synthetic_embeddings(len(corpus))
        if self.use_quantization:
            self._build_quantized(emb)
        else:
            self.corpus_embeddings_fp32 = emb
            self._index = DenseF32Index(emb, device=self.device)

    def search(self, queries: Dict[str, str], top_k: int = 10) -> Dict[str, Dict[str, float]]:
        if self._index is None:
            raise ValueError("Index not built. Call build_index_from_corpus() first.")
        results: Dict[str, Dict[str, float]] = {qid: {} for qid in queries}
        live = [(qid, text) for qid, text in queries.items() if text]
        if not live:
            return results
        embs = [self._generate_query_embedding(text) for _, text in live]
        k = max(1, min(int(top_k), len(self.doc_ids)))
        if self.use_quantization:
            d, s, n = self._search_quantized(embs, k)
        else:
            d, s, n = self._index.search(np.stack(embs), k)
        for i, (qid, _) in enumerate(live):
            results[qid] = rows_to_dict(self.doc_ids, d, s, n, i)  # score > 0 only (:515-519)
        return results

    def score(self, query_embeddings: Dict[str, np.ndarray], candidates: Dict[str, Any]) -> Dict[str, Dict[str, float]]:
        """The score of caller-named documents for caller-given query embeddings ``{qid: f32[embedding_dim]}``:
        ``{qid: {doc_id: score}}`` with every doc of ``candidates[qid]`` in the caller's order, quantized and scored with
        the arithmetic of :meth:`search` (``srx_dense_score_docs_i8`` / ``_u8`` / ``_f32``).  No ``score > 0`` filter;
        ``{}`` for a qid without candidates; ``ValueError`` for an unknown doc id.  One batch, no cache."""
        from .backend import RowOfIds, scores_to_dicts
        if self._index is None:
            raise ValueError("Index not built. Call build_index_from_corpus() first.")
        if getattr(self, "_rows", None) is None or self._rows.ids is not self.doc_ids:
            self._rows = RowOfIds(self.doc_ids)  # kept between calls, like the sparse side's
        results, live, cand_doc, cand_count = self._rows.candidate_block(query_embeddings, candidates)
        if not live:
            return results
        embs = [np.asarray(e, dtype=np.float32) for _, e, _ in live]
        if self.use_quantization:
            scores = self._score_quantized(embs, cand_doc, cand_count)
        else:
            scores = self._index.score_docs(np.stack(embs), cand_doc, cand_count)
        return scores_to_dicts(results, live, scores)


class HybridRetriever:
    """The ``hybrid`` retriever type the reference configures (configs/ms_marco_paper_results.yaml:108-120: ``model:
    {sparse, dense}``, ``params: {sparse_weight: 0.3, dense_weight: 0.7, ...}``) but does not implement
    (retriever_registry.py:596-599 rejects it).  Composes the two mirrors above over one corpus dict -- row i is the same
    document on both sides -- and fuses their top lists on the GPU (``srx_fuse_topk``, include/sparse_rx.h).

    ``fusion``: "weighted" (each side's scores divided by its best score, then the weighted sum) or "rrf" (weighted
    reciprocal rank fusion with constant ``rrf_c``).  ``candidates``: rows fetched from each side (default ``top_k``; each
    side is capped at ``min(candidates, n_docs, 1024)``).  A doc only one side retrieved scores with that side alone,
    unless ``rescore=True`` ("weighted" only; ``ValueError`` with "rrf"; also read from the registry block's ``params``):
    then each list is completed with the other side's exact score of its docs before the fusion (``srx_score_docs``,
    ``srx_dense_score_docs_i8``, ``srx_fuse_topk_scored``; include/sparse_rx_rescore.h) and the fused score of a returned
    doc no longer depends on ``candidates``.
    With one weight 0 the result is the other side's SET, but equal normalised scores rank by doc id, so the order can
    differ from that side's own.  ``top_k`` > 1024 raises ``ValueError``: fused rankings deeper than the engine's lists
    are not paged, and a silently shorter list would be worse than an error.  The dense side is the symmetric INT8 engine
    whatever the embeddings' origin.  Needs the whole index on one GPU."""

    def __init__(self, model=None, sparse_weight: float = 0.3, dense_weight: float = 0.7, fusion: str = "weighted",
                 rrf_c: float = 60.0, candidates: Optional[int] = None, embedding_dim: int = 768, device: Optional[str] = None,
                 k1: float = 1.2, b: float = 0.75, tile_log2: int = 14, rescore: bool = False, quantize: str = "host", **kwargs):
        model = model or {}
        if not isinstance(model, dict):
            raise ValueError("hybrid retriever: model must be a dict {sparse: ..., dense: ...}")
        fusion = str(fusion).lower()
        check_fuse_args(fusion, (sparse_weight, dense_weight), rrf_c)
        self.rescore = check_rescore_args(fusion, rescore)
        if candidates is not None and int(candidates) < 1:
            raise ValueError(f"candidates must be >= 1, got {candidates}")
        self.method = "hybrid"
        self.sparse_weight, self.dense_weight = float(sparse_weight), float(dense_weight)
        self.fusion, self.rrf_c, self.candidates = fusion, float(rrf_c), candidates
        # top_k, use_numba, cache_matrices of the reference's config block are accepted and mean nothing here
        sparse, dense = str(model.get("sparse", "bm25")), str(model.get("dense", "dpr"))
        group = {key: kwargs[key] for key in ("group", "sharded", "shard_searcher_factory") if key in kwargs}
        if sparse.lower() == "tfidf":
            self.sparse = OptimizedBM25Retriever(method="tfidf", model=sparse, k1=1000, b=0, device=device, tile_log2=tile_log2,
                                                 cache_queries=False, **group)
        else:  # a bm25 type name, or a model name for the default type
            self.sparse = OptimizedBM25Retriever(method=sparse if sparse.lower() in _BM25_TYPES else "bm25", model=sparse, k1=k1, b=b,
                                                 device=device, tile_log2=tile_log2, cache_queries=False, **group)
        self.dense = QuantizedEmbeddingRetriever(method=dense if dense.lower() in ("dpr", "contriever", "splade") else "dpr",
                                                 model=dense, embedding_dim=embedding_dim, device=self.sparse.device, quantize=quantize)
        self.device = self.sparse.device

    @property
    def doc_ids(self):
        return self.sparse.doc_ids

    def _refuse_sharded(self):
        if self.sparse._be.sharded():
            raise ValueError("hybrid search needs the whole index on one GPU (the dense corpus is not sharded)")

    def build_index_from_corpus(self, corpus: Dict[str, Dict], embeddings=None) -> None:
        """``embeddings``: f32[n_docs, dim], row i = the i-th corpus key; ``None`` = the dense mirror's simulated
        vectors (what the reference's dense types index).  Either way the rows are quantised into one INT8 index -- on the
        host, or with ``quantize="device"`` by ``DenseInt8Index.from_embeddings``."""
        self._refuse_sharded()
        if not corpus:
            raise ValueError("Empty corpus provided")
        if embeddings is not None:
            emb = np.asarray(embeddings, dtype=np.float32)
            if emb.ndim != 2 or emb.shape[0] != len(corpus):
                raise ValueError("embeddings must be [n_docs, dim] with one row per document")
        self.sparse.build_index_from_corpus(corpus)
        d = self.dense
        if embeddings is None:
            emb = d.synthetic_embeddings(len(corpus))
        d.embedding_dim = int(emb.shape[1])
        d.doc_ids = list(corpus.keys())
        d.use_quantization, d.quantization_method = True, "symmetric"
        d.device = self.device
        d._build_quantized(emb)

    def _live_query_vectors(self, queries, live, query_embeddings):
        """The f32 vectors of the ``live`` (qid, text) pairs: a list of host rows -- or, for a 2-D block with
        ``quantize="device"``, the block's live rows as they are (a device tensor stays on the device)."""
        d = self.dense
        if query_embeddings is None:
            return [d._generate_query_embedding(text) for _, text in live]
        if not isinstance(query_embeddings, dict):  # a 2-D block: row i belongs to the i-th key of ``queries``
            block = query_embeddings
            if tuple(block.shape) != (len(queries), d.embedding_dim):
                raise ValueError(f"query_embeddings has shape {tuple(block.shape)}, expected ({len(queries)}, {d.embedding_dim})")
            rows = [i for i, text in enumerate(queries.values()) if text]
            if d.quantize == "device":
                return block[rows]
            block = block.cpu().numpy() if hasattr(block, "cpu") else np.asarray(block)  # the host quantisers take NumPy rows
            return [np.asarray(block[i], dtype=np.float32) for i in rows]
        embs = []
        for qid, _ in live:
            if qid not in query_embeddings:
                raise ValueError(f"no query embedding for {qid!r}")
            e = np.asarray(query_embeddings[qid], dtype=np.float32)
            if e.shape != (d.embedding_dim,):
                raise ValueError(f"query embedding of {qid!r} has shape {e.shape}, expected ({d.embedding_dim},)")
            embs.append(e)
        return embs

    def search(self, queries: Dict[str, str], top_k: int = 10, query_embeddings=None, *, allowed_docs=None,
               excluded_docs=None) -> Dict[str, Dict[str, float]]:
        """``{qid: {doc_id: fused score}}`` in rank order.  ``allowed_docs`` / ``excluded_docs`` raise ``ValueError``: this
        retriever's dense side is the INT8 engine, whose search takes no doc filter (``RetrievalService.search_hybrid``
        filters both sides of an f32 hybrid).  ``query_embeddings``: ``{qid: f32[dim]}``, or a 2-D tensor /
        array whose row i belongs to the i-th key of ``queries`` (a float32 device tensor stays on the device with
        ``quantize="device"``); ``None`` = the dense mirror's simulated query vectors (seeded by ``hash(text)``: they differ
        between processes, like the reference's)."""
        from .dense import quantize_queries_symmetric_device, quantize_query_symmetric, stack_queries_f32
        if allowed_docs is not None or excluded_docs is not None:
            raise ValueError("HybridRetriever takes no doc filter: its dense side is the INT8 engine, whose screen thresholds come "
                             "from a sample of all docs (use RetrievalService.search_hybrid)")
        self._refuse_sharded()
        rescore = check_rescore_args(self.fusion, self.rescore)  # both are plain attributes
        if self.sparse.host is None or self.dense._index is None:
            raise ValueError("Index not built. Call build_index_from_corpus() first.")
        results: Dict[str, Dict[str, float]] = {qid: {} for qid in queries}
        n_docs = len(self.doc_ids)
        k, cand = hybrid_depths(top_k, self.candidates, n_docs)
        live = [(qid, text) for qid, text in queries.items() if text]
        if k <= 0 or not live:
            return results
        import torch
        vecs = self._live_query_vectors(queries, live, query_embeddings)
        if self.dense.quantize == "device":  # one stack, one upload (none for a device tensor), one quantisation launch
            q_dev = quantize_queries_symmetric_device(stack_queries_f32(self.dense._index, vecs))[:2]
        else:
            qq = [quantize_query_symmetric(e) for e in vecs]
            q_i8, q_scale = np.stack([a for a, _ in qq]), np.array([s for _, s in qq], dtype=np.float32)
            q_dev = (torch.as_tensor(np.ascontiguousarray(q_i8, dtype=np.int8), device=self.device), torch.as_tensor(q_scale, device=self.device))
        q_ptr, q_term, q_w = encode_queries([text for _, text in live], self.sparse.host.vocabulary)

        def dense_search(kb):
            return self.dense._index.search_device(*q_dev, kb)

        def dense_score(cand_doc, cand_count):
            return self.dense._index.score_docs_device(*q_dev, cand_doc, cand_count)

        doc, score, count = hybrid_search(self.sparse.dev, q_ptr, q_term, q_w, dense_search, cand, cand, k, self.fusion,
                                          (self.sparse_weight, self.dense_weight), self.rrf_c, rescore, dense_score)
        for i, (qid, _) in enumerate(live):
            results[qid] = rows_to_dict(self.doc_ids, doc, score, count, i)
        return results

    def close(self):
        self.sparse.close()
        self.dense._index = None


class RetrieverRegistry:
    """retriever_registry.py:562-599."""

    _retrievers: Dict[str, Any] = {}

    @classmethod
    def register(cls, name: str, retriever_class) -> None:
        cls._retrievers[name] = retriever_class

    @classmethod
    def create(cls, config):
        if isinstance(config, str):
            method, model, params = config, None, {}
        else:
            method = config.get("type", config.get("name"))
            model = config.get("model")
            params = config.get("params", {}) or {}
        if not method:
            raise ValueError("Retriever name/type not specified")
        m = method.lower()
        if m in _BM25_TYPES:
            return OptimizedBM25Retriever(method=method, model=model, **params)
        if m == "tfidf":
            return OptimizedBM25Retriever(method="tfidf", model=model, k1=1000, b=0, **params)  # :593-595
        if m in ("dpr", "contriever", "splade"):  # :588-592
            p2 = dict(params)
            embedding_dim = p2.pop("embedding_dim", 768)
            return QuantizedEmbeddingRetriever(method=method, model=model or f"quantized_{method}", embedding_dim=embedding_dim, **p2)
        if m == "hybrid":  # configured by the reference, implemented here only (HybridRetriever)
            return HybridRetriever(model=model, **params)
        if method in cls._retrievers:
            return cls._retrievers[method](**params)
        raise ValueError(f"Unknown retriever method: {method}")

    @classmethod
    def list_available(cls):
        return {"optimized_sparse": ["bm25", "bm25_custom", "tfidf"], "quantized_dense": ["dpr", "contriever", "splade"],
                "hybrid": ["hybrid"],                 "registered_custom": list(cls._retrievers.keys())}
