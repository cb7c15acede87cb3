"""Drop-in mirror of the reference's ``RetrievalService`` BM25 API
(/root/reference/rag_system/core/retrieval.py:95-506) running on the MI355X HIP engine.

Same names, argument meaning, result shape and error behaviour for the hot path:
``build_bm25_index(corpus)`` (:129), ``search_bm25(queries, top_k)`` (:203), ``get_stats()`` (:471),
``clear_cache()`` (:464), ``close()`` / context manager (:495-506), and the dense ``search_by_vector`` (:402-436).  The
document store (MemoryIndex) is outside this build's scope.

``top_k``: any value, like the reference (``k >= n_docs`` ranks the whole corpus, :281-284): rankings deeper than the
engine's 1024-row lists are paged with ``srx_search_after``; ``top_k <= 0`` returns ``{}`` for every query like the
reference's ``argpartition``.

What changes underneath: ``search_bm25`` scores the WHOLE query dict as one batch through
``srx_search`` (libsparse_rx.so) instead of looping ``simd_bm25_score`` + ``fast_topk_selection`` per query
(:210-229, :256-284).  There is no CPU fallback: without the HIP library / a GPU the calls raise.

Multi-GPU: when the process is a rank of an initialised ``torch.distributed`` group of more than one rank (one process
per GPU, backend "nccl" = RCCL), the SAME two calls shard the index by doc-id range: every rank passes the same corpus /
query dicts, ``build_bm25_index`` builds the rank's doc range with corpus-wide vocabulary, idf and avgdl
(distributed.build_sharded_host_index), ``search_bm25`` scores the batch on every shard, exchanges the per-shard top-k
over RCCL and merges (distributed.ShardedSearcher); every rank returns the dicts the single-GPU service returns
(backend.SparseBackend holds that wiring for this class and the registry mirrors).
"""
from __future__ import annotations

import logging
import os
import threading
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .backend import SparseBackend, SparseIndexViews, apply_operators, collapse_pool_depth
from .index import check_fuse_args, check_rescore_args, encode_queries, hybrid_depths, hybrid_search, mmr_pool_depth, rows_to_dict

logger = logging.getLogger(__name__)

NUMBA_AVAILABLE = False  # kept for get_stats() key compatibility (retrieval.py:476)


class RetrievalService(SparseIndexViews):
    """BM25 retrieval with the reference's API; scoring + top-k run on the GPU."""

    not_built = "BM25 index not built. Call build_bm25_index() first."  # mode "bm25", term_order "term": backend.SparseIndexViews
    search_door = "search_bm25"
    blank = "whitespace"  # no text or white space only is answered {} (:211-213); the cache key is the stripped text (:216), the cache always on

    def __init__(self, index_path=None, embedding_path=None, num_workers: int = 4, cache_size: int = 1000, *,
                 device: Optional[str] = None, tile_log2: int = 14, group=None, sharded: Optional[bool] = None,
                 shard_searcher_factory=None, one_copy: bool = True, **compat_kwargs):
        # index_path / embedding_path / num_workers are accepted for signature compatibility (retrieval.py:98-102);
        # README-only kwargs (use_simd, batch_size, monitor, ...) are swallowed.
        self.index_path = index_path
        self.embedding_path = embedding_path
        self.num_workers = num_workers
        self.cache_size = cache_size
        self.logger = logger
        # group: the torch.distributed group to shard over (None = the default group, when one is initialised);
        # shard_searcher_factory: test hook of backend.SparseBackend (the product never sets it)
        # sharded: None = automatic (a group of more than one rank), True = the sharded path even in a group of one rank
        # one_copy: only the compact copy of the postings stays in HBM (backend.SparseBackend)
        self._be = SparseBackend(device, tile_log2, group=group, searcher_factory=shard_searcher_factory, sharded=sharded, one_copy=one_copy)
        self.device = self._be.device
        self.tile_log2 = tile_log2
        self.k1: float = 1.2   # retrieval.py:116
        self.b: float = 0.75   # retrieval.py:117
        self._built_k1b: Optional[Tuple[float, float]] = None
        self.query_cache: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}
        self.cache_lock = threading.RLock()
        self.build_time = 0.0

    # -- reference attribute names (read-only views; host, dev, vocabulary, doc_ids, corpus_tf: backend.SparseIndexViews) --
    @property
    def idf_weights(self):
        return self.host.idf if self.host else None

    @property
    def doc_lengths(self):
        return self._be.doc_lengths  # the whole corpus' lengths (sharded: all-gathered at build)

    @property
    def avgdl(self) -> float:
        return self.host.avgdl if self.host else 0.0

    # -- build ------------------------------------------------------------------------------------------
    def build_bm25_index(self, corpus: Dict[str, Dict]) -> None:
        """retrieval.py:129-201 on the host (bit-equal arrays), then the device inverted index."""
        t0 = time.perf_counter()
        self._be.build(corpus, idf_kind="bm25")
        self._upload()
        self.build_time = time.perf_counter() - t0
        self.logger.info("BM25 index built in %.2fs (%d docs, %d terms, %d postings)", self.build_time,
                         self.host.n_docs, self.host.vocab_size, self.host.nnz)

    def _upload(self) -> None:
        self._be.upload("bm25", self.k1, self.b)
        self._built_k1b = (self.k1, self.b)
        with self.cache_lock:
            self.query_cache.clear()

    # -- search -----------------------------------------------------------------------------------------
    def search_bm25(self, queries: Dict[str, str], top_k: int = 10, *, allowed_docs=None, excluded_docs=None, must_terms=None,
                    any_terms=None, must_not_terms=None, operators: bool = False, where=None, collapse_by: Optional[str] = None,
                    per_group: int = 1, collapse_nulls: str = "own", collapse_depth: Optional[int] = None, expand_docs: Optional[int] = None,
                    expand_terms: int = 10, expand_weight: float = 0.5, expand_by: str = "score", boost=None,
                    boost_depth: Optional[int] = None, rank_model: bool = False, rank_pool: Optional[int] = None) -> Dict[str, Dict[str, float]]:
        """retrieval.py:203-231 semantics; one batched GPU call for all uncached queries.

        ``allowed_docs`` / ``excluded_docs`` (no reference counterpart: it has no filters): restrict the search to, or keep
        out of it, the named docs -- a sequence of doc ids for every query of the call, or a dict ``qid -> sequence`` (a qid
        missing from it is not filtered).  The result is the top ``top_k`` OF THE ALLOWED DOCS, exact
        (``srx_search_filtered``), not a filtered top list.  Giving both, or an unknown doc id, raises ``ValueError``; a
        filtered call neither reads nor writes the query cache; a sharded index refuses.

        ``must_terms`` / ``any_terms`` / ``must_not_terms`` (no reference counterpart either): term constraints -- a result must
        contain every word of ``must_terms``, at least one of ``any_terms`` (when given) and none of ``must_not_terms``; each
        a sequence of strings for every query, or a dict ``qid -> sequence``.  The words are tokenised like the corpus; a word
        the vocabulary does not know is contained in no doc.  The rows are built on the GPU from the posting lists
        (``srx_filter_from_terms``, include/sparse_rx_terms.h: n_docs / 8 bytes per distinct constraint, 1.25 MB at 10 M docs)
        and restrict the doc set only: scores and the ``score > 0`` rule are unchanged.  They combine with ``allowed_docs`` /
        ``excluded_docs`` and behave like them otherwise (no cache, a sharded index refuses).  ``operators=True``: the
        ``+word`` / ``-word`` words of every query text are read as must / must-not constraints
        (:func:`~.index.parse_operators`) and merged with the keywords.

        ``where`` (no reference counterpart): a field predicate over the columns of :meth:`set_doc_fields` -- one group
        ``{"must": [...], "should": [...], "must_not": [...]}`` (or a bare list of clauses) for every query, or a dict
        ``qid -> group``; the clauses are :meth:`~.fields.FieldTable.filter`'s.  The rows are built on the GPU
        (``srx_filter_from_fields``, include/sparse_rx_fields.h) and restrict the doc set only.  It combines with the doc and the
        term keywords (doc filter, then term rows, then field rows) and behaves like them otherwise: no cache, a sharded index
        refuses; without :meth:`set_doc_fields` it raises ``ValueError``.

        ``collapse_by`` (default None: nothing changes; no reference counterpart): the name of an int32 / int64 / category column
        of :meth:`set_doc_fields` -- a parent document, an author, a source.  The result is then the top ``top_k`` of the
        COLLAPSED complete ranking, exact: the ranking with every doc removed that has ``per_group`` better-ranked docs of its
        group (``srx_collapse_topk``, include/sparse_rx_collapse.h).  The ranking is read in pages on the GPU
        (:func:`~.backend.collapse_deep`: first ``min(max(4 * top_k, 64), 1024, n_docs)`` rows, then 1 024 at a time with
        ``srx_search_after``) until every query has ``top_k`` groups or its ranking ends.  ``collapse_nulls``: a doc without a
        value is a group of its "own" (default), all of them are "one" group, or they "drop" out.  ``collapse_depth`` (default
        None: no limit) stops reading after that many rows of the ranking; a query may then return FEWER than ``top_k`` docs
        although more groups exist further down -- that is not an error.  It works under the doc, term and field keywords (the
        collapsed ranking of the allowed docs) and bypasses the query cache as they do.  ``ValueError``: ``top_k`` above
        1 024, an unknown, float or set column, no :meth:`set_doc_fields`, a sharded index (columns are shard-local).

        ``expand_docs`` (default None: nothing changes; no reference counterpart): pseudo-relevance feedback, RM3.  With
        ``expand_docs=R`` (1..32; needs :meth:`enable_feedback`) the query is first searched ``R`` deep under the call's doc, term
        and field keywords (never collapsed); the query is then rebuilt on the GPU from its own terms and the ``expand_terms``
        (1..128) terms its ``R`` docs characterise best (``srx_feedback_expand``, include/ext/sparse_rx_feedback.h: alpha =
        1 - ``expand_weight``, beta = ``expand_weight`` in [0, 1], docs weighted by ``expand_by`` "score" or "uniform"), and the
        result is the existing search of that expanded query at ``top_k`` under the same keywords, ``collapse_by`` included.
        Nothing is copied back between the two passes for ``top_k`` <= 1 024.  The scores are those of the EXPANDED query, whose
        weights sum to at most 1: they are NOT comparable to plain BM25 scores.  Such a call bypasses the query cache.
        ``ValueError``: no :meth:`enable_feedback`, a sharded index, a keyword out of range.

        ``boost`` (default None: nothing changes; no reference counterpart): a spec :class:`~.boost.BoostResolver` takes --
        ``{"functions": [{"decay": {...}} | {"field_value": {...}} | {"curve": {...}}, ...], "score_mode", "boost_mode"}`` over the
        number columns of :meth:`set_doc_fields`: "prefer recent", "prefer popular".  The result is the top ``top_k`` of the
        BOOSTED complete ranking with its boosted scores, exact (``srx_boost_topk``, include/boost/sparse_rx_boost.h): the
        ranking is read in pages on the GPU (:func:`~.boost.boost_deep`) until no unseen doc can reach a query's k-th boosted
        score.  ``boost_depth`` (default None: no limit) stops after that many rows of the ranking; the result is then the
        boosted top of the rows read.  It works under the doc, term and field keywords and with ``expand_docs``, and bypasses
        the query cache.  ``ValueError``: ``collapse_by`` in the same call (chain :meth:`collapse` over the result), ``boost_mode``
        "replace" or a factor that can be negative under "multiply" (no bound exists), ``top_k`` above 1 024, an unknown or set
        column, no :meth:`set_doc_fields`, a sharded index.

        ``rank_model`` (default False: nothing changes; no reference counterpart): rerank with the learned model of
        :meth:`set_rank_model` (``srx_ltr_topk``, include/ltr/sparse_rx_ltr.h).  The result is POOL-RELATIVE: the first ``rank_pool``
        rows of this search under the call's other keywords (default ``min(max(4 * top_k, 100), 1024, n_docs)``), re-scored by the
        model and cut to ``top_k`` -- what ``rerank_model(search_bm25(top_k=rank_pool, ...), top_k)`` returns; the values are the
        model's scores.  ``ValueError``: no :meth:`set_rank_model`, a feature that names a column without :meth:`set_doc_fields`,
        a set column, "sparse_score" / "dense_score" (:meth:`search_hybrid` only), ``rank_pool`` above 1 024, ``boost=`` in the same
        call (chain :meth:`boost_results`), a sharded index."""
        return self._search(queries, top_k, (allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, operators, where),
                            (collapse_by, per_group, collapse_nulls, collapse_depth), (expand_docs, expand_terms, expand_weight, expand_by),
                            boost, boost_depth, rank_model, rank_pool)

    def _before_search(self, top_k, expand) -> bool:
        if min(int(top_k), self._be.n_docs_total) <= 0:  # the reference's argpartition(-scores, 0)[:0] keeps nothing (:276-279)
            return False
        if (self.k1, self.b) != self._built_k1b:
            self._upload()  # k1 / b are plain attributes on the reference (:116-117): impacts depend on them
            if expand is not None:
                self._be.enable_feedback("bm25")  # the upload dropped the forward index; its rows do not depend on k1 / b
        return True

    def score_bm25(self, queries: Dict[str, str], candidates: Dict[str, Sequence[str]]) -> Dict[str, Dict[str, float]]:
        """The exact BM25 score of caller-named documents (no reference counterpart: it can only rank):
        ``{qid: {doc_id: score}}`` with every doc of ``candidates[qid]`` in the caller's order, scored with the arithmetic
        of :meth:`search_bm25` (``srx_score_docs``: a row ``search_bm25`` returned scores to the same float).  There is no
        ``score > 0`` filter: a doc no query term matches scores 0.0, as does every doc for a blank or all-OOV query; a qid
        without candidates gives ``{}``; an unknown doc id raises ``ValueError``.  All queries of the call run as one batch
        (ragged lists padded); the query cache is not used.  Sharded: every rank makes the same call and gets the same dict."""
        self._need_index()
        if (self.k1, self.b) != self._built_k1b:
            self._upload()
        return self._be.score_dicts(queries, candidates, order="term")

    # -- misc -------------------------------------------------------------------------------------------
    # -- dense side (retrieval.py:320-339, 402-436) ----------------------------------------------------------
    def set_embeddings(self, embeddings, storage: str = "f32", screen=None, oversample: int = 4) -> None:
        """Make a [n_docs, dim] float32 matrix (row i = doc_ids[i]) the ``embedding_index`` and put it on the GPU.  The
        reference memory-maps ``embedding_path`` with the row count of its document store (``_load_embeddings``,
        retrieval.py:320-339); the store is out of scope here, so the rows come from the caller or, in
        :meth:`search_by_vector`, from ``embedding_path`` once ``build_bm25_index`` has fixed ``doc_ids``.

        ``storage``: how the GPU keeps the rows.  "f32" (default): as given (``DenseF32Index``, an exact streaming matvec per
        pass of four queries).  "f16" / "bf16" (no reference counterpart): rounded to half precision and searched a whole
        query batch at a time by MFMA (``DenseHalfIndex``, include/sparse_rx_half.h); :meth:`search_by_vector`,
        :meth:`search_hybrid` and :meth:`score_by_vector` then return the scores OF THE ROUNDED ROWS (and rounded query
        vectors).  Any other value raises ``ValueError``.

        ``screen``: None (default: every search reads every row) or "binary" (no reference counterpart): 1-bit codes of the rows
        (``DenseBinaryIndex``, include/binary/sparse_rx_binary.h; centred on the column means) screen the corpus by Hamming
        distance under the search's filter, and the rows above are read only for the ``min(k * oversample, 1024)`` nearest
        (``ScreenedDenseIndex``).  :meth:`search_by_vector` and the dense side of :meth:`search_hybrid` then return the best of
        that pool -- approximate unless the pool covers the allowed docs; the scores are those of the storage.  The rows stay
        resident: the screen saves bandwidth, not memory.  Not offered with a sharded index.  Any other value raises
        ``ValueError``, as does ``oversample < 1``."""
        from .dense import DenseF32Index, DenseHalfIndex
        storage = str(storage).lower()
        if storage not in ("f32", "f16", "bf16"):
            raise ValueError(f"storage must be 'f32', 'f16' or 'bf16', got {storage!r}")
        if screen is not None:
            from .binary import check_oversample
            if screen != "binary":
                raise ValueError(f"screen must be None or 'binary', got {screen!r}")
            oversample = check_oversample(oversample)
            if self._be.sharded():
                raise ValueError("screen='binary' is not offered with a sharded index")
        e = np.asarray(embeddings, dtype=np.float32)
        if e.ndim != 2 or (self.doc_ids and e.shape[0] != len(self.doc_ids)):
            raise ValueError("embeddings must be [n_docs, dim] with one row per document")
        self.embedding_index = e
        # either index streams a memory map to the device in <= 64 MB chunks
        self._dense = DenseF32Index(e, device=self.device) if storage == "f32" else DenseHalfIndex(e, dtype=storage, device=self.device)
        self.embedding_storage = storage
        self.embedding_screen, self.embedding_oversample = screen, (oversample if screen is not None else None)
        if screen is not None:
            from .binary import DenseBinaryIndex, ScreenedDenseIndex
            self._dense = ScreenedDenseIndex(self._dense, DenseBinaryIndex(e, center="mean", device=self.device), oversample)

    def search_by_vector(self, query_vector: np.ndarray, k: int = 10, min_score: float = 0.0, *, allowed_docs=None,
                         excluded_docs=None, must_terms=None, any_terms=None, must_not_terms=None, where=None) -> List[Dict]:
        """retrieval.py:402-436: ``np.dot(embedding_index, query_vector)`` + top-k on the GPU (``srx_dense_search_f32``),
        the ``min_score`` cut and the ``[{"doc_id", "score"}]`` result as in the reference.

        The engine ranks positive values only, so the unshifted search runs first: when it fills all k rows they are all
        > 0 >= ``min_score`` and ARE the reference's top-k -- the common case, exact, no host work.  Only when fewer than k
        docs score above 0 and ``min_score <= 0`` (the default 0.0 admits rows with a score of exactly 0, negative
        thresholds admit negative scores, :425-427) a second pass shifts the scores by a bound on the largest |score| so
        that every doc is rankable; its k rows are re-scored on the host with ``np.dot`` (fp32, the reference's own
        expression) and re-ranked, so the shift never shows in the result.  The shift coarsens that pass's ranking to
        ulp(offset): docs whose true scores differ by less can swap places at the k-th boundary (scores <= 0 only).

        ``allowed_docs`` / ``excluded_docs``: a sequence of doc ids, as in :meth:`search_bm25`; both passes rank the allowed
        docs alone (``srx_dense_search_f32_filtered``).  ``must_terms`` / ``any_terms`` / ``must_not_terms``: a sequence of
        strings each, as in :meth:`search_bm25` -- keyword-constrained vector search: the docs are those whose TEXT satisfies
        the constraint (the BM25 index's posting lists), so it needs ``build_bm25_index``.  ``where``: one group, as in
        :meth:`search_bm25` -- vector search under a metadata predicate; it needs :meth:`set_doc_fields`.

        With half-precision storage (:meth:`set_embeddings`) both passes run on the half index (``srx_dense_search_half``):
        the first pass returns the scores of the rounded rows; the second pass still re-scores its rows on the host with the
        f32 rows the service was given."""
        for what, given in (("must_terms", must_terms), ("any_terms", any_terms), ("must_not_terms", must_not_terms)):
            if isinstance(given, dict):
                raise ValueError(f"{what} of search_by_vector must be a sequence of strings (there is one query)")
        if where is not None:
            from .fields import is_group
            if not is_group(where):
                raise ValueError("where of search_by_vector must be one group (there is one query)")
        self._ensure_dense()
        q = np.asarray(query_vector, dtype=np.float32)
        kk = max(1, min(int(k), self._dense.n_docs))
        flt = self._dense_filter({"q": None}, allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, where, "search_by_vector")
        flt = {} if flt is None else {"filter": flt[0]}  # one query: its row is row 0
        d, s, n = self._dense.search(q, kk, **flt)
        if min_score > 0 or int(n[0]) == kk:
            idx, sc = d[0, : int(n[0])].astype(np.int64), s[0, : int(n[0])]
        else:
            # |score| <= |q|_2 * max row norm (Cauchy-Schwarz): the smallest shift that makes every doc rankable keeps
            # the most fp32 resolution for the ranking (the shifted scores are only used to pick the k rows)
            bound = float(np.linalg.norm(q.astype(np.float64))) * self._dense.max_row_norm()
            # half storage scores the ROUNDED query: rounding raises a component by up to 2^-9 (bf16) / 2^-12 (f16) of itself,
            # so its norm can exceed |q|_2 by 0.2 %: the margin covers that (max_row_norm is already that of the rounded rows)
            offset = bound * (1.001 if getattr(self, "embedding_storage", "f32") == "f32" else 1.01) + 1e-30
            d, s, n = self._dense.search(q, kk, score_offset=offset, **flt)
            idx = d[0, : int(n[0])].astype(np.int64)
            sc = np.dot(self.embedding_index[idx], q).astype(np.float32)  # the reference's fp32 expression on the k rows
            order = np.argsort(-sc, kind="stable")
            idx, sc = idx[order], sc[order]
        results = []
        for i, score in zip(idx, sc):
            if score < min_score:
                break
            if self.doc_ids and i < len(self.doc_ids):
                results.append({"doc_id": self.doc_ids[int(i)], "score": float(score)})
            elif not self.doc_ids:
                results.append({"doc_id": str(int(i)), "score": float(score)})
        return results

    def _dense_filter(self, queries, allowed_docs, excluded_docs, must_terms=None, any_terms=None, must_not_terms=None, where=None,
                      call: str = "search_hybrid"):
        """The filter keywords as (DocFilter over the embedding rows, spec), or None when none constrains a query"""
        terms = not (must_terms is None and any_terms is None and must_not_terms is None)
        if allowed_docs is None and excluded_docs is None and not terms and where is None:
            return None
        if self.host is not None:
            spec = self._be.filter_spec(queries, allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, where, call)
        elif where is not None:
            raise ValueError(f"{call}(where=...) needs the docs' fields: call build_bm25_index() and set_doc_fields() first")
        elif terms:
            raise ValueError("must_terms / any_terms / must_not_terms need the BM25 index (its posting lists): call build_bm25_index() first")
        else:  # embeddings without a BM25 index: docs are named by their row number
            from .backend import RowOfIds, doc_filter_spec
            spec = doc_filter_spec(RowOfIds.numbered(self._dense.n_docs).row_of, queries, allowed_docs, excluded_docs)
        if spec is None:
            return None
        return spec.on_device(self._dense).for_index(self._dense), spec

    def _ensure_dense(self) -> None:
        if getattr(self, "_dense", None) is None and self.embedding_path and os.path.exists(str(self.embedding_path)) and self.doc_ids:
            n = len(self.doc_ids)
            dim = os.path.getsize(str(self.embedding_path)) // (n * 4)  # retrieval.py:324-328
            self.set_embeddings(np.memmap(str(self.embedding_path), dtype="float32", mode="r", shape=(n, dim)))
        if getattr(self, "_dense", None) is None:
            raise ValueError("No embedding index available")

    def search_hybrid(self, queries: Dict[str, str], query_vectors: Dict[str, np.ndarray], top_k: int = 10, *,
                      sparse_weight: float = 0.3, dense_weight: float = 0.7, fusion: str = "weighted", rrf_c: float = 60.0,
                      candidates: Optional[int] = None, rescore: bool = False, allowed_docs=None,
                      excluded_docs=None, mmr_lambda: Optional[float] = None, mmr_pool: Optional[int] = None,
                      mmr_similarity: str = "cosine", must_terms=None, any_terms=None, must_not_terms=None,
                      operators: bool = False, late_query_tokens=None, late_pool: Optional[int] = None, where=None,
                      collapse_by: Optional[str] = None, per_group: int = 1, collapse_nulls: str = "own",
                      collapse_pool: Optional[int] = None, boost=None, boost_pool: Optional[int] = None, rank_model: bool = False,
                      rank_pool: Optional[int] = None) -> Dict[str, Dict[str, float]]:
        """Hybrid retrieval (no reference counterpart: its ``hybrid`` retriever type is configured but not implemented):
        the BM25 top list of every query text and the f32 ``embedding_index`` top list of its vector in
        ``query_vectors[qid]``, fused on the GPU into one ranking (``srx_fuse_topk``; include/sparse_rx.h has the exact
        arithmetic).  ``fusion`` "weighted": each side's scores divided by its best score, then
        ``sparse_weight * s + dense_weight * d``; "rrf": ``weight / (rrf_c + rank)`` per side.  A doc only one side
        retrieved scores with that side alone -- unless ``rescore=True`` ("weighted" only; with "rrf" it raises
        ``ValueError``): then each list is completed with the other side's exact score of its docs before the fusion
        (``srx_score_docs``, ``srx_dense_score_docs_f32``, ``srx_fuse_topk_scored``; include/sparse_rx_rescore.h), and the
        fused score of a returned doc no longer depends on ``candidates``.  A query without in-vocabulary terms is the
        dense list re-scored.
        ``candidates``: rows fetched from each side (default ``top_k``, capped at ``min(candidates, n_docs, 1024)``).
        All queries of the call run as one batch: sparse search, dense search and fusion stay on the device, followed by
        one synchronisation and the copy back.  Returns ``{qid: {doc_id: fused score}}`` in rank order, ``{}`` for a blank
        query; ``top_k <= 0`` gives ``{}`` per query.  ``top_k`` > 1024 raises ``ValueError``: a fused ranking deeper
        than the engine's lists is not paged, and a silently shorter list would be worse than an error.  With one weight
        0 the result is the other side's set, but equal normalised scores rank by doc id.  The query cache is not used.
        Needs the whole index on one GPU.
        ``allowed_docs`` / ``excluded_docs`` as in :meth:`search_bm25`: the filter goes to both sides, so the fused list is
        the fusion of the two FILTERED top lists (``rescore=True`` included: every doc of either list is an allowed one).
        With half-precision storage (:meth:`set_embeddings`) the dense side is ``srx_dense_search_half`` /
        ``srx_dense_score_docs_half``: the dense scores are those of the rounded rows, everything else is unchanged.
        ``mmr_lambda`` (default None: no diversification, every step and result is as described above): a number in [0, 1]
        makes the call return a DIVERSIFIED ``top_k``.  The fused ranking is then taken ``mmr_pool`` deep (default
        ``min(max(4 * top_k, top_k), 256, n_docs)``; more than 256 raises ``ValueError``), ``candidates`` defaults to at
        least the pool, and Maximal Marginal Relevance picks ``top_k`` of the pool on the device (``srx_mmr_select_f32`` /
        ``_half``, include/sparse_rx_mmr.h; ``mmr_similarity`` "cosine" or "dot" of the embedding rows) -- still one
        synchronisation and one copy back per call.  The result is what ``diversify(search_hybrid(top_k=mmr_pool, ...),
        top_k)`` returns: the docs in SELECTION order, each with its fused score, so the values are not descending.  Works
        with ``rescore=True`` and with the filter keywords (the pool is then the filtered fusion).
        ``must_terms`` / ``any_terms`` / ``must_not_terms`` / ``operators`` as in :meth:`search_bm25`: the term-built rows go to
        both sides like a doc filter's (``rescore=True`` and ``mmr_lambda`` included) and combine with ``allowed_docs`` /
        ``excluded_docs``.
        ``late_query_tokens`` (default None: nothing changes): ``{qid: f32[t_q, dim]}`` makes the call return the fused
        ranking RERANKED by late interaction.  The fused ranking is then taken ``late_pool`` deep (default
        ``min(max(top_k, 100), 1024, n_docs)``; more than 1024 raises ``ValueError``), ``candidates`` defaults to at least the
        pool, and the MaxSim scores over the token index of :meth:`set_token_embeddings` pick and order ``top_k`` of the pool
        on the device (``srx_maxsim_rerank_half``, include/sparse_rx_maxsim.h) -- still one synchronisation and one copy
        back.  The result is what ``rerank_late(search_hybrid(top_k=late_pool, ...), late_query_tokens, top_k)`` returns: the
        values are MaxSim scores.  Works with ``rescore=True`` and the filter / term keywords; together with ``mmr_lambda`` it
        raises ``ValueError`` (chain :meth:`rerank_late` and :meth:`diversify` instead).
        ``where`` as in :meth:`search_bm25`: the field-built rows go to both sides like a doc filter's (``rescore=True``,
        ``mmr_lambda`` and ``late_query_tokens`` included) and combine with the doc and the term keywords.
        ``collapse_by`` / ``per_group`` / ``collapse_nulls`` (default None: nothing changes) as in :meth:`search_bm25`: at most
        ``per_group`` docs per value of the column.  The fused ranking is then taken ``collapse_pool`` deep (default
        ``min(max(4 * top_k, 100), 1024, n_docs)``; more than 1024 raises ``ValueError``), ``candidates`` defaults to at least the
        pool, and the pool is collapsed on the device (``srx_collapse_topk``) before the one copy back.  Unlike
        :meth:`search_bm25`'s the result is POOL-RELATIVE, not the collapsed complete ranking: it is what
        ``collapse(search_hybrid(top_k=collapse_pool, ...), collapse_by, top_k, ...)`` returns, and it can be SHORTER than
        ``top_k`` when the pool holds fewer groups.  With ``late_query_tokens`` the order is fuse, rerank the whole ``late_pool``,
        collapse to ``top_k`` (``collapse_pool`` is not used): ``collapse(rerank_late(search_hybrid(top_k=late_pool, ...), tokens,
        late_pool), ...)``.  With ``mmr_lambda`` it is fuse ``collapse_pool`` deep, collapse to ``mmr_pool``, MMR to ``top_k``:
        ``diversify(collapse(search_hybrid(top_k=collapse_pool, ...), collapse_by, mmr_pool, ...), top_k, ...)``.
        ``boost`` (default None: nothing changes) as in :meth:`search_bm25`, every ``boost_mode`` allowed ("replace" too).  The fused
        ranking is taken ``boost_pool`` deep (default ``min(max(4 * top_k, 100), 1024, n_docs)``; more than 1024 raises
        ``ValueError``; with ``late_query_tokens`` the pool is ``late_pool``, reranked as a whole first), ``candidates`` defaults to
        at least the pool, and the pool is boosted on the device (``srx_boost_topk``) before the one copy back.  The result is
        POOL-RELATIVE: what ``boost_results(search_hybrid(top_k=boost_pool, ...), boost, top_k)`` returns, values = boosted fused
        scores.  With ``collapse_by`` the whole boosted pool is then collapsed (``collapse_pool`` is not used), with ``mmr_lambda``
        the boosted (and collapsed) pool's first ``mmr_pool`` rows are diversified.
        ``rank_model`` (default False: nothing changes) as in :meth:`search_bm25`: the fused ranking is taken ``rank_pool`` deep
        (default ``min(max(4 * top_k, 100), 1024, n_docs)``; more than 1024 raises ``ValueError``; with ``late_query_tokens`` the pool
        is ``late_pool``) and re-scored by the model of :meth:`set_rank_model` on the device (``srx_ltr_topk``).  "score" is the
        fused (or late) score and "rank" the pool position; the feature names "sparse_score" and "dense_score" are the EXACT BM25
        and embedding scores of the pool's docs (``srx_score_docs``, ``srx_dense_score_docs_f32`` / ``_half``), computed on the
        device and stacked into the model's extra plane, so nothing is copied back before the cut.  Not with ``boost=``.
        In one sentence: the steps run in the order late rerank, boost or model, collapse, MMR, each only if its keyword is given; the
        fusion is as deep as the FIRST step's pool, and a step keeps all its rows for a boost, model or collapse behind it, ``mmr_pool``
        rows for MMR behind it, ``top_k`` rows as the last -- never more than it was handed."""
        if late_query_tokens is not None and mmr_lambda is not None:
            raise ValueError("late_query_tokens and mmr_lambda do not combine in one call: chain rerank_late() and diversify()")
        if operators:
            queries, must_terms, must_not_terms = apply_operators(queries, must_terms, must_not_terms)
        fusion = str(fusion).lower()
        check_fuse_args(fusion, (sparse_weight, dense_weight), rrf_c)
        rescore = check_rescore_args(fusion, rescore)
        n_docs = self._be.n_docs_total
        k, cand = hybrid_depths(top_k, candidates, n_docs)
        pools = {}  # stage -> the depth its pool keyword gives: the first stage's is the fused depth, MMR's is also what is kept for it
        if mmr_lambda is not None:
            from .dense import check_mmr_args
            check_mmr_args(mmr_lambda, mmr_similarity)
            pools["mmr"] = mmr_pool_depth(top_k, mmr_pool, n_docs)
        if late_query_tokens is not None:
            from .late import late_pool_depth
            pools["late"] = late_pool_depth(top_k, late_pool, n_docs)
        if self._be.sharded():
            raise ValueError("hybrid search needs the whole index on one GPU (the dense corpus is not sharded)")
        self._need_index()
        self._ensure_dense()
        collapse = self._be.collapse_spec(collapse_by, per_group, collapse_nulls, None, top_k, "search_hybrid")
        if collapse is not None and late_query_tokens is None:
            pools["collapse"] = collapse_pool_depth(top_k, collapse_pool, n_docs)
        boosted = self._be.boost_spec(boost, None, top_k, "search_hybrid", exact=False)
        if boosted is not None:  # range-checked under late_query_tokens too, where it is not used
            pools["boost"] = collapse_pool_depth(top_k, boost_pool, n_docs, "boost_pool")
        ranked = self._be.rank_spec(rank_model, rank_pool, top_k, "search_hybrid", boost, hybrid=True)
        if ranked is not None:
            pools["model"] = ranked.pool
        stages = [name for name, given in (("late", late_query_tokens), ("boost", boosted), ("model", ranked), ("collapse", collapse),
                                           ("mmr", mmr_lambda)) if given is not None]
        depth = pools[stages[0]] if stages else k  # how deep the fusion is taken
        if stages and candidates is None:
            # at least the fused depth.  Collapse + MMR alone also reach for mmr_pool: an irregularity, but it decides which rows are fetched
            cand = hybrid_depths(top_k, max(int(top_k), depth, pools["mmr"] if stages == ["collapse", "mmr"] else 1), n_docs)[1]
        results: Dict[str, Dict[str, float]] = {qid: {} for qid in queries}
        live = [(qid, text) for qid, text in queries.items() if text and text.strip()]
        if k <= 0 or not live:
            return results
        vecs = []
        for qid, _ in live:
            if qid not in query_vectors:
                raise ValueError(f"no query vector for {qid!r}")
            v = np.asarray(query_vectors[qid], dtype=np.float32)
            if v.shape != (self._dense.dim,):
                raise ValueError(f"query vector of {qid!r} has shape {v.shape}, expected ({self._dense.dim},)")
            vecs.append(v)
        if (self.k1, self.b) != self._built_k1b:
            self._upload()
        q_ptr, q_term, q_weight = encode_queries([text for _, text in live], self.host.vocabulary)
        flt = {}
        fs = self._dense_filter(queries, allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, where)  # one DocFilter serves both sides: same rows, same device
        if fs is not None:
            import torch
            q_rows = np.asarray([fs[1].row_of_qid[qid] for qid, _ in live], dtype=np.int32)
            flt = {"filter": fs[0], "q_filter": torch.as_tensor(q_rows, device=self._dense.device)}

        def dense_search(kb):
            import torch
            return self._dense.search_device(torch.as_tensor(np.stack(vecs), device=self._dense.device), kb, **flt)

        def dense_score(cand_doc, cand_count):
            import torch
            return self._dense.score_docs_device(torch.as_tensor(np.stack(vecs), device=self._dense.device), cand_doc, cand_count)

        if boosted is not None:
            from .boost import BoostFn
            bfn = BoostFn(self._be.field_table(), boosted)
        if late_query_tokens is not None:
            from .late import stack_query_tokens
            tokens = self._ensure_late()
            q_tok, q_cnt = stack_query_tokens(late_query_tokens, [qid for qid, _ in live], tokens.dim)

        def post(f_doc, f_score, f_count):  # the fused triple, depth wide, still on the device, through the stages
            import torch
            width = depth  # every stage returns as many columns as it is asked to keep
            for stage, follower in zip(stages, stages[1:] + [None]):
                keep = min(k, width) if follower is None else min(pools["mmr"], width) if follower == "mmr" else width
                if stage == "late":
                    f_doc, f_score, f_count = tokens.rerank_device(torch.as_tensor(q_tok, device=tokens.device), torch.as_tensor(q_cnt, device=tokens.device),
                                                                   f_doc, f_count, keep)
                elif stage == "boost":
                    f_doc, f_score, f_count = bfn(f_doc, f_score, f_count, keep)
                elif stage == "model":  # the pool's exact scores of both sides become the first two extra slots
                    from .index import _batch_to_device
                    exact = None if not ranked.named_extra else torch.stack([self.dev.score_docs_device(*_batch_to_device(torch, q_ptr, q_term, q_weight, self.dev.device), f_doc, f_count),
                                         dense_score(f_doc, f_count)], dim=2)
                    f_doc, f_score, f_count = ranked(f_doc.contiguous(), f_score.contiguous(), f_count, keep, extra=exact)
                elif stage == "collapse":
                    f_doc, f_score, f_count = self._be.field_table().collapse_device(collapse.by, f_doc, f_score, f_count, keep, collapse.per_group,
                                                                                     collapse.nulls)
                else:
                    f_doc, f_score, _, f_count = self._dense.mmr_device(f_doc, f_score, f_count, keep, mmr_lambda, mmr_similarity)
                width = keep
            return f_doc, f_score, f_count

        doc, score, count = hybrid_search(self.dev, q_ptr, q_term, q_weight, dense_search, cand, cand, depth, fusion, (sparse_weight, dense_weight),
                                          rrf_c, rescore, dense_score, **(dict(flt, post=post) if stages else flt))  # no stage: nothing is added
        for i, (qid, _) in enumerate(live):
            results[qid] = rows_to_dict(self.host.doc_ids, doc, score, count, i)
        return results

    def score_by_vector(self, query_vectors: Dict[str, np.ndarray], candidates: Dict[str, Sequence[str]]) -> Dict[str, Dict[str, float]]:
        """The dense twin of :meth:`score_bm25`: ``{qid: {doc_id: score}}`` with the ``embedding_index`` score of every doc
        of ``candidates[qid]`` for ``query_vectors[qid]``, in the caller's order, with the arithmetic of the dense search
        (``srx_dense_score_docs_f32``: a row :meth:`search_hybrid`'s dense side returned scores to the same float).  No
        ``score > 0`` filter; a qid without candidates gives ``{}``; an unknown doc id raises ``ValueError``.  One batch
        (ragged lists padded with -1, passed with their lengths); no cache.  With half-precision storage the scores are those
        of the rounded rows (``srx_dense_score_docs_half``), bit for bit what the half search returns."""
        from .backend import RowOfIds, scores_to_dicts
        self._ensure_dense()
        if self.host is not None:
            results, live, cand_doc, cand_count = self._be.candidate_block(query_vectors, candidates)  # its doc id -> row map is kept
        else:  # embeddings without a BM25 index: docs are named by their row number, as search_by_vector names them
            results, live, cand_doc, cand_count = RowOfIds.numbered(self._dense.n_docs).candidate_block(query_vectors, candidates)
        if not live:
            return results
        vecs = [np.asarray(v, dtype=np.float32) for _, v, _ in live]
        for (qid, _, _), v in zip(live, vecs):
            if v.shape != (self._dense.dim,):
                raise ValueError(f"query vector of {qid!r} has shape {v.shape}, expected ({self._dense.dim},)")
        return scores_to_dicts(results, live, self._dense.score_docs(np.stack(vecs), cand_doc, cand_count))

    def diversify(self, results: Dict[str, Dict[str, float]], top_k: int = 10, *, mmr_lambda: float = 0.5,
                  similarity: str = "cosine") -> Dict[str, Dict[str, float]]:
        """Diversified top-k of ranked lists (no reference counterpart: it cannot diversify): Maximal Marginal Relevance over
        ``results`` = ``{qid: {doc_id: score}}`` as any search of this service returns it (the dict order is the list order).
        Each pick maximises ``mmr_lambda * score - (1 - mmr_lambda) * (largest similarity to a doc already picked)``, the
        similarity ("cosine" or "dot") taken between the ``embedding_index`` rows of the docs -- the rounded rows with
        half-precision storage -- on the GPU (``srx_mmr_select_f32`` / ``srx_mmr_select_half``, include/sparse_rx_mmr.h has
        the exact arithmetic; ties go to the doc listed first).  All queries of the call run as one batch.

        Returns the same shape with ``top_k`` docs per query (fewer when the list is shorter) in SELECTION order, each with
        its ORIGINAL score: the values of a returned dict are therefore NOT descending.  ``mmr_lambda = 1`` keeps the order
        of the scores.  ``{}`` stays ``{}``, a qid with an empty list keeps it, ``top_k <= 0`` gives ``{}`` per query.
        ``ValueError``: an unknown doc id, a list longer than 256 docs (no silent truncation), ``mmr_lambda`` outside [0, 1],
        an unknown ``similarity``, a sharded index (the embedding rows are not sharded)."""
        from .backend import RowOfIds
        from .dense import check_mmr_args
        check_mmr_args(mmr_lambda, similarity)
        if self._be.sharded():
            raise ValueError("diversify needs the whole index on one GPU (the dense corpus is not sharded)")
        if not results:
            return {}
        self._ensure_dense()
        lists = {qid: list(row) for qid, row in results.items()}
        if self.host is not None:
            out, live, cand_doc, cand_count = self._be.candidate_block(results, lists)
            doc_ids = self.host.doc_ids
        else:  # embeddings without a BM25 index: docs are named by their row number, as search_by_vector names them
            out, live, cand_doc, cand_count = RowOfIds.numbered(self._dense.n_docs).candidate_block(results, lists)
            doc_ids = None
        m = int(cand_doc.shape[1])
        if m > 256:
            raise ValueError(f"diversify takes lists of at most 256 docs, got one of {m} (no silent truncation)")
        if not live or int(top_k) <= 0:
            return out
        rel = np.zeros(cand_doc.shape, dtype=np.float32)
        for i, (qid, _, cands) in enumerate(live):
            rel[i, : len(cands)] = [results[qid][d] for d in cands]
        doc, score, _, count = self._dense.mmr(cand_doc, rel, cand_count, min(int(top_k), m), mmr_lambda, similarity)
        for i, (qid, _, _) in enumerate(live):
            out[qid] = {(doc_ids[int(doc[i, j])] if doc_ids is not None else str(int(doc[i, j]))): float(score[i, j]) for j in range(int(count[i]))}
        return out

    def collapse(self, results, by: str, top_k: int = 10, per_group: int = 1, nulls: str = "own"):
        """Collapse ranked lists by a field (no reference counterpart: it does not group results): at most ``per_group`` docs per
        value of the column ``by`` of :meth:`set_doc_fields`, over ``results`` = ``{qid: {doc_id: score}}`` as any search of this
        service, :meth:`rerank_late` or :meth:`diversify` returns it (the dict order is the list order), on the GPU
        (``srx_collapse_topk``, include/sparse_rx_collapse.h).  A value may also be :meth:`search_by_vector`'s list of
        ``{"doc_id", "score"}`` dicts and comes back in that shape.  All lists of the call run as one batch.

        Returns the first ``top_k`` survivors of every list in list order -- a subsequence, every value as it was given; the
        scores are never looked at.  ``nulls``: a doc without a value is a group of its "own" (default), all of them are "one"
        group, or they "drop" out.  The result is relative to the lists GIVEN: a deeper list can hold more groups
        (:meth:`search_bm25`'s ``collapse_by=`` reads the ranking as deep as it takes).  ``{}`` stays ``{}``, ``top_k <= 0`` gives
        an empty list per query.  ``ValueError``: an unknown doc id, a list longer than 2 048 docs (no silent truncation), an
        unknown, float or set column, ``per_group`` < 1, no :meth:`set_doc_fields`, a sharded index."""
        return self._be.collapse_results(results, by, top_k, per_group, nulls, "collapse")

    # -- late interaction (no reference counterpart) -----------------------------------------------------------
    def set_token_embeddings(self, token_embeddings, storage: str = "f16") -> None:
        """Put the TOKEN vectors of the docs on the GPU for :meth:`rerank_late` (:class:`~.late.TokenIndex`; rounded to
        ``storage`` "f16" or "bf16").  ``token_embeddings``: ``{doc_id: f32[t_d, dim]}`` with every indexed doc present (``t_d``
        may be 0), or ``(matrix f32[n_tok, dim], counts)`` with the docs' tokens in ``doc_ids`` order.  Needs the BM25 index
        (it fixes ``doc_ids``) and the whole index on one GPU.  ``ValueError`` otherwise, and for a missing or unknown doc, a
        shape mismatch, no token at all or a non-finite value."""
        from .dense import check_half_dtype
        from .late import TokenIndex
        storage = check_half_dtype(storage)
        if self._be.sharded():
            raise ValueError("late interaction needs the whole index on one GPU (the token store is not sharded)")
        self._need_index()
        ids = self.host.doc_ids
        if isinstance(token_embeddings, dict):
            known = set(ids)
            for d in token_embeddings:
                if d not in known:
                    raise ValueError(f"unknown doc id {d!r} among the token embeddings")
            mats = []
            for d in ids:
                if d not in token_embeddings:
                    raise ValueError(f"no token embeddings for doc {d!r} (a doc without tokens needs an empty [0, dim] matrix)")
                mats.append(np.asarray(token_embeddings[d], dtype=np.float32))
            dims = {t.shape[1] for t in mats if t.ndim == 2}
            if any(t.ndim != 2 for t in mats) or len(dims) != 1:
                raise ValueError("token embeddings must be [t_d, dim] matrices of one dim")
            matrix, counts = np.concatenate(mats, axis=0), [t.shape[0] for t in mats]
        else:
            matrix, counts = token_embeddings
            matrix = np.asarray(matrix, dtype=np.float32)
            if matrix.ndim != 2 or len(counts) != len(ids):
                raise ValueError("token embeddings must be (f32[n_tok, dim], one token count per document)")
        self._late = TokenIndex.from_token_embeddings(matrix, counts, dtype=storage, device=self.device)
        self.token_storage = storage

    def _ensure_late(self):
        if getattr(self, "_late", None) is None:
            raise ValueError("No token index available. Call set_token_embeddings() first.")
        return self._late

    def rerank_late(self, results: Dict[str, Dict[str, float]], query_tokens, top_k: int = 10) -> Dict[str, Dict[str, float]]:
        """Late-interaction rerank of ranked lists (no reference counterpart): ``results`` = ``{qid: {doc_id: score}}`` as any
        search of this service returns it, ``query_tokens`` = ``{qid: f32[t_q, dim]}``.  Every listed doc is scored
        ``sum over the query's tokens of the largest similarity to any token of the doc`` over the token index of
        :meth:`set_token_embeddings`, on the GPU (``srx_maxsim_rerank_half``, include/sparse_rx_maxsim.h has the exact
        arithmetic).  All queries of the call run as one batch.

        Returns ``{qid: {doc_id: maxsim_score}}`` with the ``top_k`` best docs per query (fewer when the list is shorter) by
        (score descending, row of the doc ascending); scores may be negative or 0 (a doc without tokens scores 0).  ``{}``
        stays ``{}``, a qid with an empty list gives ``{}``, ``top_k <= 0`` gives ``{}`` per query.  ``ValueError``: an
        unknown doc id, a list longer than 1024 docs (no silent truncation), more than 128 query tokens, missing query
        tokens, no token index, a sharded index."""
        from .late import LATE_MAX_M, stack_query_tokens
        if self._be.sharded():
            raise ValueError("late interaction needs the whole index on one GPU (the token store is not sharded)")
        if not results:
            return {}
        tokens = self._ensure_late()
        out, live, cand_doc, cand_count = self._be.candidate_block(results, {qid: list(row) for qid, row in results.items()})
        m = int(cand_doc.shape[1])
        if m > LATE_MAX_M:
            raise ValueError(f"rerank_late takes lists of at most {LATE_MAX_M} docs, got one of {m} (no silent truncation)")
        q_tok, q_cnt = stack_query_tokens(query_tokens, [qid for qid, _, _ in live], tokens.dim)
        if not live or int(top_k) <= 0:
            return out
        doc, score, count = tokens.rerank(q_tok, q_cnt, cand_doc, cand_count, min(int(top_k), m))
        for i, (qid, _, _) in enumerate(live):
            out[qid] = rows_to_dict(self.host.doc_ids, doc, score, count, i)
        return out

    def clear_cache(self) -> None:
        with self.cache_lock:
            self.query_cache.clear()

    def get_stats(self) -> Dict[str, object]:
        """Same keys as retrieval.py:471-493, plus backend facts."""
        stats: Dict[str, object] = {"cache_size": 0, "query_cache_size": len(self.query_cache),
                                    "numba_available": NUMBA_AVAILABLE, "backend": "hip-gfx950"}
        stats["n_gpus"] = self._be.world()  # doc-range shards (one process per GPU); 1 = the whole index on one card
        if self.host is not None:
            h = self.host  # sharded: this rank's rows -- density and memory are the shard's, num_docs the corpus'
            density = h.nnz / max(1, h.n_docs * h.vocab_size)
            memory_mb = (h.data.nbytes + h.indices.nbytes + h.indptr.nbytes) / (1024 * 1024)
            stats.update({"num_docs": self._be.n_docs_total, "vocab_size": h.vocab_size, "matrix_density": density,
                          "bm25_memory_mb": memory_mb, "avgdl": h.avgdl})
            if self._be.sharded():
                stats["shard_docs"], stats["shard_doc_base"] = h.n_docs, self._be.doc_base
        if self.dev is not None:
            stats["device_index_mb"] = self.dev.device_bytes() / (1024 * 1024)
        if getattr(self, "_dense", None) is not None:
            stats["embedding_storage"] = getattr(self, "embedding_storage", "f32")  # "f32", "f16" or "bf16" (set_embeddings)
            stats["embedding_screen"] = getattr(self, "embedding_screen", None)     # None or "binary"
            stats["embedding_oversample"] = getattr(self, "embedding_oversample", None)
        return stats

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close()

    def close(self) -> None:
        if getattr(self, "_late", None) is not None:
            self._late.close()
            self._late = None
        self._be.close()
        self.clear_cache()
