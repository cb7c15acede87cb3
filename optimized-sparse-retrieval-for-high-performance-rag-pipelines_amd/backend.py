"""The engine behind the three API mirrors (``RetrievalService``, ``OptimizedBM25Retriever``, ``OptimizedRetriever``):
host index -> device index -> batched search, on one GPU or doc-range sharded over the ranks of a ``torch.distributed``
group (one process per GPU; backend "nccl" = RCCL over xGMI).

The reference has one process and one index (rag_system/core/retrieval.py:129-231); its API is kept as it is.  When
the calling process is a rank of an initialised group of W > 1 ranks, every rank makes the SAME calls with the SAME
corpus / query dicts (SPMD) and

  * ``build``  tokenises and counts the rank's doc range [r n / W, (r + 1) n / W) only, with corpus-wide vocabulary, idf
    and avgdl (distributed.build_sharded_host_index: bit-equal to the single-process arrays), uploads it with
    ``doc_base`` = the range's first row and installs corpus-wide score bounds (distributed.global_term_bounds);
  * ``search_arrays``  scores the batch on the shard, exchanges the packed per-shard top-k over RCCL and merges them
    exactly (distributed.ShardedSearcher) -- every rank gets the rows the single-GPU index returns.
"""
from __future__ import annotations

import copy
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from .boost import boost_deep  # beside collapse_deep: the same search_fn contract
from .index import DeviceIndex, HostIndex, build_host_index, deep_reduce, encode_queries, parse_operators, pool_depth, score_host_batch, search_host_batch, tokenize


class SparseBackend:
    def __init__(self, device: Optional[str], tile_log2: int, group=None, searcher_factory=None, sharded: Optional[bool] = None,
                 one_copy: bool = True):
        # searcher_factory(host_index, doc_base, mode, k1, b, group) -> ShardedSearcher on CPU tensors: TEST hook that puts
        # another scorer behind the sharding protocol (the gloo tests inject the CPU oracle).  The product never sets it:
        # without it every search runs on the HIP engine or raises.
        # sharded: None = shard iff the process is a rank of a group of more than one rank; True = take the sharded path even in
        # a group of ONE rank (the whole exchange runs -- RCCL collectives, packed merge -- on one GPU: rehearsals and tests)
        # one_copy (default): only the compact copy of the postings stays resident (DeviceIndex.drop_canonical: -56 % index memory
        # on fp32 values, and the tier-2 kernel moves fewer bytes: C4 -2.5 %, C5 -4 % per batch); False keeps the canonical
        # blocks too, which a search with another unit than the built one (set_opts) or a shard-file save needs
        self.one_copy = bool(one_copy)
        self.group = group
        self._searcher_factory = searcher_factory
        self._force_sharded = bool(sharded)
        if device is None:  # one process per GPU: the launcher's LOCAL_RANK picks the card
            device = f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}" if self.world() > 1 else "cuda:0"
        self.device = device
        self.tile_log2 = tile_log2
        self.host: Optional[HostIndex] = None
        self.dev: Optional[DeviceIndex] = None
        self.searcher = None
        self.doc_base = 0
        self.n_docs_total = 0
        self._doc_lengths_all = None
        self._fields = None        # set_fields: the docs' metadata columns on the host (fields.HostColumn by name) ...
        self._rank_model = None    # set_rank_model: (ltr.ForestModel, feature names)
        self._field_table = None   # ... and on the device, uploaded by the first call that filters with them
        self._rows = None          # _row_table
        self._forward = None       # enable_feedback: the doc-major forward index (feedback.ForwardIndex) and its term gains
        self._fb_gain = None
        self._fb_term_weight = "rm"
        self._words = None         # expand_queries: term id -> word

    def world(self) -> int:
        try:
            import torch.distributed as dist
        except ImportError:  # pragma: no cover
            return 1
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def sharded(self) -> bool:
        if self._force_sharded:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()):
                raise ValueError("sharded=True needs an initialised torch.distributed process group")
            return True
        return self.world() > 1

    @property
    def doc_lengths(self):
        if self._doc_lengths_all is not None:
            return self._doc_lengths_all
        return self.host.doc_lengths if self.host is not None else None

    # -- build ------------------------------------------------------------------------------------------
    def build(self, corpus, idf_kind: str = "bm25") -> HostIndex:
        self._drop_field_table()
        self._fields = None  # columns are aligned with the docs of one build
        if self.sharded():
            from .distributed import build_sharded_host_index
            self.host, self.doc_base, self.n_docs_total, self._doc_lengths_all = build_sharded_host_index(corpus, idf_kind, self.group)
        else:
            self.set_host(build_host_index(corpus, idf_kind=idf_kind))
        return self.host

    def set_host(self, host: HostIndex) -> None:
        """A complete host index (built here or read from the .npz cache): the one-shard case."""
        if self.sharded():
            raise ValueError("a pre-built whole-corpus index cannot be adopted by a sharded group: build it from the corpus")
        self._drop_field_table()
        self._fields = None
        self.host, self.doc_base, self.n_docs_total, self._doc_lengths_all = host, 0, host.n_docs, None

    def upload(self, mode: str, k1: float, b: float) -> None:
        self.close()
        h = self.host
        if self.sharded() and self._searcher_factory is not None:
            self.searcher = self._searcher_factory(h, self.doc_base, mode, k1, b, self.group)
            return
        if mode == "bm25":
            self.dev = DeviceIndex.from_host_index(h, k1=k1, b=b, device=self.device, tile_log2=self.tile_log2, doc_base=self.doc_base,
                                                   keep_canonical=not self.one_copy)
        else:
            self.dev = DeviceIndex.from_csr(h.indptr, h.indices, h.data, h.idf, mode="dot", device=self.device,
                                            tile_log2=self.tile_log2, doc_base=self.doc_base, keep_canonical=not self.one_copy)
        if self.sharded():
            from .distributed import ShardedSearcher, global_term_bounds
            global_term_bounds(self.dev, self.group)  # corpus-wide thresholds; the search stays exact
            self.searcher = ShardedSearcher.for_device_index(self.dev, self.group)
            self.searcher.force_exchange = self._force_sharded

    # -- search -----------------------------------------------------------------------------------------
    def _batch_device(self):
        """The device the batches go to: the index's, or the CPU for a test searcher (CPU tensors, no synchronisation)."""
        import torch
        return self.dev.device if self.dev is not None else torch.device("cpu")

    def search_arrays(self, q_ptr, q_term, q_weight, k: int):
        """Host CSR batch -> host rows (doc i32[nq, k] GLOBAL row ids, score f32[nq, k], count i32[nq]); any k >= 1."""
        if self.searcher is None:
            return self.dev.search(q_ptr, q_term, q_weight, k)
        return search_host_batch(self.searcher.search, q_ptr, q_term, q_weight, k, self.host.vocab_size, self._batch_device(),
                                 wait=self.searcher.wait)

    def score_arrays(self, q_ptr, q_term, q_weight, cand_doc, cand_count=None) -> np.ndarray:
        """Host CSR batch + host candidate block (cand_doc int[nq, m] GLOBAL row ids, cand_count int[nq] or None) -> the exact
        scores f32[nq, m] (``srx_score_docs``): on the one shard, or scored on every shard and summed
        (distributed.ShardedSearcher.score_docs)."""
        if self.searcher is None:
            return self.dev.score_docs(q_ptr, q_term, q_weight, cand_doc, cand_count)
        return score_host_batch(self.searcher.score_docs, q_ptr, q_term, q_weight, cand_doc, cand_count, self.host.vocab_size,
                                self._batch_device())

    def to_dict(self, idx: np.ndarray, sc: np.ndarray) -> Dict[str, float]:
        """Ranked rows -> {doc_id: score}, ``score > 0`` only (retrieval.py:292-296)."""
        ids = self.host.doc_ids
        return {ids[int(i)]: float(s) for i, s in zip(idx, sc) if s > 0}

    def filter_spec(self, queries, allowed_docs=None, excluded_docs=None, must_terms=None, any_terms=None, must_not_terms=None, where=None,
                    call: str = "search"):
        """The filter keywords of one API call as one spec (``.row_of_qid``, ``.on_device(index)``), or None when none of them
        constrains a query of ``queries``: :func:`doc_filter_spec` over this index's doc ids, then :func:`term_filter_spec` over
        its vocabulary (bound to its device index), then :func:`field_filter_spec` over the columns of :meth:`set_fields`, each
        with what came before as its base.  ValueError: a malformed keyword, term keywords without an index, ``where`` without
        fields (the message names ``call``); a sharded index refuses every kind that constrains a query."""
        spec = None
        if allowed_docs is not None or excluded_docs is not None:
            self._refuse_sharded("allowed_docs / excluded_docs need")
            spec = doc_filter_spec(self._row_table().row_of, queries, allowed_docs, excluded_docs)
        if not (must_terms is None and any_terms is None and must_not_terms is None):
            if self.host is None:
                raise ValueError("term constraints need the sparse index: build it first")
            terms = term_filter_spec(self.host.vocabulary, queries, must_terms, any_terms, must_not_terms)
            if terms is not None:  # else: empty lists, or operators=True on texts without operators
                self._refuse_sharded("must_terms / any_terms / must_not_terms need")
                spec = terms.with_base(spec, queries)
                spec.sparse = lambda: self.dev
        if where is not None:
            self._need_fields(call, "where=...")
            flds = field_filter_spec(self._fields, queries, where)
            if flds is not None:
                self._refuse_sharded("where= needs")
                spec = flds.with_base(spec, queries)
                spec.table = self.field_table
        return spec

    def _refuse_sharded(self, what_needs: str) -> None:
        if self.sharded():
            raise ValueError(f"{what_needs} the whole index on one GPU (a sharded search takes no doc filter)")

    def _need_fields(self, call: str, what: str, reason: Optional[str] = None) -> None:
        """ValueError unless :meth:`set_fields` was called (``what``: the message's brackets) and, given a ``reason`` (its parenthesis), the index is on one GPU"""
        if self._fields is None:
            raise ValueError(f"{call}({what}) needs the docs' fields: call set_doc_fields() first")
        if reason is not None and self.sharded():
            raise ValueError(f"{call} needs the whole index on one GPU ({reason})")

    def _row_table(self) -> "RowOfIds":
        """doc id -> row of this index's doc ids, kept between calls"""
        if self._rows is None or self._rows.ids is not self.host.doc_ids:
            self._rows = RowOfIds(self.host.doc_ids)
        return self._rows

    def set_fields(self, columns) -> None:
        """The docs' metadata columns (``fields.FieldTable.from_columns`` takes the same dict), row i = the i-th doc of the built
        index.  Kept on the host; the first ``where=`` call uploads them.  ValueError: no index, a length that is not the index's."""
        from .fields import host_columns
        if self.host is None:
            raise ValueError("the docs' fields are aligned with the index: build it first")
        cols = host_columns(columns)
        n = len(next(iter(cols.values())))
        if n != self.host.n_docs:
            raise ValueError(f"the columns have {n} entries, the index {self.host.n_docs} docs: one entry per doc, in the order of the corpus")
        self._drop_field_table()
        self._fields = cols

    def _drop_field_table(self) -> None:
        if self._field_table is not None:
            self._field_table.close()
            self._field_table = None

    def field_table(self):
        """The columns of :meth:`set_fields` on this backend's device (uploaded once)"""
        from .fields import FieldTable
        if self._field_table is None:
            self._field_table = FieldTable.from_columns(self._fields, device=self.dev.device if self.dev is not None else self.device, doc_base=self.doc_base)
        return self._field_table

    def collapse_spec(self, by, per_group=1, nulls="own", depth=None, top_k: int = 10, call: str = "search") -> Optional["CollapseSpec"]:
        """The collapse keywords of one API call (``collapse_by``, ``per_group``, ``collapse_nulls``, ``collapse_depth``) as a
        :class:`CollapseSpec`, or None when ``by`` is None (the other three are then not looked at).  ValueError: a sharded index,
        no fields (the message names ``call``), what :func:`~.fields.check_collapse_args` refuses, ``top_k`` above the engine's
        list depth, a depth below 1."""
        if by is None:
            return None
        from . import _capi
        from .fields import check_collapse_args
        self._need_fields(call, "collapse_by=...")
        check_collapse_args(self._fields, by, per_group, nulls)
        if int(top_k) > _capi.SRX_MAX_K:
            raise ValueError(f"{call}(collapse_by=...) returns at most {_capi.SRX_MAX_K} rows per query, got top_k={top_k}")
        if depth is not None and int(depth) < 1:
            raise ValueError(f"collapse_depth must be >= 1, got {depth}")
        self._refuse_sharded("collapse_by= needs")
        return CollapseSpec(by, int(per_group), nulls, None if depth is None else int(depth))

    def result_lists(self, results, call: str, cap: Optional[int] = None, scored: bool = True):
        """``results`` = ``{qid: {doc_id: score}}`` (or ``search_by_vector``'s lists of ``{"doc_id", "score"}`` dicts) as one candidate
        block: ``(pairs = {qid: [(doc_id, score)]}, live, cand_doc, cand_count, score)`` -- the middle three as :func:`candidate_block`
        returns them, with ``doc_base`` added (GLOBAL ids); ``score`` f32 of cand_doc's shape, 0 behind a list's end (None unless
        ``scored``).  ValueError: a list deeper than ``cap`` (the message names ``call``), then an unknown doc id."""
        as_pairs = lambda row: [(r["doc_id"], r["score"] if scored else None) for r in row] if isinstance(row, (list, tuple)) else list(row.items())
        pairs = {qid: as_pairs(row) for qid, row in results.items()}
        deepest = max((len(p) for p in pairs.values()), default=0)
        if cap is not None and deepest > cap:
            raise ValueError(f"{call} takes lists of at most {cap} docs, got {deepest} (no silent truncation)")
        _, live, cand_doc, cand_count = self.candidate_block(results, {qid: [d for d, _ in p] for qid, p in pairs.items()})
        score = np.zeros(cand_doc.shape, dtype=np.float32) if scored else None
        for i, (qid, _, _) in enumerate(live if scored else ()):
            score[i, : len(pairs[qid])] = [s for _, s in pairs[qid]]
        return pairs, live, cand_doc + np.int32(self.doc_base), cand_count, score

    def collapse_results(self, results, by, top_k=10, per_group=1, nulls="own", call: str = "collapse"):
        """Result lists collapsed by the field ``by`` (``srx_collapse_topk``): what ``RetrievalService.collapse`` documents.  One
        upload, one launch, one copy back; list-shaped rows come back list-shaped, ``{}`` stays ``{}``."""
        from . import _capi
        from .fields import check_collapse_args
        self._need_fields(call, "...")
        check_collapse_args(self._fields, by, per_group, nulls)
        self._need_fields(call, "...", "the columns are shard-local")
        if not results:
            return {}
        _, live, cand_doc, cand_count, _ = self.result_lists(results, call, scored=False)
        m = int(cand_doc.shape[1])
        if m > _capi.SRX_COLLAPSE_MAX_M:  # its own line: this door names an unknown doc id first, and words the depth its way
            raise ValueError(f"{call} takes lists of at most {_capi.SRX_COLLAPSE_MAX_M} docs, got one of {m} (no silent truncation)")
        as_rows = {qid: isinstance(row, (list, tuple)) for qid, row in results.items()}
        out = {qid: ([] if as_rows[qid] else {}) for qid in results}
        if not live or int(top_k) <= 0:
            return out
        score = np.zeros(cand_doc.shape, dtype=np.float32)  # never looked at: the values come back by position
        _, _, count, pos = self.field_table().collapse(by, cand_doc, score, cand_count, min(int(top_k), m), per_group, nulls, want_pos=True)
        for i, (qid, _, cands) in enumerate(live):
            kept = [int(pos[i, j]) for j in range(int(count[i]))]
            out[qid] = [results[qid][p] for p in kept] if as_rows[qid] else {cands[p]: results[qid][cands[p]] for p in kept}
        return out

    # -- boosts by field values (include/boost/sparse_rx_boost.h) ---------------------------------------------------------------
    boost_page = 1024  # rows per page of the exact boosted search (the engine's list depth; a test may lower it)

    def boost_spec(self, boost, depth=None, top_k: int = 10, call: str = "search", collapse=None, exact: bool = True):
        """The boost keywords of one API call (``boost``, ``boost_depth``) as a :class:`~.boost.BoostResolver` with a ``depth``
        attribute, or None when ``boost`` is None.  ``exact``: the call is an exact door (:func:`~.boost.boost_deep`), which has
        no bound for ``boost_mode`` "replace" nor for a factor that can be negative under "multiply".  ValueError: no fields (the
        message names ``call``), a sharded index, what the resolver refuses (an unknown or set column among it), ``top_k`` above
        the engine's list depth, a depth below 1, ``collapse_by=`` in the same call."""
        if boost is None:
            return None
        from . import _capi
        from .boost import BoostResolver
        self._need_fields(call, "boost=...")
        self._refuse_sharded("boost= needs")
        res = boost if isinstance(boost, BoostResolver) else BoostResolver(self._fields, boost)
        if int(top_k) > _capi.SRX_MAX_K:
            raise ValueError(f"{call}(boost=...) returns at most {_capi.SRX_MAX_K} rows per query, got top_k={top_k}")
        if depth is not None and int(depth) < 1:
            raise ValueError(f"boost_depth must be >= 1, got {depth}")
        if collapse is not None:
            raise ValueError(f"{call}: boost= and collapse_by= do not combine in one call (chain collapse() over the boosted result)")
        if exact:
            if res.boost_mode_name == "replace":
                raise ValueError(f"{call}(boost=...): boost_mode \"replace\" drops the relevance score, so no page of the ranking bounds the "
                                 "rest (search_sorted orders by a field alone; boost_results reorders a given list)")
            if res.boost_mode_name == "multiply" and not float(res.F_lo) >= 0.0:
                raise ValueError(f"{call}(boost=...): under boost_mode \"multiply\" the factor must not be negative (F_lo = {float(res.F_lo)!r})")
        res.depth = None if depth is None else int(depth)
        return res

    def boost_results(self, results, boost, top_k=None, call: str = "boost_results"):
        """Result lists re-scored and re-ranked by a boost (``srx_boost_topk``): ``results`` = ``{qid: {doc_id: score}}`` as any
        search returns it (or ``search_by_vector``'s lists of ``{"doc_id", "score"}`` dicts) -> ``{qid: {doc_id: new score}}``,
        the first ``top_k`` (None: all) by (new score descending, corpus order).  It is relative to THE LISTS GIVEN; every
        ``boost_mode`` is allowed.  One upload, one launch, one copy back.  ValueError: a list deeper than 2048, an unknown doc
        id, and what :meth:`boost_spec` refuses of ``boost``."""
        from . import _capi
        from .boost import BoostFn
        res = self.boost_spec(boost, None, 1, call, exact=False)
        if res is None:
            raise ValueError(f"{call} needs a boost")
        return self._rerank_lists(results, call, _capi.SRX_BOOST_MAX_M, top_k, self.field_table,
                                  lambda table, k, upload, pairs, live: BoostFn(table, res)(*upload(), k, want_pos=True)[1:])

    def _rerank_lists(self, results, call: str, cap: int, top_k, table, run, new_scores: bool = True):
        """The door of the list operators that reorder: ``results`` (what :meth:`result_lists` takes, at most ``cap`` docs a list)
        -> ``{qid: {doc_id: score}}``, the first ``top_k`` (None: all) in the order ``run`` gives.  ``table()`` -> the field table
        (made only when a list has a doc); ``run(table, k, upload, pairs, live) -> (score [nq, k] | None, count [nq] or [nq, c] with
        the count in column 0, pos [nq, k])`` launches once on ``upload()``, the (doc, score, count) triple on the table's device,
        k = min(top_k, the deepest list).  The scores returned are ``run``'s (``new_scores``) or the ones given.  One upload of the
        triple, one copy back.  ValueError: ``top_k`` below 1, then what :meth:`result_lists` refuses."""
        if top_k is not None and int(top_k) < 1:
            raise ValueError(f"top_k must be >= 1, got {top_k}")
        out = {qid: {} for qid in (results or {})}
        if not results:
            return out
        pairs, live, cand_doc, cand_count, score = self.result_lists(results, call, cap)
        if not live:
            return out
        import torch
        table = table()
        m = cand_doc.shape[1]
        k = m if top_k is None else min(int(top_k), m)
        ns, cnt, pos = run(table, k, lambda: tuple(torch.as_tensor(a, device=table.device) for a in (cand_doc, score, cand_count)), pairs, live)
        block = torch.cat([pos, cnt.reshape(len(live), -1)] + ([ns.view(torch.int32)] if new_scores else []), dim=1).cpu().numpy()
        for i, (qid, _, _) in enumerate(live):
            n = int(block[i, k])
            given = [pairs[qid][int(p)] for p in block[i, :n]]
            if new_scores:  # the last k columns
                new = block[i, block.shape[1] - k:][:n].copy().view(np.float32)
                given = [(d, float(v)) for (d, _), v in zip(given, new)]
            out[qid] = dict(given)
        return out

    # -- reranking with a tree-ensemble model (include/ltr/sparse_rx_ltr.h) -------------------------------------------------------
    def set_rank_model(self, model, features) -> None:
        """The model and the feature list of the ``rank_model=True`` keyword and of :meth:`rerank_model_results`: a
        :class:`~.ltr.ForestModel` and what :func:`~.ltr.resolve_features` takes (plus "sparse_score" / "dense_score", which only a
        hybrid search fills).  The names are resolved against the docs' fields at every call: they may be set later."""
        from .ltr import HYBRID_FEATURES, resolve_features
        named = isinstance(features, (list, tuple)) and any(isinstance(f, str) and f in HYBRID_FEATURES for f in features)
        resolve_features(self._fields, features, model, HYBRID_FEATURES if named else (), any_column=self._fields is None)
        self._rank_model = (model, list(features))

    def rank_table(self):
        """:meth:`field_table`, or a table without columns when no fields are set (a model over scores, ranks and extras)"""
        if self._fields is not None:
            return self.field_table()
        from .fields import FieldTable
        return FieldTable.without_columns(self.n_docs_total, device=self.dev.device if self.dev is not None else self.device, doc_base=self.doc_base)

    def rank_spec(self, rank_model, rank_pool=None, top_k: int = 10, call: str = "search", boost=None, hybrid: bool = False):
        """The model keywords of one API call (``rank_model``, ``rank_pool``) as a :class:`~.ltr.RankFn` with a ``pool`` attribute
        (``rank_pool`` in 1 .. 1024, default ``min(max(4 * top_k, 100), 1024, n_docs)``), or None when ``rank_model`` is false.
        ValueError: no :meth:`set_rank_model`, a sharded index, ``boost=`` in the same call, a feature that names a column without
        the docs' fields, an unknown or set column, "sparse_score" / "dense_score" unless ``hybrid``, an ``("extra", i)`` feature when
        ``hybrid`` (such a search has no extras to give), a pool above 1 024."""
        if not rank_model:  # rank_pool is then not looked at, like boost_pool without boost
            return None
        from .ltr import HYBRID_FEATURES, RankFn
        if getattr(self, "_rank_model", None) is None:
            raise ValueError(f"{call}(rank_model=True) needs a model: call set_rank_model() first")
        self._refuse_sharded("rank_model= needs")
        if boost is not None:
            raise ValueError(f"{call}: rank_model= and boost= do not combine in one call (chain boost_results() over the reranked result)")
        model, features = self._rank_model
        if self._fields is None and any(isinstance(f, str) and f not in ("score", "rank", *HYBRID_FEATURES) for f in features):
            self._need_fields(call, "rank_model=True")
        if hybrid and any(isinstance(f, (tuple, list)) for f in features):
            raise ValueError(f"{call}(rank_model=True) cannot fill (\"extra\", i) features: a hybrid search supplies \"sparse_score\" and "
                             "\"dense_score\" only (chain rerank_model(results, top_k, extra=...) over its result)")
        pool = collapse_pool_depth(top_k, rank_pool, self.n_docs_total, "rank_pool")
        named = HYBRID_FEATURES if hybrid and any(isinstance(f, str) and f in HYBRID_FEATURES for f in features) else ()
        fn = RankFn(self.rank_table, model, features, named, columns=self._fields if self._fields is not None else {})
        fn.pool = pool
        return fn

    def rerank_model_results(self, results, top_k=None, extra=None, mode: str = "replace", call: str = "rerank_model"):
        """Result lists re-scored and re-ranked by the model of :meth:`set_rank_model` (``srx_ltr_topk``): ``results`` =
        ``{qid: {doc_id: score}}`` as any search returns it (or ``search_by_vector``'s lists of ``{"doc_id", "score"}`` dicts) ->
        ``{qid: {doc_id: model score}}``, the first ``top_k`` (None: all) by (new score descending, corpus order).  The feature
        "score" is the value given, "rank" the position in the list given.  ``extra``: ``{qid: {doc_id: sequence of floats}}``, the
        values of the ``("extra", i)`` features (a doc or a value left out is missing: NaN).  One upload, one launch, one copy
        back.  ValueError: a list deeper than 2048, an unknown doc id, what :meth:`rank_spec` refuses."""
        from . import _capi
        from .ltr import check_mode
        fn = self.rank_spec(True, None, 1, call)
        check_mode(mode)

        def run(table, k, upload, pairs, live):
            import torch
            from .ltr import resolve_features
            n_extra = resolve_features(table.columns, fn.features, fn.model)[2]
            plane = None
            if n_extra:
                host = np.full((len(live), max(len(pairs[qid]) for qid, _, _ in live), n_extra), np.nan, dtype=np.float32)
                for i, (qid, _, _) in enumerate(live):
                    row = (extra or {}).get(qid, {})
                    for c, (doc_id, _) in enumerate(pairs[qid]):
                        vals = np.asarray(row.get(doc_id, ()), dtype=np.float32).reshape(-1)[:n_extra]
                        host[i, c, : len(vals)] = vals
                plane = torch.as_tensor(host, device=table.device)
            return fn(*upload(), k, extra=plane, mode=mode, want_pos=True)[1:]

        return self._rerank_lists(results, call, _capi.SRX_LTR_MAX_M, top_k, lambda: fn.table, run)

    def facet_specs(self, fields, call: str = "facets"):
        """``fields`` of a facet door -- one name, a sequence of names, or a dict name -> binning spec (None: the column's own
        bins) -- as ``{name: fields.FacetSpec}`` (:func:`~.fields.check_facet_args`).  ValueError: no :meth:`set_fields` (the
        message names ``call``), a sharded index, no field, an unknown field, a spec that does not fit."""
        from .fields import check_facet_args
        self._need_fields(call, "...", "the columns and the filter rows are shard-local")
        if isinstance(fields, str):
            fields = [fields]
        given = dict(fields) if isinstance(fields, dict) else {name: None for name in (fields or ())}
        if not given:
            raise ValueError(f"{call} needs at least one field")
        return {name: check_facet_args(self._fields, name, spec) for name, spec in given.items()}

    def match_rows(self, queries, match="any", allowed_docs=None, excluded_docs=None, must_terms=None, any_terms=None, must_not_terms=None,
                   where=None, call: str = "facets"):
        """The doc sets of :meth:`facets` and :meth:`search_sorted` as filter rows: ``(live, filter, rows, row_of)`` -- ``live`` the
        queries that have a set at all (under match "any" / "all" a text without a token has none), ``filter`` the
        :class:`~.filter.DocFilter` of the :meth:`filter_spec` chain with the query's own text joined to its ``any`` ("any") or
        ``must`` ("all") list, or None when nothing constrains a query (every doc), ``rows`` the distinct filter rows in use and
        ``row_of`` qid -> its place in ``rows``.  ValueError: a bad ``match``, match="any" with ``any_terms=``, no index, and what
        :meth:`filter_spec` refuses."""
        check_match(match, any_terms, call)
        if self.host is None or self.dev is None:
            raise ValueError(f"{call} needs the sparse index: build it first")
        empty = {qid for qid, text in queries.items() if match is not None and not (isinstance(text, str) and tokenize(text))}
        live = {qid: text for qid, text in queries.items() if qid not in empty}
        if not live:
            return live, None, [0], {}
        if match is not None:
            given = must_terms if match == "all" else None
            if isinstance(given, (str, bytes)):
                raise ValueError("must_terms must be a sequence of strings or a dict qid -> sequence, not one string")
            own = {qid: (list(given.get(qid, ())) if isinstance(given, dict) else list(given or ())) + [text] for qid, text in live.items()}
            if match == "all":
                must_terms = own
            else:
                any_terms = own
        spec = self.filter_spec(live, allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, where, call)
        if spec is None:
            return live, None, [0], {qid: 0 for qid in live}
        flt = spec.on_device(self.dev)
        rows = sorted({spec.row_of_qid[qid] for qid in live})
        return live, flt, rows, {qid: rows.index(spec.row_of_qid[qid]) for qid in live}

    def facets(self, queries, fields, match="any", allowed_docs=None, excluded_docs=None, must_terms=None, any_terms=None, must_not_terms=None,
               where=None, top=None, call: str = "facets"):
        """Facet counts per query (``srx_facet_counts``, include/sparse_rx_facets.h): ``{qid: {field: {"counts": {value: n},
        "missing": n, "other": n, "total": n}}}`` over each query's doc set.  The set is built as one row per distinct
        constraint with the :meth:`filter_spec` chain (doc keywords, then term rows, then field rows); ``match`` adds the query's
        own text to it: "any" -- the docs that hold at least one of its known terms (the text joins the ``any`` list; giving
        ``any_terms`` too is a ValueError), "all" -- the docs that hold every term (the text joins the ``must`` list), None --
        the text is ignored.  Under "any" / "all" a text without a token has the empty set.  One ``facet_device`` per field over
        the same rows, one copy back.  ``top``: keep the ``top`` largest bins of every field (:func:`facet_dict`)."""
        specs = self.facet_specs(fields, call)
        check_match(match, any_terms, call)  # before `top`, as ever: the ValueError of a call with two bad keywords stays the same
        if top is not None and int(top) < 1:
            raise ValueError(f"top must be >= 1, got {top}")
        out = {qid: {name: facet_dict(fs, None, (0, 0, 0), top) for name, fs in specs.items()} for qid in queries}
        live, flt, rows, row_of = self.match_rows(queries, match, allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, where, call)
        if not live:
            return out
        import torch
        table = self.field_table()
        qf = None if flt is None else torch.as_tensor(np.asarray(rows, dtype=np.int32), device=table.device)
        parts = []
        for name, fs in specs.items():
            parts.extend(table.facet_device(name, fs, filter=flt, q_filter=qf, n_rows=len(rows)))
        block = torch.cat(parts, dim=1).cpu().numpy()  # the one copy back
        at = 0
        for name, fs in specs.items():
            counts, extra = block[:, at: at + fs.n_bins], block[:, at + fs.n_bins: at + fs.n_bins + 3]
            at += fs.n_bins + 3
            for qid in live:
                out[qid][name] = facet_dict(fs, counts[row_of[qid]], extra[row_of[qid]], top)
        return out

    def facets_of(self, results, fields, top=None, call: str = "facets_of"):
        """Facet counts over the docs of result lists (``srx_facet_counts_lists``): ``results`` = ``{qid: {doc_id: score}}`` as any
        search returns it (or ``search_by_vector``'s lists of ``{"doc_id", "score"}`` dicts) -> the dict of :meth:`facets`.  One
        upload of the lists, one launch per field, one copy back.  ValueError: an unknown doc id, and what :meth:`facet_specs`
        refuses."""
        specs = self.facet_specs(fields, call)
        if top is not None and int(top) < 1:
            raise ValueError(f"top must be >= 1, got {top}")
        out = {qid: {name: facet_dict(fs, None, (0, 0, 0), top) for name, fs in specs.items()} for qid in (results or {})}
        if not results:
            return out
        _, live, cand_doc, cand_count, _ = self.result_lists(results, call, scored=False)
        if not live:
            return out
        import torch
        table = self.field_table()
        doc = torch.as_tensor(cand_doc, device=table.device)
        cnt = torch.as_tensor(cand_count, device=table.device)
        parts = []
        for name, fs in specs.items():
            parts.extend(table.facet_lists_device(name, doc, cnt, fs))
        block = torch.cat(parts, dim=1).cpu().numpy()
        at = 0
        for name, fs in specs.items():
            for i, (qid, _, _) in enumerate(live):
                out[qid][name] = facet_dict(fs, block[i, at: at + fs.n_bins], block[i, at + fs.n_bins: at + fs.n_bins + 3], top)
            at += fs.n_bins + 3
        return out

    # -- order by a field (include/order/sparse_rx_order.h) -------------------------------------------------------------------
    def _order_column(self, by, order, nulls, call: str):
        """The column ``by`` of :meth:`set_fields` for an ordering door; ValueError: no fields (the message names ``call``), a sharded
        index, and what :func:`~.fields.check_order_args` refuses."""
        from .fields import check_order_args
        self._need_fields(call, "...", "the columns and the filter rows are shard-local")
        check_order_args(self._fields, by, order, nulls)
        return self._fields[by]

    def search_sorted(self, queries, by, order="desc", top_k=10, match="any", nulls="last", allowed_docs=None, excluded_docs=None, must_terms=None,
                      any_terms=None, must_not_terms=None, where=None, call: str = "search_sorted"):
        """The first ``top_k`` docs of each query's doc set in the order of the field ``by`` instead of relevance
        (``srx_order_topk``, include/order/sparse_rx_order.h): ``{qid: {doc_id: value}}`` in rank order.  The doc set is the one of
        :meth:`facets` (:meth:`match_rows`: the same ``match`` and filter keywords; under "any" / "all" a text without a token gives
        ``{}``).  ``order`` "asc" / "desc"; docs with equal values come in corpus order (ascending row), in both directions.
        ``nulls``: docs without a value come "last", "first", or "drop" out.  The value is a Python int (int32 / int64), bool, float
        (float32), the dictionary string of a category column (ordered as strings: its codes are the places in the sorted
        dictionary) or None for a doc without one.  ``top_k`` above 1024 pages with the cursor until ``top_k`` docs or the set is
        exhausted.  ValueError: no :meth:`set_fields`, a sharded index, an unknown or set column, a bad keyword."""
        from . import _capi
        from .fields import order_has_value, order_values
        col = self._order_column(by, order, nulls, call)
        top_k = int(top_k)
        if top_k < 1:
            raise ValueError(f"top_k must be >= 1, got {top_k}")
        out = {qid: {} for qid in queries}
        live, flt, rows, row_of = self.match_rows(queries, match, allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, where, call)
        if not live:
            return out
        import torch
        table = self.field_table()
        qf = None if flt is None else torch.as_tensor(np.asarray(rows, dtype=np.int32), device=table.device)
        ids, base = self.host.doc_ids, self.doc_base
        got = [[] for _ in rows]  # per row: (doc row, value) in rank order
        open_rows, after = list(range(len(rows))), None
        while open_rows:  # one page of at most 1024 per round, for the rows that may go on
            k = min(top_k - min(len(got[r]) for r in open_rows), _capi.SRX_MAX_K)
            sel = None if qf is None else qf[torch.as_tensor(open_rows, device=table.device)]
            doc, key, extra = table.top_by_device(by, k, order, nulls, filter=flt, q_filter=sel, n_rows=len(open_rows), after=after)
            doc, key, extra = doc.cpu().numpy(), key.cpu().numpy(), extra.cpu().numpy()
            has = order_has_value(extra, nulls, k)
            still, cursor = [], []
            for i, r in enumerate(open_rows):
                n = int(extra[i, 0])
                take = min(n, top_k - len(got[r]))
                got[r].extend(zip((int(d) - base for d in doc[i, :take]), order_values(col, key[i, :take], has[i, :take])))
                if n == k and len(got[r]) < top_k:  # a full page and more wanted: the set may go on behind its last doc
                    still.append(r)
                    cursor.append(int(doc[i, n - 1]))
            open_rows, after = still, torch.as_tensor(np.asarray(cursor, dtype=np.int32), device=table.device)
        for qid in live:
            out[qid] = {ids[d]: v for d, v in got[row_of[qid]]}
        return out

    def sort_results(self, results, by, order="desc", nulls="last", top_k=None, call: str = "sort_results"):
        """Result lists reordered by the field ``by`` (``srx_order_lists``): ``results`` = ``{qid: {doc_id: score}}`` as any search
        returns it (or ``search_by_vector``'s lists of ``{"doc_id", "score"}`` dicts) -> ``{qid: {doc_id: score}}`` with the
        original scores, the first ``top_k`` (None: all) in the order of the value; docs with equal values, and docs without one,
        keep the order they came in.  One upload, one launch, one copy back.  ValueError: a list deeper than 2048, an unknown doc
        id, and what :meth:`search_sorted` refuses of ``by`` / ``order`` / ``nulls``."""
        from . import _capi
        self._order_column(by, order, nulls, call)
        return self._rerank_lists(results, call, _capi.SRX_ORDER_MAX_M, top_k, self.field_table,
                                  lambda table, k, upload, pairs, live: (None,) + table.sort_lists_device(by, *upload(), k, order, nulls, want_pos=True)[3:],
                                  new_scores=False)

    # -- relevance feedback (include/ext/sparse_rx_feedback.h) ----------------------------------------------------------------
    def enable_feedback(self, mode: str = "bm25") -> None:
        """Build the doc-major forward index (:class:`~.feedback.ForwardIndex`: 8 bytes per posting + 12 per doc) from the host
        CSR, on the device of the index.  ``mode`` "bm25": rows hold tf, contributions are tf / doc_len (RM) and a term's gain is
        ``max(idf, 0)`` -- a term with a non-positive idf is never an expansion term; "dot": raw values and a gain of 1.
        :meth:`upload` and :meth:`close` drop it.  ValueError: no index, a sharded index."""
        from .feedback import ForwardIndex
        if self.host is None or self.dev is None:
            raise ValueError("enable_feedback() needs the sparse index: build it first")
        if self.sharded():
            raise ValueError("relevance feedback needs the whole index on one GPU (a forward index is shard-local, a query's feedback docs are not)")
        self._drop_forward()
        import torch
        h = self.host
        self._forward = ForwardIndex.from_csr(h.indptr, h.indices, h.data, h.idf, doc_lengths=h.doc_lengths if mode == "bm25" else None,
                                              device=self.dev.device, doc_base=self.doc_base)
        self._fb_gain = torch.clamp(torch.as_tensor(np.ascontiguousarray(h.idf, dtype=np.float32), device=self.dev.device), min=0.0) if mode == "bm25" else None
        self._fb_term_weight = "rm" if mode == "bm25" else "raw"

    def _drop_forward(self) -> None:
        if self._forward is not None:
            self._forward.close()
        self._forward = self._fb_gain = None

    def _need_forward(self, call: str, what: str):
        if self.sharded():
            raise ValueError(f"{call}({what}) needs the whole index on one GPU (a sharded index has no forward index)")
        if self._forward is None:
            raise ValueError(f"{call}({what}) needs the forward index: call enable_feedback() first")
        return self._forward

    def expand_spec(self, expand_docs, expand_terms=10, expand_weight=0.5, expand_by="score", call: str = "search") -> Optional["ExpandSpec"]:
        """The expansion keywords of one API call as an :class:`ExpandSpec`, or None when ``expand_docs`` is None (the other three
        are then not looked at).  ValueError: what :func:`~.feedback.check_expand_args` refuses, a sharded index, no
        :meth:`enable_feedback`."""
        if expand_docs is None:
            return None
        from .feedback import check_expand_args
        spec = ExpandSpec(*check_expand_args(expand_docs, expand_terms, expand_weight, expand_by))
        self._need_forward(call, "expand_docs=...")
        return spec

    def search_rows(self, q_ptr, q_term, q_weight, k: int, filter=None, q_filter=None, collapse=None, expand=None, boost=None):
        """Host CSR batch -> host rows (doc i32[nq, k] GLOBAL row ids, score f32[nq, k], count i32[nq]): the one route of the
        optional stages.  ``filter`` / ``q_filter``: a DocFilter and the host row numbers.  Without a staged keyword the call is
        :meth:`search_arrays` or, filtered, the index's ``search`` -- any k, nothing else runs.  Otherwise the batch goes to the
        device once and

          * ``expand`` (:class:`ExpandSpec`): a first pass ``min(expand.docs, n_docs)`` deep under the filter, never collapsed, then
            ``srx_feedback_expand`` with alpha = 1 - weight, beta = weight; its lists and the expanded batch stay on the device;
          * :meth:`_second_pass` searches the batch under the filter: collapsed (``collapse``, a :class:`CollapseSpec`), boosted
            (``boost``, a resolver of :meth:`boost_spec`), or plain."""
        if collapse is None and expand is None and boost is None:
            if filter is None:
                return self.search_arrays(q_ptr, q_term, q_weight, k)
            return self.dev.search(q_ptr, q_term, q_weight, k, filter=filter, q_filter=q_filter)
        import torch
        from .index import _batch_to_device, validate_query_batch
        validate_query_batch(q_ptr, q_term, q_weight, self.host.vocab_size)
        nq = len(q_ptr) - 1
        if nq == 0:
            return np.zeros((0, k), np.int32), np.zeros((0, k), np.float32), np.zeros(0, np.int32)
        flt = self._device_filter(filter, q_filter, nq)
        batch = _batch_to_device(torch, q_ptr, q_term, q_weight, self.dev.device)
        if expand is not None:
            d, s, c = self.dev.search_device(*batch, min(expand.docs, self.n_docs_total), **flt)
            batch = self._forward.expand_device(*batch, d, s, c, fb_docs=expand.docs, n_terms=expand.terms, alpha=1.0 - expand.weight,
                                                beta=expand.weight, doc_weight=expand.by, term_weight=self._fb_term_weight,
                                                term_gain=self._fb_gain)[:3]
        return self._second_pass(batch, k, filter, q_filter, collapse, boost, flt)

    def _device_filter(self, filter, q_filter, nq: int) -> dict:
        """The filter keywords of ``search_device``: none, or the DocFilter and its host row numbers, checked and uploaded"""
        from .filter import q_filter_to_device
        return {} if filter is None else {"filter": filter, "q_filter": q_filter_to_device(filter.for_index(self.dev), q_filter, nq)}

    def _second_pass(self, batch, k: int, filter=None, q_filter=None, collapse=None, boost=None, flt: Optional[dict] = None):
        """A batch on the device -> host rows, one copy back: the plain ``search_device``, :func:`collapse_deep` (``first`` =
        min(max(4 k, 64), 1024, n_docs), pages of 1 024) or :func:`~.boost.boost_deep` (pages of min(``boost_page``, 1 024), ``first``
        = min(max(4 k, 64), max(page, k), n_docs)) over it, under ``filter`` / ``q_filter`` (``flt``: their :meth:`_device_filter`,
        when the caller has it).  k > 1024 (never collapsed or boosted): the batch goes to the host once and takes the paged route
        of :meth:`~.index.DeviceIndex.search`."""
        import torch
        from . import _capi
        from .boost import BoostFn
        from .index import _to_host
        dev = self.dev
        if k > _capi.SRX_MAX_K:
            p = batch[0].cpu().numpy()
            n = int(p[-1])
            return dev.search(p, batch[1][:n].cpu().numpy(), batch[2][:n].cpu().numpy(), k, filter=filter, q_filter=q_filter)
        if flt is None:
            flt = self._device_filter(filter, q_filter, batch[0].numel() - 1)
        search_fn = lambda qp, qt, qw, kk, after=None: dev.search_device(qp, qt, qw, kk, after=after, **flt)
        if boost is not None:
            page = min(int(self.boost_page), _capi.SRX_MAX_K)
            out = boost_deep(search_fn, BoostFn(self.field_table(), boost), *batch, k, min(max(4 * k, 64), max(page, k), self.n_docs_total),
                             page=page, max_depth=boost.depth)
        elif collapse is not None:
            table = self.field_table()
            out = collapse_deep(search_fn, lambda d, s, c, kk: table.collapse_device(collapse.by, d, s, c, kk, collapse.per_group, collapse.nulls),
                                *batch, k, min(max(4 * k, 64), _capi.SRX_MAX_K, self.n_docs_total), page=_capi.SRX_MAX_K, max_depth=collapse.depth)
        else:
            out = dev.search_device(*batch, k, **flt)
        return _to_host(torch, dev.device, out)

    def _seed_block(self, lists, call: str, what: str):
        """{qid: sequence of doc ids} -> (qids, doc i32[nq, m] GLOBAL row ids padded with -1, count i32[nq]); at most 32 per qid"""
        from . import _capi
        row_of = self._row_table().row_of
        qids, rows = list(lists), []
        for qid in qids:
            ids = lists[qid]
            if isinstance(ids, (str, bytes)):
                raise ValueError(f"{what}[{qid!r}] must be a sequence of doc ids, not one string")
            try:
                rows.append([row_of[d] + self.doc_base for d in ids])
            except KeyError as e:
                raise ValueError(f"unknown doc id {e.args[0]!r} among the {what} of {qid!r}") from None
            if len(rows[-1]) > _capi.SRX_FEEDBACK_MAX_DOCS:
                raise ValueError(f"{call} takes at most {_capi.SRX_FEEDBACK_MAX_DOCS} {what} per query, got {len(rows[-1])} for {qid!r} (no silent truncation)")
        m = max((len(r) for r in rows), default=1) or 1
        doc = np.full((len(rows), m), -1, dtype=np.int32)
        for i, r in enumerate(rows):
            doc[i, : len(r)] = r
        return qids, doc, np.asarray([len(r) for r in rows], dtype=np.int32)

    def more_like_this(self, seeds, top_k: int = 10, terms: int = 25, include_seeds: bool = False, allowed_docs=None, excluded_docs=None,
                       must_terms=None, any_terms=None, must_not_terms=None, where=None, call: str = "more_like_this"):
        """``{qid: [doc_id, ...]}`` -> ``{qid: {doc_id: score}}``: the docs most like each query's seed docs.  The query is built
        on the GPU from the seeds alone -- empty input queries, the seeds as UNIFORM feedback docs, beta = 1: the ``terms`` terms
        that characterise them best, weights summing to 1 -- and searched with the seeds denied per query (``excluded_docs``
        machinery) unless ``include_seeds``.  The filter keywords are those of the searches.  ValueError: no
        :meth:`enable_feedback`, a sharded index, an unknown doc id, more than 32 seeds, ``terms`` outside 1..128."""
        import torch
        from .feedback import check_expand_args
        check_expand_args(1, terms, 1.0, "uniform")
        fwd = self._need_forward(call, "...")
        if isinstance(seeds, (str, bytes)) or not isinstance(seeds, dict):
            raise ValueError("seeds must be a dict qid -> sequence of doc ids")
        qids, doc, count = self._seed_block(seeds, call, "seeds")
        queries = {qid: "" for qid in qids}
        if not include_seeds:
            allowed_docs, excluded_docs = _without_seeds(seeds, qids, allowed_docs, excluded_docs)
        spec = self.filter_spec(queries, allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, where, call)
        out = {qid: {} for qid in qids}
        k_eff = min(int(top_k), self.n_docs_total)
        if not qids or k_eff <= 0:
            return out
        dev = self.dev
        nq = len(qids)
        qp = torch.zeros(nq + 1, dtype=torch.int32, device=dev.device)
        qt, qw = torch.empty(0, dtype=torch.int32, device=dev.device), torch.empty(0, dtype=torch.float32, device=dev.device)
        batch = fwd.expand_device(qp, qt, qw, torch.as_tensor(doc, device=dev.device), None, torch.as_tensor(count, device=dev.device),
                                  fb_docs=max(1, int(doc.shape[1])), n_terms=int(terms), alpha=0.0, beta=1.0, doc_weight="uniform",
                                  term_weight=self._fb_term_weight, term_gain=self._fb_gain)
        rows = None if spec is None else np.asarray([spec.row_of_qid[qid] for qid in qids], dtype=np.int32)
        docs, scores, counts = self._second_pass(batch[:3], k_eff, None if spec is None else spec.on_device(dev), rows)
        for i, qid in enumerate(qids):
            c = int(counts[i])
            out[qid] = self.to_dict(docs[i, :c].astype(np.int64), scores[i, :c])
        return out

    def expand_queries(self, queries, results, expand_terms=10, expand_weight=0.5, expand_by="score", order: str = "term", call: str = "expand_queries"):
        """What the queries are expanded to: ``queries`` {qid: text}, ``results`` {qid: {doc_id: score}} as a search returned
        them (the feedback docs, in dict order, at most 32 per query) -> ``{qid: {word: weight}}`` in ascending term id, the
        batch ``search(..., expand_docs=len(results[qid]))`` searches in its second pass.  A qid without results gets its
        normalised query."""
        from .feedback import check_expand_args
        _, n_terms, weight, by = check_expand_args(1, expand_terms, expand_weight, expand_by)
        fwd = self._need_forward(call, "...")
        lists = {qid: list((results or {}).get(qid, {}) or {}) for qid in queries}
        qids, doc, count = self._seed_block(lists, call, "results")
        if not qids:
            return {}
        score = np.zeros(doc.shape, dtype=np.float32)
        for i, qid in enumerate(qids):
            score[i, : count[i]] = [results[qid][d] for d in lists[qid]]
        q_ptr, q_term, q_weight = encode_queries([queries[qid] or "" for qid in qids], self.host.vocabulary, order=order)
        e_ptr, e_term, e_weight, _ = fwd.expand(q_ptr, q_term, q_weight, doc, score, count, fb_docs=max(1, int(doc.shape[1])), n_terms=n_terms,
                                                alpha=1.0 - weight, beta=weight, doc_weight=by, term_weight=self._fb_term_weight,
                                                term_gain=None if self._fb_gain is None else self._fb_gain.cpu().numpy())
        if self._words is None or self._words[0] is not self.host.vocabulary:
            words = [None] * self.host.vocab_size
            for w, t in self.host.vocabulary.items():
                words[t] = w
            self._words = (self.host.vocabulary, words)
        words = self._words[1]
        return {qid: {words[int(t)]: float(w) for t, w in zip(e_term[e_ptr[i]: e_ptr[i + 1]], e_weight[e_ptr[i]: e_ptr[i + 1]])} for i, qid in enumerate(qids)}

    def search_dicts(self, queries, top_k: int, *, order: str = "term", cache=None, lock=None, strip_key: bool = True,
                     blank: str = "empty", filter: Optional["DocFilterSpec"] = None, collapse: Optional["CollapseSpec"] = None,
                     expand: Optional["ExpandSpec"] = None, boost=None):
        """The cached batched search the API mirrors share: ``queries`` {qid: text} -> {qid: {doc_id: score}} with every qid
        in the caller's order, one batched search for all texts the cache does not hold (equal texts share one row).  What
        the call sites of the reference do differently is named here:

          * ``blank``      "empty": only a false text (``""``, ``None``) is answered ``{}`` unsearched
                           (retriever_registry.py:237-239); "whitespace": so is a text of white space only (retrieval.py:211-213)
                           -- which "empty" searches as an empty row;
          * ``strip_key``  the cache key is ``f"{text.strip()}:{top_k}"`` (retrieval.py:216) or the text as it is
                           (evaluate_rag_pipeline.py:340);
          * ``cache``      the caller's dict (entries: (rows i64, scores f32), read and written under ``lock``), at most
                           1 000 entries (retrieval.py:288); ``None`` = every call searches;
          * ``order``      the accumulation order of :func:`index.encode_queries`.

        A row without in-vocabulary terms gives ``{}`` and is not cached (retrieval.py:237-238, :251-252).  ``top_k`` beyond
        the corpus asks for ``n_docs`` rows; ``top_k <= 0`` keeps nothing (the reference's ``argpartition(...)[:0]``), cache
        hits aside.

        ``filter`` (:meth:`filter_spec`): the search is restricted to each query's allowed docs (``srx_search_filtered``).
        A filtered call neither reads nor writes the cache -- its key is the query text --, and equal texts share a row only
        under the same filter row.

        ``collapse`` (:meth:`collapse_spec`): every row is the top ``top_k`` of the COLLAPSED complete ranking, under ``filter``
        when given; such a call bypasses the cache as a filtered one does.

        ``expand`` (:meth:`expand_spec`): every row is the search of the query EXPANDED from its own first results, under
        ``filter`` and ``collapse`` when given; such a call bypasses the cache too.

        ``boost`` (:meth:`boost_spec`): every row is the top ``top_k`` of the BOOSTED complete ranking with its boosted scores,
        under ``filter`` and ``expand`` when given; such a call bypasses the cache too.  :meth:`search_rows` is the route of all four."""
        if filter is not None or collapse is not None or expand is not None or boost is not None:
            cache = None
        k_eff = min(int(top_k), self.n_docs_total)  # any depth: search_arrays pages past the engine's 1024-row lists
        results: Dict[str, Dict[str, float]] = {}
        pending: Dict[str, List[str]] = {}  # cache key -> the qids waiting for it
        texts: List[str] = []
        keys: List[str] = []
        frows: List[int] = []  # filtered: the filter row of every searched text
        for qid, text in queries.items():
            if not text or (blank == "whitespace" and not text.strip()):
                results[qid] = {}
                continue
            key = f"{text.strip() if strip_key else text}:{top_k}"
            hit = None
            if cache is not None:
                with lock:
                    hit = cache.get(key)
            if hit is not None:
                results[qid] = self.to_dict(*hit)
                continue
            results[qid] = {}  # keeps the caller's qid order; filled below
            if filter is not None:
                key = (key, filter.row_of_qid[qid])
            if key not in pending:
                pending[key] = []
                texts.append(text)
                keys.append(key)
                if filter is not None:
                    frows.append(filter.row_of_qid[qid])
            pending[key].append(qid)
        if texts and k_eff > 0:
            q_ptr, q_term, q_weight = encode_queries(texts, self.host.vocabulary, order=order)
            docs, scores, counts = self.search_rows(q_ptr, q_term, q_weight, k_eff, None if filter is None else filter.on_device(self.dev),
                                                    None if filter is None else np.asarray(frows, dtype=np.int32), collapse, expand, boost)
            for i, key in enumerate(keys):
                if q_ptr[i + 1] == q_ptr[i]:
                    continue
                c = int(counts[i])
                entry = (docs[i, :c].astype(np.int64), scores[i, :c].copy())
                if cache is not None:
                    with lock:
                        if len(cache) < 1000:
                            cache[key] = entry
                d = self.to_dict(*entry)
                for qid in pending[key]:
                    results[qid] = dict(d)
        return results

    def score_dicts(self, queries, candidates, order: str = "term"):
        """The dict form the API mirrors share: ``queries`` {qid: text}, ``candidates`` {qid: sequence of doc ids} ->
        {qid: {doc_id: exact score}} with every listed candidate in the caller's order (0.0 where no query term matches,
        and for a blank or all-OOV query); a qid without candidates gives {}; an unknown doc id raises ValueError.  One
        batch: ragged lists are padded with -1 and passed with their lengths (``cand_count``)."""
        results, live, cand_doc, cand_count = self.candidate_block(queries, candidates)
        if not live:
            return results
        q_ptr, q_term, q_weight = encode_queries([text for _, text, _ in live], self.host.vocabulary, order=order)
        scores = self.score_arrays(q_ptr, q_term, q_weight, cand_doc, cand_count)
        return scores_to_dicts(results, live, scores)

    def candidate_block(self, queries, candidates):
        """:func:`candidate_block` over this index's doc ids (their row numbers are kept between calls)"""
        return self._row_table().candidate_block(queries, candidates)

    def close(self) -> None:
        self._drop_field_table()
        self._drop_forward()
        if self.dev is not None:
            self.dev.close()
            self.dev = None
        self.searcher = None


def check_match(match, any_terms, call: str) -> None:
    """The ``match`` keyword of :meth:`SparseBackend.facets` / ``search_sorted`` next to ``any_terms``; raises ValueError"""
    if match not in ("any", "all", None):
        raise ValueError(f"match must be \"any\", \"all\" or None, got {match!r}")
    if match == "any" and any_terms is not None:
        raise ValueError(f"{call}: match=\"any\" puts the query's own terms into the any list; give match=None (or \"all\") with "
                         "any_terms=, or match=\"any\" without it")


class CollapseSpec:
    """The collapse keywords of one API call, checked (:meth:`SparseBackend.collapse_spec`): ``by`` = the column, ``per_group``,
    ``nulls`` ("own", "one", "drop") and ``depth`` = how deep the ranking may be read (None: until it is exhausted)."""

    def __init__(self, by: str, per_group: int = 1, nulls: str = "own", depth: Optional[int] = None):
        self.by, self.per_group, self.nulls, self.depth = by, per_group, nulls, depth


def _without_seeds(seeds, qids, allowed_docs, excluded_docs):
    """The two doc keywords of ``more_like_this`` with every qid's seeds denied: an allow list loses the seeds, otherwise the seeds
    join the exclude list (per qid; a sequence counts for every qid).  An ``allowed_docs`` dict must name every qid: a qid it
    leaves out could lose its seeds through an exclude list only, and the two keywords do not combine."""
    for what, given in (("allowed_docs", allowed_docs), ("excluded_docs", excluded_docs)):
        if isinstance(given, (str, bytes)):
            raise ValueError(f"{what} must be a sequence of doc ids or a dict qid -> sequence, not one string")
    of = lambda given, qid: list(given.get(qid, ())) if isinstance(given, dict) else list(given)
    if allowed_docs is None:
        return None, {qid: list(seeds[qid]) + ([] if excluded_docs is None else of(excluded_docs, qid)) for qid in qids}
    if isinstance(allowed_docs, dict) and any(qid not in allowed_docs for qid in qids):
        raise ValueError("more_like_this: an allowed_docs dict must name every qid (or pass include_seeds=True)")
    return {qid: [d for d in of(allowed_docs, qid) if d not in set(seeds[qid])] for qid in qids}, excluded_docs


class ExpandSpec:
    """The expansion keywords of one API call, checked (:meth:`SparseBackend.expand_spec`): ``docs`` = feedback docs per query,
    ``terms`` = expansion terms, ``weight`` = the feedback model's share of the expanded query, ``by`` = "score" or "uniform"."""

    def __init__(self, docs: int, terms: int = 10, weight: float = 0.5, by: str = "score"):
        self.docs, self.terms, self.weight, self.by = docs, terms, weight, by


def collapse_pool_depth(top_k: int, collapse_pool, n_docs: int, name: str = "collapse_pool") -> int:
    """Rows of the fused ranking a hybrid search collapses -- or boosts, under the ``name`` "boost_pool" -- (:func:`~.index.pool_depth`):
    ``collapse_pool`` in 1 .. 1024, else ``min(max(4 * top_k, 100), 1024)``."""
    from . import _capi
    return pool_depth(name, collapse_pool, max(4 * int(top_k), 100), _capi.SRX_MAX_K, n_docs)


def collapse_deep(search_fn, collapse_fn, q_ptr, q_term, q_weight, k: int, first: int, page: int = 1024, max_depth: Optional[int] = None):
    """The top ``k`` of the COLLAPSED complete ranking, exact, on top of a search limited to ``page`` rows per call:
    ``search_fn(q_ptr, q_term, q_weight, kk, after=None | (doc i32[nq], score f32[nq]))`` as :func:`~.index.deep_search` takes it,
    ``collapse_fn(doc [nq, m], score [nq, m], count [nq] | None, kk) -> (doc [nq, kk], score [nq, kk], count [nq])`` with the
    contract of ``srx_collapse_topk`` (include/sparse_rx_collapse.h: a doc id of -1 is a dead position), torch tensors throughout.

    The first ``first`` rows are fetched and collapsed.  A query is done when its count reached ``k`` or its last page came back
    short (its ranking is exhausted).  For the others the next page is the rows ranked strictly after their last row, and
    ``concat(kept so far, page)`` is collapsed: a query that continues was not cut at ``k``, and for such a list A
    ``collapse(collapse(A) ++ B) == collapse(A ++ B)``.  A finished query's bound is score 0 -- nothing ranks after it --, so
    its page is empty and its kept rows stay as they are.  One synchronisation per page (the "is anyone left" test), as in
    ``deep_search``.

    ``max_depth`` None reads until every query is done; a number stops after that many rows of the ranking, and a query may
    then come back with FEWER than ``k`` rows although more groups exist further down: that is the caller's trade, not an error.
    ``m`` stays below ``k + page`` <= 2048 for k, page <= 1024."""
    import torch

    def reduce(d, s, c, kept, kk):
        if kept is None:
            return collapse_fn(d, s, c, kk)
        # the padding of the kept rows lies in front of the page: no count, a doc id of -1 is dead
        return collapse_fn(torch.cat([kept[0], d], dim=1).contiguous(), torch.cat([kept[1], s], dim=1).contiguous(), None, kk)

    def unfinished(d, s, c, kk, ks, kc):
        return (kc < k) & (c == kk)

    return deep_reduce(search_fn, reduce, unfinished, q_ptr, q_term, q_weight, k, first, page, max_depth)


def facet_dict(spec, counts, extra, top=None) -> dict:
    """One row of a facet call decoded: ``{"counts": {value: n, ...}, "missing": n, "other": n, "total": n}``.  ``spec``: the
    :class:`~.fields.FacetSpec` (``values[i]`` = what bin i stands for: a category string, a label, an int, a ``(lo, hi)`` pair of
    the caller's edges); ``counts``: the row's n_bins numbers, or None for a row that was not counted; ``extra``: (missing, other,
    total).  Only bins with a count above 0 are listed, by count descending, then by bin ascending, cut to ``top``."""
    listed = {}
    if counts is not None:
        order = sorted((i for i in range(spec.n_bins) if int(counts[i]) > 0), key=lambda i: (-int(counts[i]), i))
        listed = {spec.values[i]: int(counts[i]) for i in (order if top is None else order[: int(top)])}
    return {"counts": listed, "missing": int(extra[0]), "other": int(extra[1]), "total": int(extra[2])}


class RowOfIds:
    """doc id -> row of one list of doc ids, built once and kept by whoever scores named docs (``ids`` is the list it was
    built from: a holder rebuilds it when its list is another object)."""

    def __init__(self, ids):
        self.ids = ids
        self.row_of = {d: i for i, d in enumerate(ids)}

    @classmethod
    def numbered(cls, n: int) -> "RowOfIds":
        """Docs named by their row number as a string: no table"""
        r = cls(())
        r.row_of = _NumberedRows(n)
        return r

    def candidate_block(self, queries, candidates):
        return candidate_block(self.row_of, queries, candidates)


class _NumberedRows:
    def __init__(self, n: int):
        self.n = n

    def __getitem__(self, d):
        i = int(d) if isinstance(d, str) and d.isdigit() else -1
        if not (0 <= i < self.n and str(i) == d):
            raise KeyError(d)
        return i


def candidate_block(row_of, queries, candidates):
    """``candidates`` {qid: sequence of doc ids} for the qids of ``queries`` as one padded block; ``row_of`` maps a doc id
    to its row.  Returns (results = {qid: {}} for every qid, live = [(qid, queries[qid], or "" for None, its candidates)]
    for the qids that have any, cand_doc i32[len(live), m] padded with -1, cand_count i32[len(live)]).  An unknown doc id
    raises ValueError."""
    results = {qid: {} for qid in queries}
    live, rows = [], []
    for qid, text in queries.items():
        cands = list(candidates.get(qid, ()) or ())
        if not cands:
            continue
        try:
            rows.append([row_of[d] for d in cands])
        except KeyError as e:
            raise ValueError(f"unknown doc id {e.args[0]!r} among the candidates of {qid!r}") from None
        live.append((qid, "" if text is None else text, cands))
    m = max((len(r) for r in rows), default=1)
    cand_doc = np.full((len(rows), m), -1, dtype=np.int32)
    cand_count = np.zeros(len(rows), dtype=np.int32)
    for i, r in enumerate(rows):
        cand_doc[i, : len(r)] = r
        cand_count[i] = len(r)
    return results, live, cand_doc, cand_count


class DocFilterSpec:
    """The ``allowed_docs`` / ``excluded_docs`` keywords of one API call, resolved on the host: ``lists`` = one array of doc
    rows per filter row, ``allow`` = the listed rows are the allowed ones (else the excluded ones), ``row_of_qid`` = every
    qid's filter row (-1: not filtered)."""

    def __init__(self, allow: bool, lists, row_of_qid):
        self.allow, self.lists, self.row_of_qid = allow, lists, row_of_qid

    def on_device(self, index):
        """The :class:`~.filter.DocFilter` over ``index``'s rows (a DeviceIndex or a dense index of the same corpus)"""
        from .filter import DocFilter
        build = DocFilter.allow if self.allow else DocFilter.deny
        base = int(index.doc_base)
        return build([r + base for r in self.lists], index.n_docs, device=index.device, doc_base=base)


def doc_filter_spec(row_of, queries, allowed_docs, excluded_docs) -> Optional[DocFilterSpec]:
    """The two filter keywords of the API mirrors -> a :class:`DocFilterSpec`, or None when both are None.  Each keyword is a
    sequence of doc ids (one filter for every query of the call) or a dict ``qid -> sequence`` (a qid missing from it is not
    filtered).  Giving both, a bare string, or an unknown doc id raises ValueError (``row_of`` maps a doc id to its row)."""
    if allowed_docs is None and excluded_docs is None:
        return None
    if allowed_docs is not None and excluded_docs is not None:
        raise ValueError("give allowed_docs or excluded_docs, not both")
    allow = allowed_docs is not None
    what, given = ("allowed_docs", allowed_docs) if allow else ("excluded_docs", excluded_docs)
    if isinstance(given, (str, bytes)):
        raise ValueError(f"{what} must be a sequence of doc ids or a dict qid -> sequence, not one string")

    def rows(ids, whose):
        if isinstance(ids, (str, bytes)):
            raise ValueError(f"{what}{whose} must be a sequence of doc ids, not one string")
        try:
            return np.asarray([row_of[d] for d in ids], dtype=np.int64)
        except KeyError as e:
            raise ValueError(f"unknown doc id {e.args[0]!r} in {what}{whose}") from None

    if not isinstance(given, dict):
        return DocFilterSpec(allow, [rows(given, "")], {qid: 0 for qid in queries})
    lists, row_of_qid = [], {}
    for qid in queries:
        if qid in given:
            row_of_qid[qid] = len(lists)
            lists.append(rows(given[qid], f"[{qid!r}]"))
        else:
            row_of_qid[qid] = -1
    return DocFilterSpec(allow, lists or [np.zeros(0, np.int64)], row_of_qid)


class RowFilterSpec:
    """What the specs of the row builders share: ``rows`` = one (all, any, none) triple of id tuples per filter row,
    ``row_of_qid`` = every qid's row (-1: not filtered) and, with a base (:meth:`with_base`), ``base`` = the spec the rows are
    intersected with and ``base_rows`` = its row for every row here (-1: none).  A kind adds what its ids mean and
    ``on_device(index)``, which builds the rows.  Memory on the device: len(rows) * n_docs / 8 bytes -- 1.25 MB per row at 10 M docs."""

    def __init__(self, rows, row_of_qid, base=None, base_rows=None):
        self.rows, self.row_of_qid, self.base, self.base_rows = rows, row_of_qid, base, base_rows

    def with_base(self, base_spec, queries):
        """This spec restricted to the docs ``base_spec`` (any spec of the same call, or None) allows: one row per distinct
        (base row, own row) pair of the call's qids; a qid neither spec filters stays unfiltered."""
        if base_spec is None:
            return self
        pairs, row_of_qid = {}, {}
        for qid in queries:
            pair = (base_spec.row_of_qid[qid], self.row_of_qid[qid])
            row_of_qid[qid] = -1 if pair == (-1, -1) else pairs.setdefault(pair, len(pairs))
        empty = ((), (), ())
        spec = copy.copy(self)
        spec.rows, spec.row_of_qid = [self.rows[own] if own >= 0 else empty for _, own in pairs] or [empty], row_of_qid
        spec.base, spec.base_rows = base_spec, [b for b, _ in pairs] or [-1]
        return spec


class TermFilterSpec(RowFilterSpec):
    """The ``must_terms`` / ``any_terms`` / ``must_not_terms`` keywords of one API call, resolved on the host: the ids of ``rows``
    are term ids (-1: an out-of-vocabulary word).  ``sparse`` () -> the DeviceIndex whose postings answer "doc has term" (None:
    the index :meth:`on_device` is given)."""

    def __init__(self, rows, row_of_qid, base=None, base_rows=None):
        super().__init__(rows, row_of_qid, base, base_rows)
        self.sparse = None

    def on_device(self, index):
        """The :class:`~.filter.DocFilter` of the rows (``srx_filter_from_terms`` on the sparse index), for ``index``: the sparse
        index itself or a dense index of the same corpus (same n_docs / doc_base / device)"""
        sparse = index if self.sparse is None else self.sparse()
        if not hasattr(sparse, "term_filter"):
            raise ValueError("term constraints need the sparse index of the corpus (its posting lists)")
        base = None if self.base is None else self.base.on_device(sparse)
        lists = [[list(r[i]) for r in self.rows] for i in range(3)]
        return sparse.term_filter(*lists, base=base, q_base=None if base is None else self.base_rows)


def term_filter_spec(vocabulary, queries, must_terms=None, any_terms=None, must_not_terms=None) -> Optional[TermFilterSpec]:
    """The three term keywords of the API mirrors -> a :class:`TermFilterSpec`, or None when no qid of ``queries`` is
    constrained.  Each keyword is None, a sequence of strings (for every query of the call) or a dict ``qid -> sequence`` (a qid
    missing from all three is not constrained).  Every string goes through :func:`~.index.tokenize`: all its tokens join the
    list, an out-of-vocabulary token as -1; a string without tokens, or a bare string where a sequence belongs, raises
    ValueError.  Equal (must, any, must-not) triples share one row."""
    per_qid = {qid: [(), (), ()] for qid in queries}
    for i, (what, given) in enumerate((("must_terms", must_terms), ("any_terms", any_terms), ("must_not_terms", must_not_terms))):
        if given is None:
            continue
        if isinstance(given, (str, bytes)):
            raise ValueError(f"{what} must be a sequence of strings or a dict qid -> sequence, not one string")

        def ids(words, whose):
            if isinstance(words, (str, bytes)):
                raise ValueError(f"{what}{whose} must be a sequence of strings, not one string")
            out = []
            for w in words:
                toks = tokenize(w) if isinstance(w, str) else []
                if not toks:
                    raise ValueError(f"{w!r} in {what}{whose} holds no token")
                out.extend(int(vocabulary.get(t, -1)) for t in toks)
            return tuple(out)

        if isinstance(given, dict):
            for qid in queries:
                if qid in given:
                    per_qid[qid][i] = ids(given[qid], f"[{qid!r}]")
        else:
            shared = ids(given, "")
            for qid in queries:
                per_qid[qid][i] = shared
    rows, row_of, row_of_qid = [], {}, {}
    for qid in queries:
        triple = tuple(per_qid[qid])
        if triple == ((), (), ()):
            row_of_qid[qid] = -1
            continue
        if triple not in row_of:
            row_of[triple] = len(rows)
            rows.append(triple)
        row_of_qid[qid] = row_of[triple]
    return TermFilterSpec(rows, row_of_qid) if rows else None


class FieldFilterSpec(RowFilterSpec):
    """The ``where`` keyword of one API call, resolved on the host: ``resolver`` = the :class:`~.fields.WhereResolver` that holds
    the call's clause records, the ids of ``rows`` are its clause ids.  ``table`` () -> the :class:`~.fields.FieldTable` of the
    corpus."""

    def __init__(self, resolver, rows, row_of_qid, base=None, base_rows=None):
        super().__init__(rows, row_of_qid, base, base_rows)
        self.resolver, self.table = resolver, None

    def on_device(self, index):
        """The :class:`~.filter.DocFilter` of the rows (``srx_filter_from_fields`` on the field table), for ``index``: any index of
        the same corpus (same n_docs / doc_base / device)"""
        if self.table is None:
            raise ValueError("field predicates need the docs' field table")
        base = None if self.base is None else self.base.on_device(index)
        return self.table().filter_resolved(self.resolver, self.rows, base=base, q_base=None if base is None else self.base_rows)


def field_filter_spec(schema, queries, where) -> Optional[FieldFilterSpec]:
    """The ``where`` keyword of the API mirrors -> a :class:`FieldFilterSpec`, or None when no qid of ``queries`` is constrained.
    ``where`` is one group for every query -- a dict whose keys all lie in {"must", "should", "must_not"}, or a bare list of
    clauses -- or a dict ``qid -> group`` (a qid missing from it is not constrained).  ``schema``: name ->
    :class:`~.fields.HostColumn`.  Equal clauses share a record and equal groups a row; a malformed group or clause, an unknown
    field or a test that does not fit its column raises ValueError."""
    from .fields import WhereResolver, is_group
    res = WhereResolver(schema, share_rows=True)
    if is_group(where):
        shared = res.add(where)
        row_of_qid = {qid: shared for qid in queries}
    elif isinstance(where, dict):
        row_of_qid = {qid: res.add(where[qid]) if qid in where else -1 for qid in queries}
    else:
        raise ValueError("where must be a group (must / should / must_not, or a list of clauses) or a dict qid -> group")
    return FieldFilterSpec(res, list(res.rows), row_of_qid) if res.rows else None


def apply_operators(queries, must_terms=None, must_not_terms=None):
    """``operators=True`` of the API mirrors: :func:`~.index.parse_operators` on every query text.  Returns (queries with the
    scored texts, must_terms, must_not_terms) where the two keywords are dicts ``qid -> list`` that hold the caller's words (a
    sequence counts for every qid) followed by the query's own ``+`` / ``-`` words."""
    def per_qid(what, given):
        if given is None:
            return {qid: [] for qid in queries}
        if isinstance(given, (str, bytes)):
            raise ValueError(f"{what} must be a sequence of strings or a dict qid -> sequence, not one string")
        if isinstance(given, dict):
            for qid, words in given.items():
                if isinstance(words, (str, bytes)):
                    raise ValueError(f"{what}[{qid!r}] must be a sequence of strings, not one string")
            return {qid: list(given.get(qid, ())) for qid in queries}
        return {qid: list(given) for qid in queries}

    must, must_not = per_qid("must_terms", must_terms), per_qid("must_not_terms", must_not_terms)
    texts = {}
    for qid, text in queries.items():
        if not text:
            texts[qid] = text
            continue
        texts[qid], plus, minus = parse_operators(text)
        must[qid] += plus
        must_not[qid] += minus
    return texts, must, must_not


def scores_to_dicts(results, live, scores):
    """f32[len(live), m] scores of a :func:`candidate_block` into ``results``: every candidate in the caller's order"""
    for i, (qid, _, cands) in enumerate(live):
        results[qid] = {d: float(scores[i, c]) for c, d in enumerate(cands)}
    return results


class SparseIndexViews:
    """The reference's attribute names as read-only views of ``self._be`` (a :class:`SparseBackend`), and the doors that only check
    for an index and hand on to it: shared by ``RetrievalService`` and the registry mirrors.  What differs between them:"""

    not_built = "Index not built. Call build_index_from_corpus() first."  # what a door says before the build call
    mode = "bm25"  # how the index scores ("bm25" or "dot"): the feedback's forward index follows it
    term_order = "term"  # accumulation order of a doc's contributions (index.encode_queries)

    def _need_index(self) -> None:
        if self.host is None:
            raise ValueError(self.not_built)

    @property
    def host(self) -> Optional[HostIndex]:
        return self._be.host  # sharded: this rank's rows, corpus-wide vocabulary / idf / avgdl / doc ids

    @property
    def dev(self) -> Optional[DeviceIndex]:
        return self._be.dev

    @property
    def vocabulary(self) -> Dict[str, int]:
        return self.host.vocabulary if self.host else {}

    @property
    def doc_ids(self) -> List[str]:
        return self.host.doc_ids if self.host else []

    @property
    def corpus_tf(self):
        if self.host is None:
            return None
        from scipy.sparse import csr_matrix
        h = self.host
        return csr_matrix((h.data, h.indices, h.indptr), shape=(h.n_docs, h.vocab_size))

    def _to_dict(self, idx, sc) -> Dict[str, float]:
        return self._be.to_dict(idx, sc)

    # -- the shared doors (no reference counterpart) ----------------------------------------------------------------
    def set_doc_fields(self, columns) -> None:
        """The docs' metadata as typed columns for the ``where=`` keyword of the searches (no reference counterpart: nothing
        reads its ``metadata`` dicts).  ``columns``: name -> a sequence with one entry per doc, in the order of the corpus the
        build call was given (:func:`~.fields.columns_from_metadata` makes them from the corpus; the type mapping is
        :meth:`~.fields.FieldTable.from_columns`'s).  A length that is not the index's raises ``ValueError``.  The columns go to
        the GPU with the first ``where=`` call and stay there; a rebuilt index drops them."""
        self._need_index()
        self._be.set_fields(columns)

    def enable_feedback(self) -> None:
        """Opt in to relevance feedback (no reference counterpart): build the doc-major forward index of the corpus on the GPU
        (:class:`~.feedback.ForwardIndex`, include/ext/sparse_rx_feedback.h: 8 bytes per posting and 12 per doc next to the
        index) for ``expand_docs=``, :meth:`more_like_this` and :meth:`expand_queries`.  A rebuilt or re-uploaded index and
        :meth:`close` drop it.  ``ValueError``: no index, a sharded index."""
        self._need_index()
        self._be.enable_feedback(self.mode)

    def more_like_this(self, seeds: Dict[str, Sequence[str]], top_k: int = 10, terms: int = 25, include_seeds: bool = False, *, allowed_docs=None,
                       excluded_docs=None, must_terms=None, any_terms=None, must_not_terms=None, where=None) -> Dict[str, Dict[str, float]]:
        """More like these docs (Lucene's ``more_like_this``; no reference counterpart): ``seeds`` = ``{qid: [doc_id, ...]}``, at
        most 32 per query -> ``{qid: {doc_id: score}}``.  The query is built on the GPU from the seeds alone: the ``terms`` terms
        that characterise them best (``srx_feedback_expand`` with empty queries, the seeds as uniformly weighted feedback docs,
        beta = 1), weights summing to 1; it is searched with the seeds themselves denied per query unless ``include_seeds``.  The
        filter keywords are those of the searches.  ``ValueError``: no :meth:`enable_feedback`, a sharded index, an unknown doc
        id, more than 32 seeds, ``terms`` outside 1..128."""
        self._need_index()
        return self._be.more_like_this(seeds, top_k, terms, include_seeds, allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, where)

    def expand_queries(self, queries: Dict[str, str], results: Dict[str, Dict[str, float]], *, expand_terms: int = 10, expand_weight: float = 0.5,
                       expand_by: str = "score") -> Dict[str, Dict[str, float]]:
        """What queries are expanded to: ``results`` = ``{qid: {doc_id: score}}`` as a search returned them are the feedback docs
        (dict order, at most 32 per query) -> ``{qid: {word: weight}}`` in ascending term id: the batch the second pass of
        ``expand_docs=len(results[qid])`` searches.  ``ValueError`` as :meth:`more_like_this`."""
        self._need_index()
        return self._be.expand_queries(queries, results, expand_terms, expand_weight, expand_by, order=self.term_order)

    def facets(self, queries: Dict[str, str], fields, *, match="any", allowed_docs=None, excluded_docs=None, must_terms=None, any_terms=None,
               must_not_terms=None, operators: bool = False, where=None, top: Optional[int] = None):
        """Facet counts (no reference counterpart: it does not aggregate results): how the docs of each query's doc set distribute
        over metadata columns of :meth:`set_doc_fields`, counted on the GPU (``srx_facet_counts``, include/sparse_rx_facets.h).
        ``fields``: one name, a sequence of names, or a dict name -> binning spec (:func:`~.fields.check_facet_args`: a category,
        bool or set column takes none; an int column ``{"origin": o, "bins": n}`` or ``{"edges": [...]}``; a float32 column
        ``{"edges": [...]}``).  Returns ``{qid: {field: {"counts": {value: n, ...}, "missing": n, "other": n, "total": n}}}``: only
        bins with a count above 0, by count descending, then by bin ascending, cut to ``top``; a value is a category string, a
        label, False / True, an int, or the ``(lo, hi)`` pair of the caller's own edges; ``missing`` = docs without a value,
        ``other`` = docs whose value lies in no bin, ``total`` = docs of the set.

        The doc set: the doc, term and field keywords as in the searches, chained; and ``match`` for the query's own text --
        ``"any"`` (default): the docs that contain at least one known term of the text.  That is the query's candidate set BY
        TERMS, a superset of the docs the search returns under its ``score > 0`` rule.  The terms join the ``any`` list: giving
        ``any_terms=`` as well raises ``ValueError``.  ``"all"``: the docs that contain every term (they join the ``must`` list; an
        unknown word empties the set).  ``None``: the text is ignored.  Under "any" / "all" a text without a token has the empty
        set.  ``ValueError``: no :meth:`set_doc_fields`, an unknown field, a spec that does not fit its column, a sharded index."""
        self._need_index()
        if operators:
            queries, must_terms, must_not_terms = apply_operators(queries, must_terms, must_not_terms)
        return self._be.facets(queries, fields, match, allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, where, top, "facets")

    def facets_of(self, results, fields, top: Optional[int] = None):
        """Facet counts over the docs of result lists: ``results`` = ``{qid: {doc_id: score}}`` as any search of this object,
        a reranker or ``collapse`` returns it -> the dict of :meth:`facets` (``srx_facet_counts_lists``: every listed doc counts,
        whatever its score).  ``ValueError``: an unknown doc id, no :meth:`set_doc_fields`, an unknown field, a sharded index."""
        self._need_index()
        return self._be.facets_of(results, fields, top, "facets_of")

    def search_sorted(self, queries: Dict[str, str], by: str, *, order: str = "desc", top_k: int = 10, match="any", nulls: str = "last",
                      allowed_docs=None, excluded_docs=None, must_terms=None, any_terms=None, must_not_terms=None, where=None):
        """Order by a field instead of relevance (no reference counterpart): the first ``top_k`` docs of each query's doc set by the
        value the column ``by`` of :meth:`set_doc_fields` holds for them, selected on the GPU (``srx_order_topk``,
        include/order/sparse_rx_order.h) -> ``{qid: {doc_id: value}}`` in rank order.  The doc set and ``match`` are those of
        :meth:`facets`.  ``order`` "asc" / "desc"; docs with equal values come in corpus order; ``nulls``: docs without a value come
        "last", "first" or "drop" out (their value is None).  A value is an int, bool, float or a category's string (categories
        order alphabetically).  ``top_k`` above 1024 pages with a cursor.  ``ValueError``: no :meth:`set_doc_fields`, a sharded
        index, an unknown field, a set column, a bad keyword."""
        self._need_index()
        return self._be.search_sorted(queries, by, order, top_k, match, nulls, allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms,
                                      where, "search_sorted")

    def sort_results(self, results, by: str, *, order: str = "desc", nulls: str = "last", top_k: Optional[int] = None):
        """Result lists reordered by a field: ``results`` = ``{qid: {doc_id: score}}`` as any search of this object returns it ->
        the same dicts, scores unchanged, in the order of the column ``by`` (``srx_order_lists``; equal values keep their relevance
        order), cut to ``top_k``.  ``ValueError``: a list deeper than 2048, an unknown doc id, and what :meth:`search_sorted`
        refuses."""
        self._need_index()
        return self._be.sort_results(results, by, order, nulls, top_k, "sort_results")

    def boost_results(self, results, boost, top_k: Optional[int] = None):
        """Result lists re-scored by field values: ``results`` = ``{qid: {doc_id: score}}`` as any search of this object returns it
        -> ``{qid: {doc_id: boosted score}}``, the first ``top_k`` (None: all) by boosted score (``srx_boost_topk``; ties in corpus
        order).  ``boost`` as the searches take it, every ``boost_mode`` allowed; the result is relative to the lists given.
        ``ValueError``: a list deeper than 2048, an unknown doc id, what the spec gets wrong, no :meth:`set_doc_fields`, a sharded
        index."""
        self._need_index()
        return self._be.boost_results(results, boost, top_k, "boost_results")

    def set_rank_model(self, model, features) -> None:
        """The learned reranker of ``rank_model=True`` and :meth:`rerank_model` (no reference counterpart): ``model`` a
        :class:`~.ltr.ForestModel` (``ForestModel.from_sklearn`` / ``from_arrays``), ``features`` the list whose entry f is the
        model's feature f -- "score", "rank", the name of a number column of :meth:`set_doc_fields`, ``("extra", i)``, and in
        ``search_hybrid`` "sparse_score" / "dense_score".  ``ValueError``: no ForestModel, a list that does not fit the model."""
        self._be.set_rank_model(model, features)

    def rerank_model(self, results, top_k: Optional[int] = None, extra=None, mode: str = "replace"):
        """Result lists re-scored by the model of :meth:`set_rank_model`: ``results`` = ``{qid: {doc_id: score}}`` as any search of
        this object returns it -> ``{qid: {doc_id: model score}}``, the first ``top_k`` (None: all) by model score
        (``srx_ltr_topk``, include/ltr/sparse_rx_ltr.h; ties in corpus order).  ``mode`` "replace": the model's output; "sum": the
        score given plus it.  ``extra``: ``{qid: {doc_id: [floats]}}`` for the ``("extra", i)`` features.  The result is relative to
        the lists given.  ``ValueError``: no :meth:`set_rank_model`, a list deeper than 2048, an unknown doc id, a feature that names
        a column without :meth:`set_doc_fields`, a set column, "sparse_score" / "dense_score" (``search_hybrid`` only), a sharded
        index."""
        self._need_index()
        return self._be.rerank_model_results(results, top_k, extra, mode, "rerank_model")

    search_door = "search"  # the class's own batched search: what :meth:`rank_eval` runs, and its name in the messages
    blank = "empty"  # which texts are answered {} unsearched (search_dicts): a false one; the service: "whitespace"
    strip_cache_key = True  # the cache key is the stripped text; OptimizedRetriever: the text as it is

    def _search(self, queries, top_k, filters, collapse, expand, boost=None, boost_depth=None, rank_model=False, rank_pool=None):
        """The body of the class's batched search (its docstring names the keywords): ``filters`` = (allowed_docs, excluded_docs,
        must_terms, any_terms, must_not_terms, operators, where), ``collapse`` = (collapse_by, per_group, collapse_nulls,
        collapse_depth), ``expand`` = (expand_docs, expand_terms, expand_weight, expand_by).  With a rank model the search runs at
        ``top_k`` = the pool, its specs checked against the pool, and :meth:`SparseBackend.rerank_model_results` cuts it to the
        caller's ``top_k``.  The checks come in one order: the index, the model, the filter chain, collapse, expand, boost."""
        be, call = self._be, self.search_door
        self._need_index()
        ranked = be.rank_spec(rank_model, rank_pool, top_k, call, boost)
        if ranked is not None:
            if min(int(top_k), be.n_docs_total) <= 0:
                return {qid: {} for qid in queries}
            return be.rerank_model_results(self._search(queries, ranked.pool, filters, collapse, expand), top_k, call=call)
        allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, operators, where = filters
        if operators:
            queries, must_terms, must_not_terms = apply_operators(queries, must_terms, must_not_terms)
        spec = be.filter_spec(queries, allowed_docs, excluded_docs, must_terms, any_terms, must_not_terms, where, call)
        collapse = be.collapse_spec(*collapse, top_k, call)
        expand = be.expand_spec(*expand, call)
        boosted = be.boost_spec(boost, boost_depth, top_k, call, collapse)
        if not self._before_search(top_k, expand):
            return {qid: {} for qid in queries}
        # search_dicts leaves the cache alone when one of the four specs is given
        return be.search_dicts(queries, top_k, order=self.term_order, cache=self.query_cache, lock=self.cache_lock, strip_key=self.strip_cache_key,
                               blank=self.blank, filter=spec, collapse=collapse, expand=expand, boost=boosted)

    def _before_search(self, top_k, expand) -> bool:
        """What a class does between the checks and the search; False: every query is answered {} unsearched"""
        return True

    def evaluate(self, qrels, results, k_values=(1, 3, 5, 10, 100), *, gain: str = "linear", rel_level: int = 1, per_query: bool = False,
                 complete: bool = False, ignore_identical_ids: bool = False):
        """Ranking quality of result lists (the reference's ``EvaluateRetrieval.evaluate(qrels, results, k_values)`` step, which it
        takes from BEIR / pytrec_eval on the host): ``qrels`` = ``{qid: {doc_id: int grade}}`` (or a :class:`~.evaluate.Judgments`
        built once by ``Judgments.from_qrels(qrels, None, self.doc_ids, device=...)``), ``results`` = ``{qid: {doc_id: score}}`` as any
        search of this object, a reranker or a fusion returns it -> ``{"NDCG@k", "MAP@k", "Recall@k", "P@k", "MRR@k", "Success@k",
        "Judged@k" for every k of k_values, "n_queries"}``, the means over the queries that are judged and have an entry in
        ``results`` (``complete``: every judged query; one without an entry scores zeros), computed on the GPU (``srx_eval_lists``,
        include/eval/sparse_rx_eval.h).  ``per_query`` also returns ``{qid: {...}}``.  A list is ranked by (score descending, doc id
        ascending in corpus order), cut at 2 048; ``gain`` "linear" (trec_eval) | "exp2"; relevant = grade >= ``rel_level``;
        ``ignore_identical_ids`` drops ``doc_id == qid``.  Global doc ids only: a SHARDED index is evaluated like any other.
        ``ValueError``: no index, 0 or more than 8 cutoffs, not ascending, one above 2 048, a grade that is no int."""
        self._need_index()
        from .evaluate import evaluate_results
        device = self._be.dev.device if self._be.dev is not None else self._be.device
        return evaluate_results(qrels, results, self.host.doc_ids, device, k_values, gain=gain, rel_level=rel_level, per_query=per_query,
                                complete=complete, ignore_identical_ids=ignore_identical_ids)

    def rank_eval(self, queries: Dict[str, str], qrels, k_values=(1, 3, 5, 10, 100), **search_keywords):
        """Search, then :meth:`evaluate` (Elasticsearch's ``_rank_eval``): this object's own search at ``top_k = max(k_values)`` with
        ``search_keywords`` passed through (the filter, collapse, boost, rank-model keywords; ``gain``, ``rel_level``, ``per_query``,
        ``complete`` and ``ignore_identical_ids`` go to :meth:`evaluate`).  No search path of its own."""
        from .evaluate import check_cutoffs
        from . import _capi
        ks = check_cutoffs(k_values, cap=_capi.SRX_EVAL_MAX_M)
        eval_keywords = {k: search_keywords.pop(k) for k in ("gain", "rel_level", "per_query", "complete", "ignore_identical_ids") if k in search_keywords}
        if "top_k" in search_keywords:
            raise ValueError("rank_eval searches at top_k = max(k_values): give no top_k")
        results = getattr(self, self.search_door)(queries, top_k=ks[-1], **search_keywords)
        return self.evaluate(qrels, results, ks, **eval_keywords)
