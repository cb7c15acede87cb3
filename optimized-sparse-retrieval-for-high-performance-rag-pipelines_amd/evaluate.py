"""Ranking evaluation (include/eval/sparse_rx_eval.h): nDCG, MAP, recall, precision, MRR and success of ranked lists against
graded relevance judgments, at several cutoffs per query and as batch means, by ``srx_eval_lists`` on the GPU.

:class:`Judgments` is the header's CSR over the judged queries -- built once from a BEIR / pytrec_eval ``qrels`` dict
(:meth:`Judgments.from_qrels`) or from integer triples (:meth:`Judgments.from_arrays`), resident on the device;
:meth:`Judgments.evaluate_device` takes exactly what ``DeviceIndex.search_device``, the fusion and the ``*_topk`` stages return
(GLOBAL doc ids, so the merged lists of a sharded index too) and returns device tensors.  :func:`evaluate_results` is the dict
door behind ``evaluate(qrels, results, k_values)`` of the retrievers; its two host halves -- :func:`lists_from_results`,
:func:`metrics_dicts` -- hold no arithmetic of the metrics except ``Judged@k``.

The gain and discount tables are sampled here in float64 and rounded once to float32: the device contract holds no
transcendental function.  Not covered: lists deeper than 2 048, re-sorting of score ties inside :meth:`Judgments.evaluate_device`
(the order given is the ranking), set-based measures over the whole ranking (bpref, infAP), significance tests."""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _capi

GAINS = ("linear", "exp2")  # "linear": g (trec_eval's nDCG); "exp2": 2^g - 1 (Elasticsearch, LambdaMART)
WAVE_M, LDS_ROW, MEAN_CHUNK = _capi.SRX_EVAL_WAVE_M, _capi.SRX_EVAL_LDS_ROW, _capi.SRX_EVAL_MEAN_CHUNK  # the kernel's size constants
# BEIR's key spelling -> the plane of ``out``'s last axis
METRIC_KEYS = (("NDCG", _capi.SRX_EVAL_NDCG), ("MAP", _capi.SRX_EVAL_AP), ("Recall", _capi.SRX_EVAL_RECALL), ("P", _capi.SRX_EVAL_P),
               ("MRR", _capi.SRX_EVAL_RR), ("Success", _capi.SRX_EVAL_SUCCESS))
DEFAULT_K_VALUES = (1, 3, 5, 10, 100)

EvalResult = namedtuple("EvalResult", "out hits judged rel mean n")
EvalResult.__doc__ = """``out`` f32[nq, n_k, 8] (the metric planes of the header), ``hits`` / ``judged`` i32[nq, n_k], ``rel`` i32[nq], and
with means ``mean`` f64[n_k, 8] and ``n`` i32[1] (the evaluated queries); None without."""


def _torch():
    import torch
    return torch


_ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()


def gain_table(kind: str, n_gain: int) -> np.ndarray:
    """f32[n_gain]: ``g`` ("linear") or ``2^g - 1`` ("exp2"), computed in float64 and rounded once; entry 0 is +0"""
    if kind not in GAINS:
        raise ValueError(f"gain must be one of {list(GAINS)}, got {kind!r}")
    if not (1 <= int(n_gain) <= _capi.SRX_EVAL_MAX_GAIN):
        raise ValueError(f"n_gain must be in [1, {_capi.SRX_EVAL_MAX_GAIN}], got {n_gain}")
    g = np.arange(int(n_gain), dtype=np.float64)
    return (g if kind == "linear" else np.exp2(g) - 1.0).astype(np.float32)


def discount_table(m: int) -> np.ndarray:
    """f32[m]: ``1 / log2(r + 2)`` of position r, computed in float64 and rounded once"""
    return (1.0 / np.log2(np.arange(int(m), dtype=np.float64) + 2.0)).astype(np.float32)


def check_cutoffs(ks, cap: Optional[int] = None) -> List[int]:
    """The cutoffs as the header takes them: 1 to 8 ints >= 1, strictly ascending (``cap``: none above it).  ValueError otherwise."""
    try:
        out = [int(k) for k in ks]
    except TypeError:
        raise ValueError(f"k_values must be a sequence of ints, got {ks!r}") from None
    if not (1 <= len(out) <= _capi.SRX_EVAL_MAX_K) or any(k != kk for k, kk in zip(out, ks)):
        raise ValueError(f"k_values must hold 1 to {_capi.SRX_EVAL_MAX_K} ints, got {ks!r}")
    if out[0] < 1 or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"k_values must be >= 1 and strictly ascending, got {ks!r}")
    if cap is not None and out[-1] > cap:
        raise ValueError(f"a cutoff above {cap} is not evaluated (lists are taken to a depth of {cap}), got {out[-1]}")
    return out


class Judgments:
    """Graded relevance judgments as ``srx_eval_lists`` reads them: ``j_ptr`` int64 [n_rows + 1], ``j_doc`` int32 (ascending inside
    a row), ``j_grade`` int32, ``j_ideal`` int32 (a row's grades, descending).  ``query_ids``: the id of every row (or None),
    ``extra_ids``: the judged doc ids that are not in the corpus -> the ids they were given.  Build one with :meth:`from_qrels`
    or :meth:`from_arrays`; the constructor checks nothing.  ``device`` None: a host object (the arrays and the dict halves work,
    the evaluation raises)."""

    def __init__(self, j_ptr, j_doc, j_grade, j_ideal, device=None, query_ids=None, extra_ids=None, doc_rows=None):
        self.j_ptr, self.j_doc, self.j_grade, self.j_ideal = j_ptr, j_doc, j_grade, j_ideal
        self.device, self.query_ids, self.extra_ids, self.doc_rows = device, query_ids, extra_ids or {}, doc_rows
        self.row_of = {qid: r for r, qid in enumerate(query_ids)} if query_ids is not None else None
        self.max_grade = int(j_grade.max()) if len(j_grade) else 0
        self._dev = None
        self._tables = {}

    n_rows = property(lambda self: len(self.j_ptr) - 1)
    nnz = property(lambda self: len(self.j_doc))

    @property
    def n_gain(self) -> int:
        """The gain table's length by default: the largest grade + 1, at least 2, at most 32 (higher grades clamp to 31)"""
        return min(max(self.max_grade + 1, 2), _capi.SRX_EVAL_MAX_GAIN)

    @classmethod
    def from_arrays(cls, rows, docs, grades, n_rows: Optional[int] = None, device=None, query_ids=None) -> "Judgments":
        """Integer triples: judgment i says that doc ``docs[i]`` has the grade ``grades[i]`` for the query of row ``rows[i]``, in
        any order.  ``n_rows``: the number of judged queries (None: the largest row + 1); a row without a triple is a judged
        query without a judged doc.  ValueError: arrays of different lengths or no integers, a row outside [0, n_rows), a doc
        id or grade outside int32, a (row, doc) pair twice."""
        arrs = [np.asarray(a) for a in (rows, docs, grades)]
        if any(a.ndim != 1 or (len(a) and a.dtype.kind not in "iu") for a in arrs) or not (len(arrs[0]) == len(arrs[1]) == len(arrs[2])):
            raise ValueError("rows, docs and grades must be 1-D integer arrays of one length")
        rows, docs, grades = (a.astype(np.int64) for a in arrs)
        n_rows = (int(rows.max()) + 1 if len(rows) else 0) if n_rows is None else int(n_rows)
        if n_rows < 0 or n_rows > 2 ** 31 - 1:
            raise ValueError(f"n_rows must be in [0, 2^31 - 1], got {n_rows}")
        if len(rows) and (rows.min() < 0 or rows.max() >= n_rows):
            raise ValueError(f"a judgment's row must be in [0, {n_rows})")
        for a, what in ((docs, "doc id"), (grades, "grade")):
            if len(a) and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
                raise ValueError(f"a {what} must fit int32")
        order = np.lexsort((docs, rows))
        rows, docs, grades = rows[order], docs[order], grades[order]
        same = (rows[1:] == rows[:-1]) & (docs[1:] == docs[:-1])
        if same.any():
            i = int(np.flatnonzero(same)[0])
            raise ValueError(f"row {int(rows[i])} judges doc {int(docs[i])} twice")
        j_ptr = np.zeros(n_rows + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows, minlength=n_rows), out=j_ptr[1:])
        ideal = grades[np.lexsort((-grades, rows))]  # inside a row: grade descending
        return cls(j_ptr, docs.astype(np.int32), grades.astype(np.int32), ideal.astype(np.int32), device=device, query_ids=query_ids)

    @classmethod
    def from_qrels(cls, qrels: Dict[str, Dict[str, int]], query_ids: Optional[Sequence[str]], doc_ids: Sequence[str], device=None) -> "Judgments":
        """``qrels`` = BEIR's / pytrec_eval's ``{qid: {doc_id: int grade}}``.  Row r is the query ``query_ids[r]`` (None: the keys of
        ``qrels`` in their order); a query id without an entry in ``qrels`` gets an empty row, an entry of ``qrels`` outside
        ``query_ids`` is left out.  A doc is the row of its id in ``doc_ids`` (the corpus order of the index: its GLOBAL id).

        A judged doc id that is NOT in the corpus still counts towards R and the ideal ranking -- it can never be retrieved but it
        is still relevant, so recall and nDCG must not forget it.  It is stored with an id >= ``len(doc_ids)``, assigned past the
        corpus in the order of first appearance (``extra_ids``).

        ValueError: a grade that is no int, a doc id twice in one row (a ``{doc_id: grade}`` dict cannot hold one; a row given as
        a list of ``(doc_id, grade)`` pairs can), a query id twice in ``query_ids``."""
        query_ids = list(qrels) if query_ids is None else list(query_ids)
        if len(set(query_ids)) != len(query_ids):
            raise ValueError("query_ids holds a query id twice")
        doc_rows = doc_ids if isinstance(doc_ids, dict) else {d: i for i, d in enumerate(doc_ids)}
        n_docs, extra = len(doc_rows), {}
        rows, docs, grades = [], [], []
        for r, qid in enumerate(query_ids):
            row = qrels.get(qid, {})
            pairs = list(row.items()) if isinstance(row, dict) else [tuple(p) for p in row]
            seen = set()
            for d, g in pairs:
                if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
                    raise ValueError(f"qrels[{qid!r}][{d!r}]: a grade must be an int, got {g!r}")
                if d in seen:
                    raise ValueError(f"qrels[{qid!r}] judges {d!r} twice")
                seen.add(d)
                i = doc_rows.get(d)
                if i is None:
                    i = extra.setdefault(d, n_docs + len(extra))
                rows.append(r), docs.append(i), grades.append(int(g))
        j = cls.from_arrays(np.asarray(rows, dtype=np.int64), np.asarray(docs, dtype=np.int64), np.asarray(grades, dtype=np.int64),
                            n_rows=len(query_ids), device=device, query_ids=query_ids)
        j.extra_ids, j.doc_rows = extra, doc_rows
        return j

    # -- device ---------------------------------------------------------------------------------------------------------
    def _need_device(self):
        if self.device is None:
            raise ValueError("these Judgments were built without a device: pass device= to from_qrels / from_arrays")
        torch = _torch()
        if self._dev is None:
            dev = torch.device(self.device)
            pad = lambda a: a if len(a) else np.zeros(1, dtype=a.dtype)  # a NULL array is refused: an empty one keeps one word
            self._dev = tuple(torch.as_tensor(pad(a).copy(), device=dev) for a in (self.j_ptr, self.j_doc, self.j_grade, self.j_ideal))
        return torch

    def tables(self, gain: str, m: int, n_gain: Optional[int] = None):
        """``(gain f32[n_gain], discount f32[m])`` on the device, cached per (gain, n_gain, m)"""
        torch = self._need_device()
        n_gain = self.n_gain if n_gain is None else int(n_gain)
        key = (gain, n_gain, int(m))
        if key not in self._tables:
            g, d = gain_table(gain, n_gain), discount_table(m)
            self._tables[key] = (torch.as_tensor(g, device=torch.device(self.device)), torch.as_tensor(d, device=torch.device(self.device)))
        return self._tables[key]

    def evaluate_device(self, doc, count, ks, q_rows=None, gain: str = "linear", rel_level: int = 1, means: bool = True,
                        n_gain: Optional[int] = None) -> EvalResult:
        """``srx_eval_lists`` on device tensors: ``doc`` int32 [nq, m] GLOBAL doc ids in rank order, ``count`` int32 [nq] or None
        (every position is live), as ``DeviceIndex.search_device``, the fusion and the ``*_topk`` stages return them; ``ks`` 1 to 8
        ascending cutoffs; ``q_rows`` int32 [nq] or None (list q belongs to row q): the judgment row of every list, -1 = not
        judged (all zeros, left out of the means).  ``gain`` "linear" | "exp2", over ``n_gain`` grades (None: :attr:`n_gain`);
        relevant = grade >= ``rel_level``.  Returns an :class:`EvalResult` of device tensors; asynchronous on the current stream,
        one launch, plus two small ones with ``means``.  ValueError: a tensor of another dtype, shape or device, m above 2 048,
        what the header refuses."""
        torch = self._need_device()
        dev = torch.device(self.device)
        ks = check_cutoffs(ks)
        if int(rel_level) < 1:
            raise ValueError(f"rel_level must be >= 1, got {rel_level}")
        if not (torch.is_tensor(doc) and doc.dtype == torch.int32 and doc.dim() == 2 and doc.is_contiguous() and doc.device == dev):
            raise ValueError(f"doc must be a contiguous int32 tensor [nq, m] on {dev}")
        nq, m = int(doc.shape[0]), int(doc.shape[1])
        if not (1 <= m <= _capi.SRX_EVAL_MAX_M):
            raise ValueError(f"lists of 1 to {_capi.SRX_EVAL_MAX_M} positions are evaluated, got m={m}")
        for t, what in ((count, "count"), (q_rows, "q_rows")):
            if t is not None and not (torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == (nq,) and t.is_contiguous() and t.device == dev):
                raise ValueError(f"{what} must be None or a contiguous int32 tensor [nq] on {dev}")
        g_tab, d_tab = self.tables(gain, m, n_gain)
        n_k = len(ks)
        with torch.cuda.device(dev):
            out = torch.empty((nq, n_k, _capi.SRX_EVAL_METRICS), dtype=torch.float32, device=dev)
            hits, judged = torch.empty((nq, n_k), dtype=torch.int32, device=dev), torch.empty((nq, n_k), dtype=torch.int32, device=dev)
            rel = torch.empty((nq,), dtype=torch.int32, device=dev)
            mean = n = ws = None
            ws_bytes = 0
            if means:
                mean, n = torch.zeros((n_k, _capi.SRX_EVAL_METRICS), dtype=torch.float64, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
                ws_bytes = int(_capi.lib().srx_eval_workspace_bytes(nq, n_k))
                ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.float64, device=dev)
            rc = _capi.lib().srx_eval_lists(dev.index or 0, *[_ptr(t) if self.n_rows else None for t in self._dev], self.n_rows, self.nnz,
                                            _ptr(g_tab), len(g_tab), _ptr(d_tab), int(rel_level), _ptr(doc), _ptr(count), _ptr(q_rows), nq, m,
                                            (ctypes.c_int32 * n_k)(*ks), n_k, _ptr(out), _ptr(hits), _ptr(judged), _ptr(rel), _ptr(mean), _ptr(n),
                                            _ptr(ws), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
            _capi.check(rc, "srx_eval_lists")
        return EvalResult(out, hits, judged, rel, mean, n)

    def evaluate(self, doc, count=None, ks=DEFAULT_K_VALUES, q_rows=None, gain: str = "linear", rel_level: int = 1, means: bool = True,
                 n_gain: Optional[int] = None) -> EvalResult:
        """Host arrays in (``doc`` int [nq, m], ``count`` / ``q_rows`` int [nq] or None), host arrays out: :meth:`evaluate_device`
        with one upload, one synchronisation and one copy back (``n`` an int)."""
        torch = self._need_device()
        dev = torch.device(self.device)
        doc = np.ascontiguousarray(doc, dtype=np.int32)
        if doc.ndim != 2:
            raise ValueError("doc must be an int array [nq, m]")
        up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev)
        res = self.evaluate_device(up(doc), up(count), ks, up(q_rows), gain, rel_level, means, n_gain)
        host = [None if t is None else t.cpu().numpy() for t in res]
        if host[5] is not None:
            host[5] = int(host[5][0])
        return EvalResult(*host)


# ---- the dict door --------------------------------------------------------------------------------------------------------
def lists_from_results(judgments: Judgments, results, complete: bool = False, ignore_identical_ids: bool = False, cap: int = _capi.SRX_EVAL_MAX_M):
    """``results`` = ``{qid: {doc_id: score}}`` as any search returns it -> ``(qids, doc int32 [nq, m], count int32 [nq], q_rows
    int32 [nq])`` for :meth:`Judgments.evaluate`.  Only the queries that are judged (a row of ``judgments``) AND have an entry in
    ``results`` are listed -- trec_eval's default; ``complete`` adds an EMPTY list for every judged query without an entry (its -c).
    A list is ordered by (score descending, doc id ascending in corpus order) -- the order the engine itself emits, whatever the
    order of the dict; a doc id outside the corpus sorts behind the corpus at an equal score, by its string; NaN scores come
    last.  ``ignore_identical_ids`` drops ``doc_id == qid`` before the ranking (BEIR's flag).  A list deeper than ``cap`` is cut
    there.  A doc outside the corpus that is judged keeps the id :meth:`Judgments.from_qrels` gave it, any other is -1 (never
    judged).  ``m`` is the deepest list's length, at least 1."""
    if judgments.row_of is None or judgments.doc_rows is None:
        raise ValueError("the dict door needs Judgments.from_qrels (query and doc ids)")
    n_docs, rows_of = len(judgments.doc_rows), judgments.doc_rows
    qids, lists = [], []
    for qid in (judgments.query_ids if complete else results):
        if qid not in judgments.row_of:
            continue
        keyed = []
        for d, s in (results.get(qid) or {}).items():
            if ignore_identical_ids and d == qid:
                continue
            i = rows_of.get(d)
            s = float(s)
            keyed.append((s != s, -s if s == s else 0.0, n_docs if i is None else i, str(d), judgments.extra_ids.get(d, -1) if i is None else i))
        keyed.sort(key=lambda t: t[:4])
        qids.append(qid)
        lists.append([t[4] for t in keyed[:cap]])
    m = max(max((len(l) for l in lists), default=0), 1)
    doc = np.full((len(lists), m), -1, dtype=np.int32)
    for i, l in enumerate(lists):
        doc[i, :len(l)] = l
    count = np.asarray([len(l) for l in lists], dtype=np.int32)
    q_rows = np.asarray([judgments.row_of[q] for q in qids], dtype=np.int32)
    return qids, doc, count, q_rows


def metrics_dicts(res: EvalResult, ks, qids=None):
    """An :class:`EvalResult` of host arrays with means -> ``{"NDCG@k": .., "MAP@k": .., "Recall@k": .., "P@k": .., "MRR@k": ..,
    "Success@k": .., "Judged@k": .., "n_queries": n}`` (BEIR's key spelling; the means of the device), and with ``qids`` also
    ``{qid: {the same keys without n_queries}}``.  ``Judged@k`` is the mean of ``judged / k`` over the evaluated queries, computed
    here in float64 (every listed query of the dict door is evaluated)."""
    agg = {}
    n = int(res.n)
    for ik, k in enumerate(ks):
        for name, plane in METRIC_KEYS:
            agg[f"{name}@{k}"] = float(res.mean[ik, plane])
        agg[f"Judged@{k}"] = float(np.sum(res.judged[:, ik].astype(np.float64) / float(k)) / n) if n else 0.0
    agg["n_queries"] = n
    if qids is None:
        return agg
    per = {}
    for q, qid in enumerate(qids):
        row = {}
        for ik, k in enumerate(ks):
            for name, plane in METRIC_KEYS:
                row[f"{name}@{k}"] = float(res.out[q, ik, plane])
            row[f"Judged@{k}"] = float(res.judged[q, ik]) / float(k)
        per[qid] = row
    return agg, per


def evaluate_results(qrels, results, doc_ids, device, k_values=DEFAULT_K_VALUES, *, gain: str = "linear", rel_level: int = 1, per_query: bool = False,
                     complete: bool = False, ignore_identical_ids: bool = False):
    """The dict door: ``qrels`` = ``{qid: {doc_id: grade}}`` (or a :class:`Judgments` of :meth:`Judgments.from_qrels`, built once
    and reused), ``results`` = ``{qid: {doc_id: score}}``, ``doc_ids`` the corpus order -> :func:`metrics_dicts`.  One upload of the
    lists, one call of ``srx_eval_lists``, one copy back."""
    ks = check_cutoffs(k_values, cap=_capi.SRX_EVAL_MAX_M)
    if gain not in GAINS:
        raise ValueError(f"gain must be one of {list(GAINS)}, got {gain!r}")
    judgments = qrels if isinstance(qrels, Judgments) else Judgments.from_qrels(qrels, None, doc_ids, device=device)
    qids, doc, count, q_rows = lists_from_results(judgments, results, complete, ignore_identical_ids)
    res = judgments.evaluate(doc, count, ks, q_rows, gain, rel_level, means=True)
    return metrics_dicts(res, ks, qids if per_query else None)
