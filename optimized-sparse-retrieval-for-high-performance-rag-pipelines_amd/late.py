"""Late-interaction reranking (include/sparse_rx_maxsim.h): a token-vector store resident in HBM and the MaxSim scores of
given (query, doc) pairs over it -- ``score = sum over the live query tokens of the largest similarity to any token of the
doc`` -- with the top-k of a candidate list by them.  No reference counterpart: it has no reranker.

The token rows of all docs are the rows of ONE :class:`~.dense.DenseHalfIndex` (``TokenIndex.tokens``): its
``score_docs_device`` of a query token against a token row IS the similarity the MaxSim kernel computes, bit for bit.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from . import _capi
from .dense import HALF_TYPES, DenseHalfIndex, _require_f32, check_half_dtype
from .index import _candidate_block, _empty_topk, _grow_ws, _ptr, _stream_ptr, _to_host, _torch, pool_depth, validate_candidates

LATE_MAX_M = _capi.SRX_MAX_K  # candidates per list of the rerank form


def check_late_shape(tq: int, dim_pad: int, m: Optional[int] = None, k=None) -> Optional[int]:
    """The shape rules of include/sparse_rx_maxsim.h on the host, or ``ValueError``: 1 <= tq <= 128 with
    ``ceil32(tq) * dim_pad <= 32768``; with ``m`` (the rerank form) 1 <= m <= 1024 and 1 <= k <= m.  Returns ``k`` as an int."""
    max_qt = _capi.SRX_MAXSIM_MAX_QT
    if not (1 <= tq <= max_qt):
        raise ValueError(f"a query holds 1 .. {max_qt} query tokens, got {tq}")
    if (tq + 31) // 32 * 32 * dim_pad > 32768:
        raise ValueError(f"{tq} query tokens of padded dim {dim_pad} exceed the limit ceil32(tq) * dim_pad <= 32768 "
                         f"(at most {32768 // dim_pad // 32 * 32} tokens at this dim)")
    if m is None:
        return None
    if not (1 <= m <= LATE_MAX_M):
        raise ValueError(f"a rerank list holds 1 .. {LATE_MAX_M} candidates per query, got m={m} (no silent truncation)")
    k = int(k)
    if not (1 <= k <= m):
        raise ValueError(f"k must be in [1, m={m}] for the rerank, got {k}")
    return k


def late_pool_depth(top_k: int, late_pool, n_docs: int) -> int:
    """Rows of the fused ranking a late-interaction rerank of ``top_k`` reorders (:func:`~.index.pool_depth`): ``late_pool`` in
    1 .. 1024, else ``min(max(top_k, 100), 1024)``."""
    return pool_depth("late_pool", late_pool, max(int(top_k), 100), LATE_MAX_M, n_docs)


def doc_token_ptr(doc_token_counts, n_tok: int) -> np.ndarray:
    """``tok_ptr`` i32[n_docs + 1] of per-doc token counts, or ``ValueError``: a 1-D integer sequence of at least one
    non-negative count whose sum is ``n_tok`` <= 2**31 - 2."""
    c = np.asarray(doc_token_counts)
    if c.ndim != 1 or c.size < 1 or c.dtype.kind not in "iu":
        raise ValueError("doc_token_counts must be a 1-D integer sequence with one count per doc (at least one doc)")
    c = c.astype(np.int64)
    if int(c.min()) < 0:
        raise ValueError("doc_token_counts holds a negative count")
    total = int(c.sum())
    if total != n_tok:
        raise ValueError(f"doc_token_counts sum to {total} but there are {n_tok} token rows")
    if total > 2 ** 31 - 2 or c.size > 2 ** 31 - 2:
        raise ValueError("at most 2**31 - 2 docs and token rows")
    ptr = np.zeros(c.size + 1, dtype=np.int64)
    np.cumsum(c, out=ptr[1:])
    return ptr.astype(np.int32)


class TokenIndex:
    """Token vectors of a corpus resident in HBM: ``tokens`` (a :class:`~.dense.DenseHalfIndex` whose rows are ALL token
    vectors, in fragment order) and ``tok_ptr`` (device i32[n_docs + 1]: doc d owns token rows tok_ptr[d] .. tok_ptr[d+1]-1)."""

    def __init__(self, tokens: DenseHalfIndex, tok_ptr, doc_base: int = 0):
        torch = _torch()
        self.tokens = tokens
        self.device = tokens.device
        self.dtype, self.dim, self.dim_pad = tokens.dtype, tokens.dim, tokens.dim_pad
        self.tok_ptr = torch.as_tensor(np.ascontiguousarray(tok_ptr, dtype=np.int32), device=self.device)
        self.n_docs = int(self.tok_ptr.numel()) - 1
        self.n_tokens = int(tokens.n_docs)
        self.doc_base = int(doc_base)
        if self.doc_base < 0:
            raise ValueError("doc_base must be >= 0")
        self._ws = None

    @classmethod
    def from_token_embeddings(cls, tok_emb, doc_token_counts, dtype="f16", device="cuda:0", doc_base: int = 0, chunk_rows=None):
        """``tok_emb`` f32[n_tok, dim]: the token vectors of doc 0, then of doc 1, ... (a device tensor or a host array, as
        :class:`~.dense.DenseHalfIndex` takes them; rounded to ``dtype`` by ``srx_dense_convert_half``);
        ``doc_token_counts``: tokens per doc (0 is legal).  ``ValueError`` for counts that do not sum to ``n_tok``, no token at
        all, or a non-finite token row."""
        check_half_dtype(dtype)
        _require_f32(tok_emb, "tok_emb")
        ptr = doc_token_ptr(doc_token_counts, int(tok_emb.shape[0]))
        if int(tok_emb.shape[0]) == 0:
            raise ValueError("a token index needs at least one token row")
        return cls(DenseHalfIndex(tok_emb, dtype=dtype, device=device, chunk_rows=chunk_rows), ptr, doc_base)

    def device_bytes(self) -> int:
        """Bytes of the resident token rows and of ``tok_ptr``."""
        return self.tokens.device_bytes() + int(self.tok_ptr.numel()) * 4

    def close(self) -> None:
        self.tokens = self.tok_ptr = self._ws = None

    # -- the two entry points ---------------------------------------------------------------------------------------------
    def _check_queries(self, torch, q_tok, q_tok_count):
        """``q_tok`` f32[nq, tq, dim] and ``q_tok_count`` i32[nq] / None checked: (nq, tq)"""
        if not isinstance(q_tok, torch.Tensor) or q_tok.dtype != torch.float32 or q_tok.dim() != 3:
            raise ValueError("query tokens must be a float32 tensor [nq, tq, dim]")
        nq, tq, dim = (int(x) for x in q_tok.shape)
        if dim != self.dim:
            raise ValueError(f"query tokens have dim {dim}, the token index has dim {self.dim}")
        check_late_shape(tq, self.dim_pad)
        if q_tok_count is not None and (q_tok_count.dtype != torch.int32 or q_tok_count.dim() != 1 or int(q_tok_count.numel()) != nq):
            raise ValueError("q_tok_count must be an int32 tensor [nq]")
        return nq, tq

    def _padded(self, torch, q_tok, q_tok_count):
        """The query tokens zero-padded to ``dim_pad`` and the counts, contiguous on the device"""
        if int(q_tok.shape[2]) == self.dim_pad:
            q = q_tok.to(self.device).contiguous()
        else:
            q = torch.zeros((int(q_tok.shape[0]), int(q_tok.shape[1]), self.dim_pad), dtype=torch.float32, device=self.device)
            q[:, :, : self.dim] = q_tok
        return q, (None if q_tok_count is None else q_tok_count.contiguous())

    def _head(self, q, q_tok_count, nq, tq, cand_doc, cand_count, m):
        return (self.device.index or 0, HALF_TYPES[self.dtype], _ptr(self.tokens.corpus), self.n_tokens, self.dim_pad, _ptr(self.tok_ptr),
                self.n_docs, self.doc_base, _ptr(q), _ptr(q_tok_count), nq, tq, _ptr(cand_doc), _ptr(cand_count), m)

    def score_docs_device(self, q_tok, q_tok_count, cand_doc, cand_count=None, out=None):
        """``srx_maxsim_score_docs_half``: the MaxSim score of every candidate of every query.  ``q_tok`` f32[nq, tq, dim]
        device tensor, ``q_tok_count`` i32[nq] or None (live tokens of each query), ``cand_doc`` i32[nq, m] GLOBAL ids (-1 and
        ids outside the index score +0), ``cand_count`` i32[nq] or None.  Returns f32[nq, m]; asynchronous on the current stream."""
        torch = _torch()
        L = _capi.lib()
        nq, tq = self._check_queries(torch, q_tok, q_tok_count)
        cand_doc, cand_count, m, out = _candidate_block(torch, nq, cand_doc, cand_count, out, self.device)
        with torch.cuda.device(self.device):
            q, qc = self._padded(torch, q_tok, q_tok_count)
            if nq > 0:
                ws = _grow_ws(torch, self, _capi.check(L.srx_maxsim_workspace_bytes(nq, tq, self.dim_pad, 0), "srx_maxsim_workspace_bytes"))
                _capi.check(L.srx_maxsim_score_docs_half(*self._head(q, qc, nq, tq, cand_doc, cand_count, m), _ptr(out), _ptr(ws), ws.numel(),
                                                         _stream_ptr(torch, self.device)), "srx_maxsim_score_docs_half")
        return out

    def rerank_device(self, q_tok, q_tok_count, cand_doc, cand_count, k: int):
        """``srx_maxsim_rerank_half``: the ``k`` best of every query's ``m <= 1024`` candidates by MaxSim score, (score
        descending, doc ascending), no ``> 0`` filter.  Inputs as :meth:`score_docs_device`; the (doc, score, count) triple of
        any search or of the fusion goes in as ``cand_doc`` / ``cand_count``.  Returns the device triple (doc i32[nq, k], score
        f32[nq, k], count i32[nq]), rows padded with -1 / 0; asynchronous on the current stream."""
        torch = _torch()
        L = _capi.lib()
        nq, tq = self._check_queries(torch, q_tok, q_tok_count)
        if cand_doc.dim() != 2 or int(cand_doc.shape[0]) != nq or cand_doc.dtype != torch.int32 or int(cand_doc.shape[1]) < 1:
            raise ValueError("rerank_device: cand_doc must be an int32 tensor [nq, m] with m >= 1")
        if cand_count is not None and (cand_count.dtype != torch.int32 or cand_count.numel() != nq):
            raise ValueError("rerank_device: cand_count must be an int32 tensor [nq]")
        m = int(cand_doc.shape[1])
        k = check_late_shape(tq, self.dim_pad, m, k)
        with torch.cuda.device(self.device):
            q, qc = self._padded(torch, q_tok, q_tok_count)
            cand_doc, cand_count = cand_doc.contiguous(), None if cand_count is None else cand_count.contiguous()
            out = _empty_topk(torch, nq, k, self.device)
            if nq > 0:
                ws = _grow_ws(torch, self, _capi.check(L.srx_maxsim_workspace_bytes(nq, tq, self.dim_pad, m), "srx_maxsim_workspace_bytes"))
                _capi.check(L.srx_maxsim_rerank_half(*self._head(q, qc, nq, tq, cand_doc, cand_count, m), k, _ptr(out[0]), _ptr(out[1]),
                                                     _ptr(out[2]), _ptr(ws), ws.numel(), _stream_ptr(torch, self.device)), "srx_maxsim_rerank_half")
        return out

    # -- host arrays in, host arrays out ----------------------------------------------------------------------------------
    def _host_inputs(self, q_tok, q_tok_count, cand_doc, cand_count):
        torch = _torch()
        q = np.ascontiguousarray(q_tok, dtype=np.float32)
        if q.ndim != 3:
            raise ValueError("query tokens must be [nq, tq, dim]")
        nq = int(q.shape[0])
        qc = None
        if q_tok_count is not None:
            qc = np.asarray(q_tok_count)
            if qc.ndim != 1 or qc.dtype.kind not in "iu" or len(qc) != nq:
                raise ValueError(f"q_tok_count must be a 1-D integer array of length {nq}")
            qc = torch.as_tensor(np.ascontiguousarray(qc, dtype=np.int32), device=self.device)
        cand_doc, cand_count = validate_candidates(cand_doc, cand_count, nq)
        cc = None if cand_count is None else torch.as_tensor(cand_count, device=self.device)
        return torch.as_tensor(q, device=self.device), qc, torch.as_tensor(cand_doc, device=self.device), cc

    def score_docs(self, q_tok, q_tok_count, cand_doc, cand_count=None) -> np.ndarray:
        """:meth:`score_docs_device` on host arrays: one synchronisation, one copy.  Returns f32[nq, m]."""
        return _to_host(_torch(), self.device, (self.score_docs_device(*self._host_inputs(q_tok, q_tok_count, cand_doc, cand_count)),))[0]

    def rerank(self, q_tok, q_tok_count, cand_doc, cand_count, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """:meth:`rerank_device` on host arrays: one synchronisation, one copy.  Returns host (doc, score, count)."""
        return _to_host(_torch(), self.device, self.rerank_device(*self._host_inputs(q_tok, q_tok_count, cand_doc, cand_count), k))


def stack_query_tokens(query_tokens, qids, dim: int) -> Tuple[np.ndarray, np.ndarray]:
    """``{qid: f32[t_q, dim]}`` for ``qids`` as one padded block: (f32[nq, tq, dim] with tq the longest query's tokens, at
    least 1; i32[nq] live counts).  ``ValueError``: a missing qid, a wrong shape, more than 128 tokens."""
    mats = []
    for qid in qids:
        if qid not in query_tokens:
            raise ValueError(f"no query tokens for {qid!r}")
        t = np.asarray(query_tokens[qid], dtype=np.float32)
        if t.ndim != 2 or t.shape[1] != dim:
            raise ValueError(f"query tokens of {qid!r} have shape {t.shape}, expected (t_q, {dim})")
        if t.shape[0] > _capi.SRX_MAXSIM_MAX_QT:
            raise ValueError(f"query {qid!r} has {t.shape[0]} query tokens, at most {_capi.SRX_MAXSIM_MAX_QT} are supported")
        mats.append(t)
    tq = max((t.shape[0] for t in mats), default=1) or 1
    block = np.zeros((len(mats), tq, dim), dtype=np.float32)
    counts = np.zeros(len(mats), dtype=np.int32)
    for i, t in enumerate(mats):
        block[i, : t.shape[0]] = t
        counts[i] = t.shape[0]
    return block, counts
