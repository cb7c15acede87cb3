"""Relevance feedback (include/ext/sparse_rx_feedback.h): a resident doc-major forward index and the expansion of a query batch
from ranked feedback docs on the GPU -- RM3 for BM25, Rocchio-style for learned-sparse indexes, more-like-this with the docs as
the whole query.  The reference has no feedback: nothing here mirrors reference code.

The engine's own index is term-major; :class:`ForwardIndex` is the opt-in second structure that says which terms a doc holds:
8 bytes per posting plus 8 per doc (12 with doc lengths).  ``srx_feedback_expand`` reads it and leaves an expanded CSR batch on
the device, which ``DeviceIndex.search_device`` takes as it is."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _capi
from .index import _ptr, _stream_ptr, _torch, validate_candidates, validate_query_batch

DOC_WEIGHTS = {"score": _capi.SRX_FB_BY_SCORE, "uniform": _capi.SRX_FB_UNIFORM}
TERM_WEIGHTS = {"rm": _capi.SRX_FB_RM, "raw": _capi.SRX_FB_RAW}


def forward_order(torch, rows, term, value, idf):
    """The permutation that puts COO entries into forward-index order: row ascending; inside a row
    ``key = f32(value * idf[term])`` descending, then term ascending.  Keys compare as floats (-0 equals +0).  Three stable
    sorts; ``np.lexsort((term, -key, row))`` is the restatement."""
    key = value * idf[term.long()]
    o = torch.sort(term, stable=True).indices
    o = o[torch.sort(key[o], descending=True, stable=True).indices]
    return o[torch.sort(rows[o], stable=True).indices]


def check_expand_args(expand_docs, expand_terms, expand_weight, expand_by="score", what: str = "expand_docs"):
    """The expansion keywords of the API doors, or ``ValueError``: ``expand_docs`` in 1..32, ``expand_terms`` in 1..128,
    ``expand_weight`` in [0, 1], ``expand_by`` "score" or "uniform".  Returns them as (int, int, float, str)."""
    if isinstance(expand_docs, bool) or int(expand_docs) != expand_docs or not 1 <= int(expand_docs) <= _capi.SRX_FEEDBACK_MAX_DOCS:
        raise ValueError(f"{what} must be in [1, {_capi.SRX_FEEDBACK_MAX_DOCS}], got {expand_docs!r}")
    if isinstance(expand_terms, bool) or int(expand_terms) != expand_terms or not 1 <= int(expand_terms) <= _capi.SRX_FEEDBACK_MAX_TERMS:
        raise ValueError(f"expand_terms must be in [1, {_capi.SRX_FEEDBACK_MAX_TERMS}], got {expand_terms!r}")
    w = float(expand_weight)
    if not 0.0 <= w <= 1.0:  # a NaN fails both
        raise ValueError(f"expand_weight must be in [0, 1], got {expand_weight!r}")
    if expand_by not in DOC_WEIGHTS:
        raise ValueError(f"expand_by must be 'score' or 'uniform', got {expand_by!r}")
    return int(expand_docs), int(expand_terms), w, expand_by


class ForwardIndex:
    """The docs' (term, value) rows resident on one GPU: ``row_ptr`` i64[n_docs + 1], ``term`` i32[nnz], ``value`` f32[nnz] (the
    CSR's data: tf, or the learned weight), ``doc_len`` f32[n_docs] or None, and the host int ``max_row_terms``.  The first L
    entries of a row are the L terms that characterise the doc best (Lucene more-like-this's tf * idf)."""

    def __init__(self, row_ptr, term, value, doc_len, n_docs: int, vocab: int, doc_base: int, max_row_terms: int, device):
        self.row_ptr, self.term, self.value, self.doc_len = row_ptr, term, value, doc_len
        self.n_docs, self.vocab, self.doc_base, self.max_row_terms, self.device = int(n_docs), int(vocab), int(doc_base), int(max_row_terms), device
        self._ws = None
        self._desc = _capi.ForwardDesc(device=device.index or 0, reserved=0, n_docs=self.n_docs, vocab=self.vocab, doc_base=self.doc_base,
                                       row_ptr=_ptr(row_ptr), term=_ptr(term), value=_ptr(value), doc_len=_ptr(doc_len))

    @classmethod
    def from_csr(cls, indptr, indices, data, idf, *, doc_lengths=None, device="cuda:0", doc_base: int = 0) -> "ForwardIndex":
        """Build from a doc-major CSR (host numpy or device torch arrays) and the idf the row order is taken under."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise _capi.SparseRxUnavailable("no HIP device visible: ForwardIndex needs a GPU (there is no CPU fallback)")
        _capi.lib()
        dev = torch.device(device)

        def to_dev(x, dtype):
            if isinstance(x, torch.Tensor):
                return x.to(device=dev, dtype=dtype)
            return torch.as_tensor(np.ascontiguousarray(x), device=dev).to(dtype)

        with torch.cuda.device(dev):
            row_ptr = to_dev(indptr, torch.int64).contiguous()
            term, value, idf_d = to_dev(indices, torch.int32), to_dev(data, torch.float32), to_dev(idf, torch.float32)
            n_docs, vocab = row_ptr.numel() - 1, idf_d.numel()
            if n_docs < 1 or vocab < 1 or vocab > 1 << 26:
                raise ValueError(f"a forward index needs n_docs >= 1 and 1 <= vocab <= 2^26, got {n_docs} docs and {vocab} terms")
            if term.numel() != value.numel() or int(row_ptr[-1]) != term.numel() or int(row_ptr[0]) != 0:
                raise ValueError("indptr must run from 0 to len(indices) == len(data)")
            if term.numel() and (int(term.min()) < 0 or int(term.max()) >= vocab):
                raise ValueError(f"indices out of range [0, {vocab})")
            counts = row_ptr[1:] - row_ptr[:-1]
            rows = torch.repeat_interleave(torch.arange(n_docs, device=dev, dtype=torch.int32), counts)
            o = forward_order(torch, rows, term, value, idf_d)
            dl = None
            if doc_lengths is not None:
                dl = to_dev(doc_lengths, torch.float32).contiguous()
                if dl.numel() != n_docs:
                    raise ValueError(f"doc_lengths has {dl.numel()} entries for {n_docs} docs")
            longest = int(counts.max()) if n_docs else 0
            return cls(row_ptr, term[o].contiguous(), value[o].contiguous(), dl, n_docs, vocab, doc_base, longest, dev)

    def device_bytes(self) -> int:
        ts = [self.row_ptr, self.term, self.value, self.doc_len]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    def close(self) -> None:
        self.row_ptr = self.term = self.value = self.doc_len = self._ws = self._desc = None

    def default_row_cap(self, fb_docs: int) -> int:
        return max(1, min(self.max_row_terms, _capi.SRX_FEEDBACK_MAX_ENTRIES // int(fb_docs)))

    def expand_device(self, q_ptr, q_term, q_weight, fb_doc, fb_score=None, fb_count=None, *, fb_docs: int, n_terms: int = 10,
                      row_cap: Optional[int] = None, alpha: float = 0.5, beta: float = 0.5, doc_weight: str = "score", term_weight: str = "rm",
                      term_gain=None, out=None):
        """``srx_feedback_expand`` on device tensors: q_ptr i32[nq + 1], q_term i32, q_weight f32 as ``search_device`` takes them;
        fb_doc i32[nq, m] GLOBAL ids, fb_score f32[nq, m] (None under "uniform"), fb_count i32[nq] or None -- the triple of any
        search as it is; term_gain f32[vocab] or None.  Returns ``(e_ptr i32[nq + 1], e_term i32[cap], e_weight f32[cap], flag
        i32[1])`` on the device with cap = the host bound ``q_term.numel() + nq * n_terms`` (entries at or behind ``e_ptr[nq]``
        are not written): a batch ``search_device`` takes.  Bit 0 of ``flag`` = a query of more than 128 terms was copied through.
        Asynchronous on the current stream, no synchronisation.  Preconditions (NOT checked, the tensors never leave the device):
        those of ``search_device``.  ``row_cap`` None: ``min(max_row_terms, 4096 // fb_docs)``."""
        torch = _torch()
        if self._desc is None:
            raise ValueError("the forward index is closed")
        if doc_weight not in DOC_WEIGHTS or term_weight not in TERM_WEIGHTS:
            raise ValueError(f"doc_weight must be 'score' or 'uniform' and term_weight 'rm' or 'raw', got {doc_weight!r} / {term_weight!r}")
        nq = q_ptr.numel() - 1
        if q_ptr.dtype != torch.int32 or q_term.dtype != torch.int32 or q_weight.dtype != torch.float32 or nq < 0:
            raise ValueError("expand_device: q_ptr / q_term must be int32 tensors and q_weight a float32 tensor")
        if fb_doc.dim() != 2 or int(fb_doc.shape[0]) != nq or fb_doc.dtype != torch.int32 or int(fb_doc.shape[1]) < 1:
            raise ValueError("expand_device: fb_doc must be an int32 tensor [nq, m >= 1]")
        if fb_score is not None and (fb_score.dtype != torch.float32 or tuple(fb_score.shape) != tuple(fb_doc.shape)):
            raise ValueError("expand_device: fb_score must be a float32 tensor of fb_doc's shape")
        if fb_count is not None and (fb_count.dtype != torch.int32 or fb_count.numel() != nq):
            raise ValueError("expand_device: fb_count must be an int32 tensor [nq]")
        if term_gain is not None and (term_gain.dtype != torch.float32 or term_gain.numel() != self.vocab):
            raise ValueError("expand_device: term_gain must be a float32 tensor [vocab]")
        q_nnz, m = int(q_term.numel()), int(fb_doc.shape[1])
        par = _capi.FeedbackParams(fb_docs=int(fb_docs), row_cap=self.default_row_cap(fb_docs) if row_cap is None else int(row_cap),
                                   n_terms=int(n_terms), doc_weight=DOC_WEIGHTS[doc_weight], term_weight=TERM_WEIGHTS[term_weight],
                                   alpha=float(alpha), beta=float(beta))
        cap = q_nnz + nq * max(int(n_terms), 0)
        with torch.cuda.device(self.device):
            if out is None:
                out = (torch.empty(nq + 1, dtype=torch.int32, device=self.device), torch.empty(max(cap, 1), dtype=torch.int32, device=self.device),
                       torch.empty(max(cap, 1), dtype=torch.float32, device=self.device), torch.empty(1, dtype=torch.int32, device=self.device))
            e_ptr, e_term, e_weight, flag = out
            L = _capi.lib()
            need = max(int(L.srx_feedback_workspace_bytes(max(nq, 0))), 16)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            fb_doc = fb_doc.contiguous()
            fb_score = None if fb_score is None else fb_score.contiguous()
            rc = L.srx_feedback_expand(ctypes.byref(self._desc), ctypes.byref(par), _ptr(term_gain), _ptr(q_ptr), _ptr(q_term), _ptr(q_weight), nq,
                                       q_nnz, _ptr(fb_doc), _ptr(fb_score), _ptr(fb_count), m, e_ptr.data_ptr(), e_term.data_ptr(),
                                       e_weight.data_ptr(), e_term.numel(), flag.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                       _stream_ptr(torch, self.device))
            _capi.check(rc, "srx_feedback_expand")
            if nq == 0:
                e_ptr.zero_(), flag.zero_()
        return e_ptr, e_term, e_weight, flag

    def expand(self, q_ptr, q_term, q_weight, fb_doc, fb_score=None, fb_count=None, *, term_gain=None, **kw):
        """Host arrays in, host arrays out: ``(e_ptr i32[nq + 1], e_term i32[e_ptr[-1]], e_weight f32[e_ptr[-1]], flag int)``.  The
        batch is validated like ``DeviceIndex.search``'s (:func:`~.index.validate_query_batch`), the feedback block like a candidate
        block (:func:`~.index.validate_candidates`); then one call, one synchronisation, one copy."""
        torch = _torch()
        validate_query_batch(q_ptr, q_term, q_weight, self.vocab)
        nq = len(q_ptr) - 1
        fb_doc, fb_count = validate_candidates(fb_doc, fb_count, nq)
        n = int(np.asarray(q_ptr)[-1])
        if fb_score is not None:
            fb_score = np.ascontiguousarray(fb_score, dtype=np.float32)
            if fb_score.shape != fb_doc.shape:
                raise ValueError("fb_score must have fb_doc's shape")
        if term_gain is not None:
            term_gain = np.ascontiguousarray(term_gain, dtype=np.float32)
            if term_gain.shape != (self.vocab,):
                raise ValueError(f"term_gain must be a float32 array [{self.vocab}]")
        t = lambda x, dt: None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=dt), device=self.device)
        out = self.expand_device(t(q_ptr, np.int32), t(np.asarray(q_term)[:n], np.int32), t(np.asarray(q_weight)[:n], np.float32), t(fb_doc, np.int32),
                                 t(fb_score, np.float32), t(fb_count, np.int32), term_gain=t(term_gain, np.float32), **kw)
        torch.cuda.synchronize(self.device)
        e_ptr, e_term, e_weight, flag = (x.cpu().numpy() for x in out)
        return e_ptr, e_term[: int(e_ptr[-1])], e_weight[: int(e_ptr[-1])], int(flag[0])
