"""Graph dense index (include/graph/sparse_rx_graph.h): a fixed-degree neighbour graph over the half index's rows, walked by a beam
search in one launch.  No reference counterpart.  The contract is exact: :meth:`GraphHalfIndex.search` returns what the walk of the
header reaches, with ``DenseHalfIndex``'s score bits; which docs it reaches is the approximation.  The build starts from the
existing searches (k-nearest lists by ``srx_dense_search_half`` or a temporary ``IvfHalfIndex``), then ``srx_graph_prune`` (the
CAGRA rank rule) and ``srx_graph_merge`` (reverse edges).  The metric is the inner product: normalise the rows for cosine."""
import ctypes

import numpy as np

from . import _capi
from .dense import HALF_TYPES, DenseHalfIndex, _DenseIndex, check_half_dtype
from .filter import host_q_filter, resolve_filter
from .index import _empty_topk, _ptr, _stream_ptr, _torch


def check_degree(degree) -> int:
    if int(degree) not in _capi.SRX_GRAPH_DEGREES:
        raise ValueError(f"degree must be 16, 32 or 64, got {degree}")
    return int(degree)


def default_max_iter(n_seed: int, width: int, degree: int) -> int:
    """The largest ``max_iter`` within the visit budget of the header, capped at 64."""
    return max(1, min(64, (_capi.SRX_GRAPH_BUDGET - int(n_seed)) // (int(width) * int(degree))))


def knn_score_offset(max_row_norm: float) -> float:
    """The ``score_offset`` of the build's k-nearest searches: above the largest |score| of two rows (Cauchy-Schwarz), so every
    value is positive and a list is as long as the corpus allows."""
    return float(max_row_norm ** 2 * 1.01 + 1.0)


def _i32_matrix(torch, x, what: str):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.int32 or x.dim() != 2:
        raise ValueError(f"{what} must be a 2-D int32 device tensor")
    return x.contiguous()


def prune_device(knn, degree: int):
    """``srx_graph_prune``: knn i32[n, d0] (local ids, best first) -> i32[n, degree], the entries with the fewest detours;
    asynchronous."""
    torch, L = _torch(), _capi.lib()
    knn = _i32_matrix(torch, knn, "knn")
    n, d0 = int(knn.shape[0]), int(knn.shape[1])
    with torch.cuda.device(knn.device):
        out = torch.empty((n, check_degree(degree)), dtype=torch.int32, device=knn.device)
        _capi.check(L.srx_graph_prune(knn.device.index or 0, _ptr(knn), n, d0, degree, _ptr(out), _stream_ptr(torch, knn.device)), "srx_graph_prune")
    return out


def reverse_lists(fwd):
    """The CSR of the edges INTO each node: (rev_ptr i64[n + 1], rev_src i32[edges]), a node's sources ordered by (position of the
    node in the source's row, source) -- one stable sort of the targets taken in (position, source) order, and a bincount."""
    torch = _torch()
    n, degree = int(fwd.shape[0]), int(fwd.shape[1])
    dst = fwd.t().contiguous().view(-1).long()  # entry j * n + x: the target at position j of source x
    src = torch.arange(n, device=fwd.device, dtype=torch.int32).repeat(degree)
    live = (dst >= 0) & (dst < n)
    dst, src = dst[live], src[live]
    dst, order = torch.sort(dst, stable=True)
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=fwd.device)
    ptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    rev = src[order].contiguous()
    return ptr, rev if rev.numel() else torch.zeros(1, dtype=torch.int32, device=fwd.device)


def merge_device(fwd, rev_ptr=None, rev_src=None):
    """``srx_graph_merge``: fwd i32[n, degree] and its reverse lists (:func:`reverse_lists` when not given) -> i32[n, degree];
    asynchronous."""
    torch, L = _torch(), _capi.lib()
    fwd = _i32_matrix(torch, fwd, "fwd")
    n, degree = int(fwd.shape[0]), check_degree(fwd.shape[1])
    with torch.cuda.device(fwd.device):
        if rev_ptr is None:
            rev_ptr, rev_src = reverse_lists(fwd)
        out = torch.empty_like(fwd)
        _capi.check(L.srx_graph_merge(fwd.device.index or 0, _ptr(fwd), n, degree, _ptr(rev_ptr), _ptr(rev_src), _ptr(out), _stream_ptr(torch, fwd.device)),
                    "srx_graph_merge")
    return out


class GraphHalfIndex(_DenseIndex):
    """The half index's rows (f16 / bf16, MFMA-fragment order, packed once by ``DenseHalfIndex``: no second copy, no permutation)
    and ``graph`` i32[n_docs, degree] of shard-local row numbers padded with -1."""

    _score_entry = "srx_dense_score_docs_half"
    default_itopk, default_width = 64, 4  # what search / search_device read when itopk / width are not given (RetrievalService sets them)

    def __init__(self, embeddings, degree: int = 32, dtype="f16", knn=None, graph=None, build_degree=None, builder: str = "ivf", nprobe: int = 8,
                 doc_base: int = 0, device="cuda:0"):
        """``embeddings``: f32[n_docs, dim], as ``DenseHalfIndex`` takes them.  ``graph`` i32[n_docs, degree] is taken as it is;
        otherwise ``knn`` i32[n_docs, d0] (local ids, best first) or the lists of ``builder`` -- "exact": chunks of rows as queries
        of ``srx_dense_search_half``; "ivf": the same through a temporary ``IvfHalfIndex`` (``nprobe`` of about sqrt(n_docs)
        lists) -- with ``k = build_degree + 1`` (default ``2 * degree``; the self hit is dropped by the prune) go through
        :func:`prune_device` and :func:`merge_device`."""
        self.dtype, self.degree = check_half_dtype(dtype), check_degree(degree)
        if builder not in ("exact", "ivf"):
            raise ValueError(f"builder must be 'exact' or 'ivf', got {builder!r}")
        torch = self._open(device)
        self._rows = DenseHalfIndex(embeddings, dtype=self.dtype, device=device, doc_base=doc_base)
        self.n_docs, self.dim, self.dim_pad, self.doc_base, self.corpus = self._rows.n_docs, self._rows.dim, self._rows.dim_pad, self._rows.doc_base, self._rows.corpus
        self.build_seconds = {}
        with torch.cuda.device(self.device):
            if graph is None:
                if knn is None:
                    d0 = min(2 * self.degree if build_degree is None else int(build_degree), _capi.SRX_GRAPH_MAX_D0)
                    if d0 < self.degree:
                        raise ValueError(f"build_degree must be in [degree, {_capi.SRX_GRAPH_MAX_D0}], got {build_degree}")
                    knn = self._timed("knn", lambda: self._knn(torch, embeddings, d0 + 1, builder, int(nprobe)))
                knn = torch.as_tensor(np.ascontiguousarray(knn, dtype=np.int32) if not isinstance(knn, torch.Tensor) else knn, device=self.device)
                if knn.dim() != 2 or int(knn.shape[0]) != self.n_docs:
                    raise ValueError(f"knn must be int32 [{self.n_docs}, d0], got {tuple(knn.shape)}")
                if int(knn.shape[1]) > _capi.SRX_GRAPH_MAX_D0:
                    knn = knn[:, : _capi.SRX_GRAPH_MAX_D0]  # build_degree + 1 = 129: the rank rule reads 128
                if int(knn.shape[1]) < self.degree:  # a corpus smaller than the degree: pad the lists
                    knn = torch.cat([knn, torch.full((self.n_docs, self.degree - int(knn.shape[1])), -1, dtype=torch.int32, device=self.device)], 1)
                pruned = self._timed("prune", lambda: prune_device(knn.to(torch.int32), self.degree))
                graph = self._timed("merge", lambda: merge_device(pruned))
            graph = torch.as_tensor(np.ascontiguousarray(graph, dtype=np.int32) if not isinstance(graph, torch.Tensor) else graph, device=self.device)
            if graph.dtype != torch.int32 or tuple(graph.shape) != (self.n_docs, self.degree):
                raise ValueError(f"graph must be int32 [{self.n_docs}, {self.degree}], got {graph.dtype} {tuple(graph.shape)}")
            self.graph = graph.contiguous()
        self._desc = _capi.GraphDesc(device=self.device.index or 0, type=HALF_TYPES[self.dtype], n_docs=self.n_docs, doc_base=self.doc_base,
                                     dim_pad=self.dim_pad, degree=self.degree, corpus=_ptr(self.corpus), graph=_ptr(self.graph))

    def _timed(self, stage, fn):
        import time
        torch = _torch()
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(self.device)
        self.build_seconds[stage] = time.perf_counter() - t0
        return out

    def _knn(self, torch, embeddings, k: int, builder: str, nprobe: int):
        """i32[n_docs, min(k, 1024)] local ids: every row as a query of its own corpus, in chunks; the offset keeps every value
        positive, so a list is as long as the corpus (or the probed lists) allows"""
        k = min(k, self.n_docs, _capi.SRX_MAX_K)
        off = knn_score_offset(self._rows.max_row_norm())
        src = self._rows
        if builder == "ivf" and self.n_docs >= 4096:  # below that the lists would be smaller than the neighbour lists
            from .ivf import IvfHalfIndex
            nlist = max(1, min(int(self.n_docs ** 0.5), _capi.SRX_IVF_MAX_LIST))
            src = IvfHalfIndex(embeddings, nlist, dtype=self.dtype, device=self.device, train_rows=min(self.n_docs, 256 * nlist))
            src.default_nprobe = max(1, min(nprobe, nlist))
        out = torch.empty((self.n_docs, k), dtype=torch.int32, device=self.device)
        step = 4096 if src is not self._rows else max(32, min(8192, (1 << 28) // max(self.n_docs, 1) // 32 * 32))  # exact: a 1 GiB score matrix
        for lo in range(0, self.n_docs, step):
            x = embeddings[lo: lo + step]
            x = x.to(self.device) if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, dtype=np.float32)).to(self.device)
            ids = src.search_device(x, k, score_offset=off)[0]
            out[lo: lo + step] = torch.where(ids >= 0, ids - src.doc_base, ids)
        return out  # the temporary index is freed with `src`

    # ---- what the index holds ----
    def device_bytes(self) -> int:
        """Bytes resident: the rows and the graph."""
        return int(self.corpus.numel() + 4 * self.graph.numel())

    def graph_to_host(self) -> np.ndarray:
        return self.graph.cpu().numpy()

    def corpus_to_host(self) -> np.ndarray:
        return self._rows.corpus_to_host()

    def max_row_norm(self) -> float:
        return self._rows.max_row_norm()

    # ---- doors ----
    def search_device(self, queries_f32, k: int, itopk=None, width=None, max_iter=None, seeds=None, score_offset: float = 0.0, filter=None,
                      q_filter=None, with_stats: bool = False):
        """f32[nq, dim] device queries -> (doc i32[nq,k], score f32[nq,k], count i32[nq]) of the walk (``srx_graph_search``), and with
        ``with_stats`` i32[nq, 2] (steps run, docs scored); asynchronous.  ``itopk`` None: ``default_itopk``, raised to ``k``
        rounded up to 32.  ``seeds``: None (``itopk`` rows spread evenly over the corpus), an int (that many spread rows) or an int32
        device tensor [nq, n_seed] of global ids.  ``max_iter`` None: :func:`default_max_iter`."""
        torch = _torch()
        if itopk is None:
            itopk = max(int(self.default_itopk), -(-int(k) // 32) * 32)
        width = int(self.default_width if width is None else width)
        nq = int(queries_f32.shape[0])
        seed_t = None
        if seeds is None or isinstance(seeds, (int, np.integer)):
            n_seed = int(min(int(itopk), _capi.SRX_GRAPH_MAX_SEED) if seeds is None else seeds)
        else:
            if not isinstance(seeds, torch.Tensor) or seeds.dtype != torch.int32 or seeds.dim() != 2 or int(seeds.shape[0]) != nq or seeds.device != self.device:
                raise ValueError(f"seeds must be an int or an int32 tensor [{nq}, n_seed] on {self.device}")
            seed_t, n_seed = seeds.contiguous(), int(seeds.shape[1])
        if max_iter is None:
            max_iter = default_max_iter(n_seed, width, self.degree)
        with torch.cuda.device(self.device):
            q = self._padded(torch, queries_f32, torch.float32)
            out = _empty_topk(torch, nq, max(int(k), 1), self.device)
            stat = torch.empty((nq, 2), dtype=torch.int32, device=self.device) if with_stats else None
            fdesc, keep = resolve_filter(self, filter, q_filter, nq)  # keep: alive until the call has been issued
            _capi.check(_capi.lib().srx_graph_search(ctypes.byref(self._desc), _ptr(q), nq, int(itopk), width, int(max_iter), _ptr(seed_t), n_seed, int(k), fdesc,
                                                     _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(stat), _stream_ptr(torch, self.device), float(score_offset)),
                        "srx_graph_search")
        return (*out, stat) if with_stats else out

    def search(self, queries: np.ndarray, k: int, itopk=None, width=None, max_iter=None, seeds=None, score_offset: float = 0.0, filter=None, q_filter=None,
               with_stats: bool = False):
        """Host arrays in, host arrays out; ``seeds`` may be a host i32[nq, n_seed]; ``q_filter``: a host sequence of row numbers."""
        q = self._rows._queries_to_device(queries)
        if seeds is not None and not isinstance(seeds, (int, np.integer)):
            seeds = _torch().as_tensor(np.ascontiguousarray(seeds, dtype=np.int32), device=self.device)
        return self._host(self.search_device(q, k, itopk, width, max_iter, seeds, score_offset, filter=filter,
                                             q_filter=host_q_filter(self, filter, q_filter, int(q.shape[0])), with_stats=with_stats))

    def score_docs_device(self, queries_f32, cand_doc, cand_count=None, out=None):
        """``DenseHalfIndex.score_docs_device`` on the same rows."""
        return self._rows.score_docs_device(queries_f32, cand_doc, cand_count, out)

    def score_docs(self, queries: np.ndarray, cand_doc, cand_count=None) -> np.ndarray:
        return self._rows.score_docs(queries, cand_doc, cand_count)
