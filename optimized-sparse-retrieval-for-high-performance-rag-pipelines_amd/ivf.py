"""IVF dense index (include/ivf/sparse_rx_ivf.h): the half index's rows partitioned by k-means, a query reads only the
``nprobe`` lists whose centroids score highest.  No reference counterpart.  The contract is exact: :meth:`IvfHalfIndex.search`
returns the exact top k of the probed lists with ``DenseHalfIndex``'s score bits; with ``nprobe == nlist`` it is that index's
search.  Training (:func:`train_centroids`) is Lloyd's iteration on the device: assign (``srx_ivf_assign``), a stable sort by
list (torch), update (``srx_ivf_update``)."""
import ctypes

import numpy as np

from . import _capi
from .dense import HALF_TYPES, _DenseIndex, _default_chunk_rows, _f32_rows, _pad64, _require_f32, check_half_dtype, unpack_half_host
from .filter import host_q_filter, resolve_filter
from .index import _check_k, _empty_topk, _grow_ws, _ptr, _stream_ptr, _torch


def check_nlist(nlist, n_docs: int) -> int:
    if not (1 <= int(nlist) <= min(int(n_docs), _capi.SRX_IVF_MAX_LIST)):
        raise ValueError(f"nlist must be in [1, min(n_docs, {_capi.SRX_IVF_MAX_LIST})], got {nlist} for {n_docs} docs")
    return int(nlist)


def check_nprobe(nprobe, nlist: int) -> int:
    if not (1 <= int(nprobe) <= min(int(nlist), _capi.SRX_IVF_MAX_PROBE)):
        raise ValueError(f"nprobe must be in [1, min(nlist, {_capi.SRX_IVF_MAX_PROBE})], got {nprobe} for nlist {nlist}")
    return int(nprobe)


def workspace_bytes(nq: int, nlist: int, nprobe: int, k: int, max_list_tiles: int) -> int:
    """The formula of include/ivf/sparse_rx_ivf.h restated (pinned to ``srx_ivf_workspace_bytes`` by tests/test_ivf_cpu.py)."""
    r = lambda x: -(-x // 256) * 256
    ldc, strip = -(-nlist // 32) * 32, max_list_tiles * 128
    P = min(nq, max(1, min(_capi.SRX_IVF_PASS, (1 << 30) // (nprobe * strip))))
    N, fan = P * nprobe, 4096 // k
    g = -(-nprobe // fan)
    merge = 2 * (P * g * k * 8 + P * g * 4 + 256) if g > 1 else 0
    return (r(min(nq, _capi.SRX_IVF_PASS) * ldc * 4) + 4 * r(N * 4) + 4 * r((nlist + 1) * 4) + r(N * strip) + 2 * r(N * k * 4) + r(N * 4)
            + merge + 256)


def pack_half_device(x, dtype: str):
    """f32[n, dim] device tensor -> (the rows in the fragment order of include/sparse_rx_half.h as a u8 tensor, dim_pad):
    ``srx_dense_convert_half``; how the centroids are stored.  ``ValueError`` for a row that is not finite as ``dtype``."""
    torch, L = _torch(), _capi.lib()
    x, ld = _f32_rows(torch, x, "rows")
    n, dim = int(x.shape[0]), int(x.shape[1])
    dim_pad = _pad64(dim, dtype)
    with torch.cuda.device(x.device):
        out = torch.empty(_capi.check(L.srx_dense_half_bytes(n, dim_pad), "srx_dense_half_bytes"), dtype=torch.uint8, device=x.device)
        flag = torch.zeros(1, dtype=torch.int32, device=x.device)
        _capi.check(L.srx_dense_convert_half(x.device.index or 0, HALF_TYPES[dtype], _ptr(x), ld, n, dim, dim_pad, 0, n, _ptr(out), _ptr(flag),
                                             _stream_ptr(torch, x.device)), "srx_dense_convert_half")
    if int(flag.item()) & _capi.SRX_QUANT_NONFINITE:
        raise ValueError(f"rows hold a value that is not finite as {dtype}")
    return out, dim_pad


def assign_device(centroids_packed, nlist: int, dtype: str, rows, with_score: bool = False):
    """``srx_ivf_assign``: f32[n, dim] device rows against packed centroids -> list i32[n] (and score f32[n]); asynchronous."""
    torch, L = _torch(), _capi.lib()
    x, ld = _f32_rows(torch, rows, "rows")
    n, dim = int(x.shape[0]), int(x.shape[1])
    with torch.cuda.device(x.device):
        out = torch.empty(n, dtype=torch.int32, device=x.device)
        score = torch.empty(n, dtype=torch.float32, device=x.device) if with_score else None
        _capi.check(L.srx_ivf_assign(x.device.index or 0, HALF_TYPES[dtype], _ptr(centroids_packed), nlist, dim, _pad64(dim, dtype), _ptr(x), ld, n,
                                     _ptr(out), _ptr(score), _stream_ptr(torch, x.device)), "srx_ivf_assign")
    return (out, score) if with_score else out


def members_of(lists, nlist: int):
    """The stable sort by list (torch): list i32[n] -> (member_ptr i64[nlist + 1], member i32[n] sorted by (list, row))."""
    torch = _torch()
    _, order = torch.sort(lists, stable=True)
    ptr = torch.zeros(nlist + 1, dtype=torch.int64, device=lists.device)
    ptr[1:] = torch.cumsum(torch.bincount(lists, minlength=nlist), 0)
    return ptr, order.to(torch.int32)


def update_device(rows, member_ptr, member, prev_centroids):
    """``srx_ivf_update``: the mean of every list's f32 rows in the header's summation order -> f32[nlist, dim]; an empty list
    keeps its row of ``prev_centroids``.  Asynchronous."""
    torch, L = _torch(), _capi.lib()
    x, ld = _f32_rows(torch, rows, "rows")
    prev = prev_centroids.contiguous()
    nlist, dim = int(prev.shape[0]), int(prev.shape[1])
    with torch.cuda.device(x.device):
        out = torch.empty_like(prev)
        _capi.check(L.srx_ivf_update(x.device.index or 0, _ptr(x), ld, dim, nlist, _ptr(member_ptr), _ptr(member), _ptr(prev), _ptr(out),
                                     _stream_ptr(torch, x.device)), "srx_ivf_update")
    return out


def train_centroids(rows, nlist: int, dtype: str = "f16", n_iter: int = 10, seed: int = 0):
    """Lloyd's iteration on f32[n, dim] device rows -> f32[nlist, dim] device centroids.  The initial centroids are the rows at
    the first ``nlist`` entries of a CPU ``torch.randperm(n)`` seeded with ``seed``; each iteration converts the centroids
    (``srx_dense_convert_half``), assigns, sorts stably by list and updates.  Deterministic: the same bits every time."""
    torch = _torch()
    dtype = check_half_dtype(dtype)
    n = int(rows.shape[0])
    check_nlist(nlist, n)
    pick = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))[:nlist]
    cent = rows[pick.to(rows.device)].contiguous()
    for _ in range(int(n_iter)):
        packed, _ = pack_half_device(cent, dtype)
        ptr, member = members_of(assign_device(packed, nlist, dtype, rows), nlist)
        cent = update_device(rows, ptr, member, cent)
    return cent


class IvfHalfIndex(_DenseIndex):
    """The half index's rows (f16 / bf16, MFMA-fragment order) permuted so that every k-means list owns whole 32-row tiles, plus
    the packed centroids and the maps between docs and packed rows.  There is no second copy of the rows."""

    _score_entry = "srx_dense_score_docs_half"
    default_nprobe = None  # what search / search_device read when nprobe is not given (RetrievalService sets it)

    def __init__(self, embeddings, nlist: int, dtype="f16", centroids=None, n_iter: int = 10, train_rows=None, seed: int = 0, device="cuda:0",
                 doc_base: int = 0, chunk_rows=None):
        """``embeddings``: f32[n_docs, dim], a device tensor or a host array / memory map (assigned and gathered ``chunk_rows`` rows
        at a time).  ``centroids`` f32[nlist, dim] (host or device) builds with no training; otherwise :func:`train_centroids`
        runs ``n_iter`` iterations on ``train_rows`` rows picked by a seeded permutation (None: all rows)."""
        self.dtype = check_half_dtype(dtype)
        _require_f32(embeddings, "embeddings")
        torch = self._open(device)
        self.n_docs, self.dim = int(embeddings.shape[0]), int(embeddings.shape[1])
        if self.n_docs == 0:
            raise ValueError("Empty corpus provided")
        self.nlist = check_nlist(nlist, self.n_docs)
        self.dim_pad = self._pad64(self.dtype)
        self.doc_base = int(doc_base)
        self._max_norm = None
        if isinstance(embeddings, torch.Tensor) and not embeddings.is_cuda:
            embeddings = embeddings.numpy()  # a host tensor is a host array: read in chunks, never uploaded whole
        on_device = isinstance(embeddings, torch.Tensor)
        rows = _default_chunk_rows(self.dim) if chunk_rows is None else int(chunk_rows)
        if rows < 32 or rows % 32 != 0:
            raise ValueError(f"chunk_rows must be a positive multiple of 32, got {chunk_rows}")
        fetch = (lambda idx: embeddings.to(self.device)[idx]) if on_device else \
            (lambda idx: torch.from_numpy(np.asarray(embeddings[idx.cpu().numpy()], dtype=np.float32)).to(self.device))
        L = _capi.lib()
        with torch.cuda.device(self.device):
            if centroids is None:
                m = self.n_docs if train_rows is None else max(self.nlist, min(int(train_rows), self.n_docs))
                pick = torch.randperm(self.n_docs, generator=torch.Generator().manual_seed(int(seed)))[:m].sort().values
                sample = embeddings.to(self.device) if on_device and m == self.n_docs else fetch(pick.to(self.device))
                cent = train_centroids(sample, self.nlist, self.dtype, n_iter, seed)
            else:
                cent = torch.as_tensor(np.asarray(centroids, dtype=np.float32) if not isinstance(centroids, torch.Tensor) else centroids,
                                       device=self.device).contiguous()
                if tuple(cent.shape) != (self.nlist, self.dim) or cent.dtype != torch.float32:
                    raise ValueError(f"centroids must be float32 [{self.nlist}, {self.dim}], got {cent.dtype} {tuple(cent.shape)}")
            self.centroids_f32 = cent
            self.centroids, _ = pack_half_device(cent, self.dtype)
            # assign every row, then the stable sort: members of a list in ascending doc order
            lists = torch.empty(self.n_docs, dtype=torch.int32, device=self.device)
            step = self.n_docs if on_device else rows
            for lo in range(0, self.n_docs, step):
                chunk = embeddings[lo: lo + step].to(self.device) if on_device else torch.from_numpy(np.array(embeddings[lo: lo + step], dtype=np.float32)).to(self.device)
                lists[lo: lo + step] = assign_device(self.centroids, self.nlist, self.dtype, chunk)
            ptr, member = members_of(lists, self.nlist)
            sizes = ptr[1:] - ptr[:-1]
            tiles = (sizes + 31) // 32
            list_tile = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)
            list_tile[1:] = torch.cumsum(tiles, 0)
            self.n_tiles, self.max_list_tiles = int(list_tile[-1].item()), int(tiles.max().item())
            self.list_tile = list_tile.to(torch.int32)
            self._sizes = sizes
            sorted_lists = lists[member.long()].long()
            row = list_tile[sorted_lists] * 32 + (torch.arange(self.n_docs, device=self.device) - ptr[sorted_lists])  # of member i
            self.doc_row = torch.empty(self.n_docs, dtype=torch.int32, device=self.device)
            self.doc_row[member.long()] = row.to(torch.int32)
            self.row_doc = torch.full((self.n_tiles * 32,), -1, dtype=torch.int32, device=self.device)
            self.row_doc[row] = member
            # gather in chunks of packed rows (-1: a zero row) and convert into the permuted buffer
            n_rows = self.n_tiles * 32
            self.corpus = torch.empty(_capi.check(L.srx_dense_half_bytes(n_rows, self.dim_pad), "srx_dense_half_bytes"), dtype=torch.uint8, device=self.device)
            flag = torch.zeros(1, dtype=torch.int32, device=self.device)
            for lo in range(0, n_rows, rows):
                docs = self.row_doc[lo: lo + rows].long()
                live = docs >= 0
                x = torch.zeros((int(docs.shape[0]), self.dim), dtype=torch.float32, device=self.device)
                x[live] = fetch(docs[live])
                _capi.check(L.srx_dense_convert_half(self.device.index or 0, HALF_TYPES[self.dtype], _ptr(x), self.dim, int(x.shape[0]), self.dim,
                                                     self.dim_pad, lo, n_rows, _ptr(self.corpus), _ptr(flag), _stream_ptr(torch, self.device)),
                            "srx_dense_convert_half")
            if int(flag.item()) & _capi.SRX_QUANT_NONFINITE:
                raise ValueError(f"embeddings hold a value that is not finite as {self.dtype} (NaN / inf, or too large for the type)")
        self._desc = _capi.IvfDesc(device=self.device.index or 0, type=HALF_TYPES[self.dtype], n_docs=self.n_docs, doc_base=self.doc_base,
                                   n_tiles=self.n_tiles, max_list_tiles=self.max_list_tiles, dim_pad=self.dim_pad, nlist=self.nlist,
                                   corpus=_ptr(self.corpus), centroids=_ptr(self.centroids), list_tile=_ptr(self.list_tile), row_doc=_ptr(self.row_doc),
                                   doc_row=_ptr(self.doc_row))

    # ---- what the index holds ----
    def device_bytes(self) -> int:
        """Bytes resident: the permuted rows, the packed centroids and the three maps."""
        return int(self.corpus.numel() + self.centroids.numel() + 4 * (self.list_tile.numel() + self.row_doc.numel() + self.doc_row.numel()))

    def list_sizes(self) -> np.ndarray:
        """i64[nlist]: the docs of every list."""
        return self._sizes.cpu().numpy()

    def centroids_to_host(self) -> np.ndarray:
        """f32[nlist, dim]: the centroids before their rounding to the index type."""
        return self.centroids_f32.cpu().numpy()

    def corpus_to_host(self) -> np.ndarray:
        """u16[n_docs, dim]: the 16-bit codes of the rounded rows in DOC order (as ``DenseHalfIndex.corpus_to_host``)."""
        _torch().cuda.synchronize(self.device)
        packed = unpack_half_host(self.corpus.cpu().numpy(), self.n_tiles * 32, self.dim_pad)
        return np.ascontiguousarray(packed[self.doc_row.cpu().numpy().astype(np.int64)][:, : self.dim])

    def max_row_norm(self) -> float:
        """Largest Euclidean norm of the ROUNDED rows (fp64 accumulation), computed once from a host copy."""
        if self._max_norm is None:
            c = self.corpus_to_host()
            x = (c.view(np.float16) if self.dtype == "f16" else (c.astype(np.uint32) << 16).view(np.float32)).astype(np.float64)
            self._max_norm = float((x * x).sum(axis=1).max()) ** 0.5
        return self._max_norm

    # ---- doors ----
    def _ws_for(self, torch, nq, nprobe, k, tiles):
        need = _capi.check(_capi.lib().srx_ivf_workspace_bytes(nq, self.nlist, nprobe, k, tiles), "srx_ivf_workspace_bytes")
        return _grow_ws(torch, self, need)

    def assign_device(self, rows_f32, with_score: bool = False):
        """f32[n, dim] device rows -> the list of each (``srx_ivf_assign``)."""
        return assign_device(self.centroids, self.nlist, self.dtype, rows_f32, with_score)

    def assign(self, rows: np.ndarray) -> np.ndarray:
        return self.assign_device(self._queries_to_device(rows)).cpu().numpy()

    def probe_device(self, queries_f32, nprobe: int):
        """f32[nq, dim] device queries -> (list i32[nq, nprobe], score f32[nq, nprobe]): the best centroids by (score descending,
        list ascending); asynchronous."""
        torch = _torch()
        nprobe = check_nprobe(nprobe, self.nlist)
        nq = int(queries_f32.shape[0])
        with torch.cuda.device(self.device):
            q = self._padded(torch, queries_f32, torch.float32)
            out = (torch.empty((nq, nprobe), dtype=torch.int32, device=self.device), torch.empty((nq, nprobe), dtype=torch.float32, device=self.device))
            if nq > 0:
                ws = self._ws_for(torch, nq, nprobe, 1, 1)
                _capi.check(_capi.lib().srx_ivf_probe(ctypes.byref(self._desc), _ptr(q), nq, nprobe, _ptr(out[0]), _ptr(out[1]), _ptr(ws), ws.numel(),
                                                      _stream_ptr(torch, self.device)), "srx_ivf_probe")
        return out

    def probe(self, queries: np.ndarray, nprobe: int):
        return self._host(self.probe_device(self._queries_to_device(queries), nprobe))

    def search_device(self, queries_f32, k: int, nprobe=None, score_offset: float = 0.0, filter=None, q_filter=None, probe_list=None):
        """f32[nq, dim] device queries -> (doc i32[nq,k], score f32[nq,k], count i32[nq]) over the allowed docs of the probed lists
        (``srx_ivf_search``); asynchronous.  ``probe_list``: i32[nq, nprobe] device tensor of the lists to read instead of the
        ``nprobe`` best (-1 and repeated entries are skipped); ``filter`` / ``q_filter`` as ``DenseHalfIndex.search_device``."""
        torch = _torch()
        _check_k(k)
        if nprobe is None and self.default_nprobe is None:
            raise ValueError("nprobe must be given: this index has no default_nprobe")
        nprobe = check_nprobe(self.default_nprobe if nprobe is None else nprobe, self.nlist)
        nq = int(queries_f32.shape[0])
        with torch.cuda.device(self.device):
            q = self._padded(torch, queries_f32, torch.float32)
            out = _empty_topk(torch, nq, k, self.device)
            if nq == 0:
                return out
            if probe_list is not None:
                if not isinstance(probe_list, torch.Tensor) or probe_list.dtype != torch.int32 or tuple(probe_list.shape) != (nq, nprobe) or probe_list.device != self.device:
                    raise ValueError(f"probe_list must be an int32 tensor [{nq}, {nprobe}] on {self.device}")
                probe_list = probe_list.contiguous()
            ws = self._ws_for(torch, nq, nprobe, k, self.max_list_tiles)
            fdesc, keep = resolve_filter(self, filter, q_filter, nq)  # keep: alive until the call has been issued
            _capi.check(_capi.lib().srx_ivf_search(ctypes.byref(self._desc), _ptr(q), nq, nprobe, k, _ptr(probe_list), fdesc, _ptr(out[0]), _ptr(out[1]),
                                                   _ptr(out[2]), _ptr(ws), ws.numel(), _stream_ptr(torch, self.device), float(score_offset)),
                        "srx_ivf_search")
        return out

    def search(self, queries: np.ndarray, k: int, nprobe=None, score_offset: float = 0.0, filter=None, q_filter=None, probe_list=None):
        """Host arrays in, host arrays out; ``q_filter``: a host sequence of row numbers, validated here."""
        q = self._queries_to_device(queries)
        if probe_list is not None:
            probe_list = _torch().as_tensor(np.ascontiguousarray(probe_list, dtype=np.int32), device=self.device)
        return self._host(self.search_device(q, k, nprobe, score_offset, filter=filter, q_filter=host_q_filter(self, filter, q_filter, int(q.shape[0])),
                                             probe_list=probe_list))

    def _queries_to_device(self, queries):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        return _torch().as_tensor(q, device=self.device)

    def score_docs_device(self, queries_f32, cand_doc, cand_count=None, out=None):
        """``srx_dense_score_docs_half`` on the permuted rows, the ids translated through ``doc_row``: the contract and the bits of
        ``DenseHalfIndex.score_docs_device``."""
        return self._score_docs_device(queries_f32, _torch().float32, cand_doc, cand_count, out)

    def _launch_score(self, L, q, nq, cand_doc, cand_count, m, out, stream):
        torch = _torch()
        local = cand_doc.long() - self.doc_base
        inside = (local >= 0) & (local < self.n_docs)
        rows = torch.where(inside, self.doc_row[local.clamp(0, self.n_docs - 1)], torch.full_like(cand_doc, -1)).contiguous()
        return L.srx_dense_score_docs_half(self.device.index or 0, HALF_TYPES[self.dtype], _ptr(self.corpus), self.n_tiles * 32, self.dim_pad, _ptr(q),
                                           nq, 0, _ptr(rows), _ptr(cand_count), m, _ptr(out), stream)

    def score_docs(self, queries: np.ndarray, cand_doc, cand_count=None) -> np.ndarray:
        """Host arrays in (the candidates validated by ``validate_candidates``), f32[nq, m] out."""
        q = self._queries_to_device(queries)
        return self._score_docs(cand_doc, cand_count, int(q.shape[0]), lambda cd, cc: self.score_docs_device(q, cd, cc))
