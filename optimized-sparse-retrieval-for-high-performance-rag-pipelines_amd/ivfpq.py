"""IVF-PQ dense index (include/ivfpq/sparse_rx_ivfpq.h): the k-means lists of the IVF index holding 8-bit product codes of the
RESIDUAL ``x - rounded centroid`` instead of rows.  No reference counterpart.  :class:`IvfPqIndex` keeps only the codes, the
packed centroids, the residual codebooks and the maps between docs and packed rows; a query reads the codes of ``nprobe`` lists
and scores a doc ``fl(coarse + sum of table entries)``.  The arithmetic has no tolerance: the header states every fp32 operation.
Training is ``ivf.train_centroids`` for the lists and ``pq.train_codebooks`` on the residuals of the training sample."""
import ctypes

import numpy as np

from . import _capi, ivf, pq
from .dense import HALF_TYPES, _DenseIndex, _f32_rows, _pad64, _require_f32, check_half_dtype
from .filter import host_q_filter, resolve_filter
from .index import _check_k, _empty_topk, _grow_ws, _ptr, _stream_ptr, _torch

TILE_ROWS = _capi.SRX_PQ_TILE


def search_plan(nq: int, nlist: int, nprobe: int, k: int, M: int, max_list_tiles: int):
    """``(queries per pass P, slices per query S, tiles per slice L, workspace bytes)`` of ``srx_ivfpq_search``: the formulas of
    the header restated (the bytes are pinned to ``srx_ivfpq_workspace_bytes`` by tests/test_ivfpq_cpu.py)."""
    nq, nlist, nprobe, k, M, T = int(nq), int(nlist), int(nprobe), int(k), int(M), int(nprobe) * int(max_list_tiles)
    r = lambda x: -(-x // 256) * 256
    P = min(nq, max(1, min(_capi.SRX_IVFPQ_PASS, (1 << 30) // (256 * T))))
    S = max(1, min(_capi.SRX_IVFPQ_TARGET_ITEMS // max(P, 1), _capi.SRX_IVFPQ_MAX_SLICES, (T + _capi.SRX_IVFPQ_SLICE_TILES - 1) // _capi.SRX_IVFPQ_SLICE_TILES))
    L = -(-T // S)
    g = -(-S // (4096 // k))
    merge = 2 * (P * g * k * 8 + P * g * 4 + 256) if g > 1 else 0
    ldc, N = -(-nlist // 32) * 32, P * nprobe
    total = (r(4 * P * ldc) + r(1024 * P * M) + 4 * r(4 * N) + r(4 * P * (nprobe + 1)) + r(256 * P * S * L) + r(4 * P * S * L)
             + 2 * r(4 * P * S * k) + r(4 * P * S) + merge + 256)
    return P, S, L, total


def rounded_centroids(centroids_f32, dtype: str):
    """The f32 values of the centroids after their rounding to the index type (round to nearest even): what the packed centroids
    hold and what the residuals are taken against."""
    torch = _torch()
    return centroids_f32.to(torch.float16 if dtype == "f16" else torch.bfloat16).to(torch.float32)


class IvfPqIndex(_DenseIndex):
    """Product codes of the residuals in 64-row tiles permuted so that every k-means list owns whole tiles, plus the packed
    centroids, the residual codebooks f32[M, 256, dsub] and the maps between docs and packed rows.  No row is kept."""

    _score_entry = "srx_ivfpq_score_docs"
    default_nprobe = None  # what search / search_device read when nprobe is not given (RetrievalService sets it)

    def __init__(self, embeddings, nlist: int, dsub: int = 8, dtype="f16", centroids=None, codebooks=None, lists=None, n_iter: int = 8,
                 train_rows=65536, seed: int = 0, device="cuda:0", doc_base: int = 0, chunk_rows=None):
        """``embeddings``: f32[n_docs, dim], a device tensor or a host array / memory map (assigned and gathered ``chunk_rows``
        rows at a time, a multiple of 64).  ``centroids`` f32[nlist, dim] and ``codebooks`` f32[M, 256, dsub] (host or device)
        build with no training of that part; otherwise ``ivf.train_centroids`` and, on the residuals of the same sample,
        ``pq.train_codebooks`` run ``n_iter`` iterations on ``train_rows`` rows picked by a seeded permutation (None: all rows).
        ``lists``: i32[n_docs], the list of every row, from a caller that clusters elsewhere (default: ``srx_ivf_assign``)."""
        self.dtype = check_half_dtype(dtype)
        _require_f32(embeddings, "embeddings")
        torch = self._open(device)
        self.n_docs, self.dim = int(embeddings.shape[0]), int(embeddings.shape[1])
        if self.n_docs == 0:
            raise ValueError("Empty corpus provided")
        self.nlist = ivf.check_nlist(nlist, self.n_docs)
        self.dsub = int(dsub)
        self.M = pq.subspaces(self.dim, self.dsub)
        self.dim_pad = _pad64(self.dim, "IVF-PQ")
        self.doc_base = int(doc_base)
        self._max_norm = None
        if isinstance(embeddings, torch.Tensor) and not embeddings.is_cuda:
            embeddings = embeddings.numpy()  # a host tensor is a host array: read in chunks, never uploaded whole
        on_device = isinstance(embeddings, torch.Tensor)
        rows = max(TILE_ROWS, ((64 << 20) // (4 * self.dim)) // TILE_ROWS * TILE_ROWS) if chunk_rows is None else int(chunk_rows)
        if rows < TILE_ROWS or rows % TILE_ROWS != 0:
            raise ValueError(f"chunk_rows must be a positive multiple of {TILE_ROWS}, got {chunk_rows}")
        fetch = (lambda idx: embeddings.to(self.device)[idx]) if on_device else \
            (lambda idx: torch.from_numpy(np.asarray(embeddings[idx.cpu().numpy()], dtype=np.float32)).to(self.device))
        L = _capi.lib()
        with torch.cuda.device(self.device):
            sample = None
            if centroids is None or codebooks is None:
                m = self.n_docs if train_rows is None else max(self.nlist, min(int(train_rows), self.n_docs))
                pick = torch.randperm(self.n_docs, generator=torch.Generator().manual_seed(int(seed)))[:m].sort().values
                sample = embeddings.to(self.device) if on_device and m == self.n_docs else fetch(pick.to(self.device))
            if centroids is None:
                cent = ivf.train_centroids(sample, self.nlist, self.dtype, n_iter, seed)
            else:
                cent = torch.as_tensor(np.asarray(centroids, dtype=np.float32) if not isinstance(centroids, torch.Tensor) else centroids,
                                       device=self.device).contiguous()
                if tuple(cent.shape) != (self.nlist, self.dim) or cent.dtype != torch.float32:
                    raise ValueError(f"centroids must be float32 [{self.nlist}, {self.dim}], got {cent.dtype} {tuple(cent.shape)}")
            self.centroids_f32 = cent
            self.centroids, _ = ivf.pack_half_device(cent, self.dtype)
            self.centroids_rounded = rounded_centroids(cent, self.dtype)
            if codebooks is None:  # the residuals of the sample against the centroids it is assigned to: one f32 subtraction each
                own = ivf.assign_device(self.centroids, self.nlist, self.dtype, sample).long()
                self.codebooks = pq.train_codebooks(sample - self.centroids_rounded[own], self.dsub, n_iter, seed)
            else:
                self.codebooks = pq._check_codebooks(torch, codebooks, self.M, self.dsub, self.device)
            del sample
            # the list of every row, then the stable sort: members of a list in ascending doc order
            if lists is None:
                lists = torch.empty(self.n_docs, dtype=torch.int32, device=self.device)
                step = self.n_docs if on_device else rows
                for lo in range(0, self.n_docs, step):
                    chunk = embeddings[lo: lo + step].to(self.device) if on_device else \
                        torch.from_numpy(np.array(embeddings[lo: lo + step], dtype=np.float32)).to(self.device)
                    lists[lo: lo + step] = ivf.assign_device(self.centroids, self.nlist, self.dtype, chunk)
            else:
                given = np.asarray(lists.cpu() if isinstance(lists, torch.Tensor) else lists)
                if given.shape != (self.n_docs,) or not np.issubdtype(given.dtype, np.integer) or given.min() < 0 or given.max() >= self.nlist:
                    raise ValueError(f"lists must be {self.n_docs} integers in [0, {self.nlist})")
                lists = torch.as_tensor(given.astype(np.int32), device=self.device)
            self.lists = lists
            ptr, member = ivf.members_of(lists, self.nlist)
            sizes = ptr[1:] - ptr[:-1]
            tiles = (sizes + TILE_ROWS - 1) // TILE_ROWS
            list_tile = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)
            list_tile[1:] = torch.cumsum(tiles, 0)
            self.n_tiles, self.max_list_tiles = int(list_tile[-1].item()), int(tiles.max().item())
            self.list_tile = list_tile.to(torch.int32)
            self.tile_list = torch.repeat_interleave(torch.arange(self.nlist, dtype=torch.int32, device=self.device), tiles)
            self._sizes = sizes
            sorted_lists = lists[member.long()].long()
            row = list_tile[sorted_lists] * TILE_ROWS + (torch.arange(self.n_docs, device=self.device) - ptr[sorted_lists])  # of member i
            self.doc_row = torch.empty(self.n_docs, dtype=torch.int32, device=self.device)
            self.doc_row[member.long()] = row.to(torch.int32)
            n_rows = self.n_tiles * TILE_ROWS
            self.row_doc = torch.full((n_rows,), -1, dtype=torch.int32, device=self.device)
            self.row_doc[row] = member
            # encode chunks of gathered packed rows (-1: padding, zero codes) into the permuted buffer
            self.codes = torch.empty(_capi.check(L.srx_pq_bytes(n_rows, self.M), "srx_pq_bytes"), dtype=torch.uint8, device=self.device)
            for lo in range(0, n_rows, rows):
                docs = self.row_doc[lo: lo + rows].long()
                live = docs >= 0
                x, ld = _f32_rows(torch, fetch(docs[live]), "embeddings")
                src = torch.where(live, torch.cumsum(live, 0) - 1, torch.full_like(docs, -1)).to(torch.int32)
                row_list = torch.repeat_interleave(self.tile_list[lo // TILE_ROWS: (lo + int(docs.shape[0])) // TILE_ROWS], TILE_ROWS)
                _capi.check(L.srx_ivfpq_encode(self.device.index or 0, HALF_TYPES[self.dtype], _ptr(self.centroids), self.nlist, self.dim_pad, _ptr(x), ld,
                                               int(x.shape[0]), self.dim, self.dsub, _ptr(self.codebooks), _ptr(src), _ptr(row_list), int(docs.shape[0]),
                                               lo, n_rows, _ptr(self.codes), _stream_ptr(torch, self.device)), "srx_ivfpq_encode")
        self._desc = _capi.IvfPqDesc(device=self.device.index or 0, type=HALF_TYPES[self.dtype], n_docs=self.n_docs, doc_base=self.doc_base,
                                     n_tiles=self.n_tiles, max_list_tiles=self.max_list_tiles, dim=self.dim, dsub=self.dsub, dim_pad=self.dim_pad,
                                     nlist=self.nlist, codes=_ptr(self.codes), codebooks=_ptr(self.codebooks), centroids=_ptr(self.centroids),
                                     list_tile=_ptr(self.list_tile), row_doc=_ptr(self.row_doc), doc_row=_ptr(self.doc_row),
                                     tile_list=_ptr(self.tile_list))

    # ---- what the index holds ----
    def device_bytes(self) -> int:
        """Bytes resident: the codes, the codebooks, the packed centroids and the four maps."""
        return int(self.codes.numel() + 4 * self.codebooks.numel() + self.centroids.numel()
                   + 4 * (self.list_tile.numel() + self.row_doc.numel() + self.doc_row.numel() + self.tile_list.numel()))

    def list_sizes(self) -> np.ndarray:
        """i64[nlist]: the docs of every list."""
        return self._sizes.cpu().numpy()

    def list_of_docs(self) -> np.ndarray:
        """i32[n_docs]: the list of every doc."""
        return self.lists.cpu().numpy()

    def codes_to_host(self) -> np.ndarray:
        """u8[n_docs, M]: the residual codes in DOC order."""
        _torch().cuda.synchronize(self.device)
        packed = pq.untile_host(self.codes.cpu().numpy(), self.n_tiles * TILE_ROWS, self.M)
        return np.ascontiguousarray(packed[self.doc_row.cpu().numpy().astype(np.int64)])

    def codebooks_to_host(self) -> np.ndarray:
        return self.codebooks.cpu().numpy()

    def centroids_to_host(self) -> np.ndarray:
        """f32[nlist, dim]: the centroids before their rounding to the index type."""
        return self.centroids_f32.cpu().numpy()

    def _reconstruct_device(self, torch, d):
        np_ = -(-self.M // 16)
        r = self.doc_row[d].long()
        piece = torch.arange(np_, device=self.device)[None, :]
        at = (((r >> 6)[:, None] * np_ + piece) * 64 + (r & 63)[:, None]) * 16  # [n, pieces]: the byte of each piece
        codes = self.codes[(at[:, :, None] + torch.arange(16, device=self.device)).reshape(len(d), -1)[:, : self.M].long()].long()
        res = self.codebooks[torch.arange(self.M, device=self.device)[None, :], codes].reshape(len(d), -1)[:, : self.dim]
        return self.centroids_rounded[self.lists[d].long()] + res

    def reconstruct(self, docs) -> np.ndarray:
        """f32[len(docs), dim]: rounded centroid + codewords (one f32 addition) for LOCAL doc numbers (a torch gather)."""
        torch = _torch()
        d = torch.as_tensor(np.asarray(docs, dtype=np.int64), device=self.device)
        if d.numel() and (int(d.min()) < 0 or int(d.max()) >= self.n_docs):
            raise ValueError(f"reconstruct: docs must be in [0, {self.n_docs})")
        return self._reconstruct_device(torch, d).cpu().numpy()

    def max_row_norm(self) -> float:
        """Largest Euclidean norm of a RECONSTRUCTED row (fp64), computed once in chunks."""
        if self._max_norm is None:
            torch = _torch()
            best = 0.0
            for lo in range(0, self.n_docs, 65536):
                x = self._reconstruct_device(torch, torch.arange(lo, min(lo + 65536, self.n_docs), device=self.device)).double()
                best = max(best, float((x * x).sum(dim=1).max().item()))
            self._max_norm = best ** 0.5
        return self._max_norm

    # ---- doors ----
    def assign_device(self, rows_f32, with_score: bool = False):
        """f32[n, dim] device rows -> the list of each (``srx_ivf_assign``)."""
        return ivf.assign_device(self.centroids, self.nlist, self.dtype, rows_f32, with_score)

    def probe_device(self, queries_f32, nprobe: int):
        """f32[nq, dim] device queries -> (list i32[nq, nprobe], score f32[nq, nprobe]): ``srx_ivf_probe`` over this index's
        centroids; asynchronous."""
        torch = _torch()
        nprobe = ivf.check_nprobe(nprobe, self.nlist)
        nq = int(queries_f32.shape[0])
        with torch.cuda.device(self.device):
            q = self._padded(torch, queries_f32, torch.float32)
            out = (torch.empty((nq, nprobe), dtype=torch.int32, device=self.device), torch.empty((nq, nprobe), dtype=torch.float32, device=self.device))
            if nq > 0:
                ws = _grow_ws(torch, self, _capi.check(_capi.lib().srx_ivf_workspace_bytes(nq, self.nlist, nprobe, 1, 1), "srx_ivf_workspace_bytes"))
                desc = _capi.IvfDesc(device=self.device.index or 0, type=HALF_TYPES[self.dtype], n_docs=self.n_docs, doc_base=self.doc_base, n_tiles=1,
                                     max_list_tiles=1, dim_pad=self.dim_pad, nlist=self.nlist, corpus=_ptr(self.centroids), centroids=_ptr(self.centroids),
                                     list_tile=_ptr(self.list_tile), row_doc=_ptr(self.row_doc), doc_row=_ptr(self.doc_row))  # the probe reads the centroids only
                _capi.check(_capi.lib().srx_ivf_probe(ctypes.byref(desc), _ptr(q), nq, nprobe, _ptr(out[0]), _ptr(out[1]), _ptr(ws), ws.numel(),
                                                      _stream_ptr(torch, self.device)), "srx_ivf_probe")
        return out

    def probe(self, queries: np.ndarray, nprobe: int):
        return self._host(self.probe_device(self._queries_to_device(queries), nprobe))

    def search_plan(self, nq: int, k: int, nprobe=None):
        """:func:`search_plan` for this index."""
        return search_plan(nq, self.nlist, self.default_nprobe if nprobe is None else nprobe, k, self.M, self.max_list_tiles)

    def search_device(self, queries_f32, k: int, nprobe=None, score_offset: float = 0.0, filter=None, q_filter=None, probe_list=None):
        """f32[nq, dim] device queries -> (doc i32[nq,k], score f32[nq,k], count i32[nq]) over the allowed docs of the probed lists
        (``srx_ivfpq_search``); asynchronous.  ``probe_list``, ``filter`` / ``q_filter`` as ``IvfHalfIndex.search_device``."""
        torch = _torch()
        _check_k(k)
        if nprobe is None and self.default_nprobe is None:
            raise ValueError("nprobe must be given: this index has no default_nprobe")
        nprobe = ivf.check_nprobe(self.default_nprobe if nprobe is None else nprobe, self.nlist)
        nq = int(queries_f32.shape[0])
        L = _capi.lib()
        with torch.cuda.device(self.device):
            q = self._padded(torch, queries_f32, torch.float32)
            out = _empty_topk(torch, nq, k, self.device)
            if nq == 0:
                return out
            if probe_list is not None:
                if not isinstance(probe_list, torch.Tensor) or probe_list.dtype != torch.int32 or tuple(probe_list.shape) != (nq, nprobe) or probe_list.device != self.device:
                    raise ValueError(f"probe_list must be an int32 tensor [{nq}, {nprobe}] on {self.device}")
                probe_list = probe_list.contiguous()
            ws = _grow_ws(torch, self, _capi.check(L.srx_ivfpq_workspace_bytes(nq, self.nlist, nprobe, k, self.M, self.max_list_tiles),
                                                   "srx_ivfpq_workspace_bytes"))
            fdesc, keep = resolve_filter(self, filter, q_filter, nq)  # keep: alive until the call has been issued
            _capi.check(L.srx_ivfpq_search(ctypes.byref(self._desc), _ptr(q), nq, nprobe, k, _ptr(probe_list), fdesc, _ptr(out[0]), _ptr(out[1]),
                                           _ptr(out[2]), _ptr(ws), ws.numel(), _stream_ptr(torch, self.device), float(score_offset)), "srx_ivfpq_search")
            del keep
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
        """``srx_ivfpq_score_docs``: as ``DensePqIndex.score_docs_device``; the bits are those of :meth:`search_device` with
        ``score_offset = 0``."""
        return self._score_docs_device(queries_f32, _torch().float32, cand_doc, cand_count, out)

    def _launch_score(self, L, q, nq, cand_doc, cand_count, m, out, stream):
        ws = _grow_ws(_torch(), self, _capi.check(L.srx_ivfpq_score_docs_workspace_bytes(nq, m), "srx_ivfpq_score_docs_workspace_bytes"))
        return L.srx_ivfpq_score_docs(ctypes.byref(self._desc), _ptr(q), nq, _ptr(cand_doc), _ptr(cand_count), m, _ptr(out), _ptr(ws), ws.numel(), stream)

    def score_docs(self, queries: np.ndarray, cand_doc, cand_count=None) -> np.ndarray:
        """Host arrays in (the candidates validated by ``validate_candidates``), f32[nq, m] out."""
        q = self._queries_to_device(queries)
        return self._score_docs(cand_doc, cand_count, int(q.shape[0]), lambda cd, cc: self.score_docs_device(q, cd, cc))
