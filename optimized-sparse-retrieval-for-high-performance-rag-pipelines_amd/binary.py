"""Binary dense index (include/binary/sparse_rx_binary.h): one bit per dimension, Hamming top-m on the GPU, and a screened
search that rescores the Hamming pool with the exact rows.

:class:`DenseBinaryIndex` keeps ONLY the 1-bit codes (32 times fewer bytes than f32).  :class:`ScreenedDenseIndex` pairs it
with a :class:`~.dense.DenseF32Index` or :class:`~.dense.DenseHalfIndex` over the same rows: the codes screen the corpus, the
exact index scores the short pool.  The screened index keeps the exact rows resident: it saves bandwidth, not memory.
The reference has no binary index: nothing here mirrors reference code.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from .dense import DenseF32Index, DenseHalfIndex, _f32_rows, _require_f32
from .filter import host_q_filter, resolve_filter
from .index import _check_k, _grow_ws, _ptr, _stream_ptr, _to_host, _torch, merge_topk_device, validate_candidates

# the kernels' geometry (csrc/dense_binary.hip; pinned to the library's workspace formula by tests/test_binary_cpu.py)
TILE_ROWS = _capi.SRX_BINARY_TILE              # rows per tile of the corpus layout: one per lane
QUERY_TILE = _capi.SRX_BINARY_QTILE            # queries a wave walks with its tile's words in registers
PASS_QUERIES = _capi.SRX_BINARY_PASS           # queries per pass at most (one distance matrix in the workspace)
RANK_CHUNK = _capi.SRX_BINARY_RANK_CHUNK       # columns a workgroup of the rank kernel folds per step
SPLIT_DOCS = _capi.SRX_BINARY_SPLIT_DOCS       # a row split of the rank kernel is at least this many docs
BLOCK_DOCS = _capi.SRX_BINARY_BLOCK_DOCS       # docs per workgroup of the distance kernel (four tiles)
MAX_DIM = 1024
MAX_POOL = _capi.SRX_MAX_K                     # the Hamming pool of a screened search: one list of the engine


def pad128(dim: int) -> int:
    """``dim_pad``: the row length rounded up to the 128 columns a 16-byte piece covers.  ``ValueError`` above 1024."""
    dim = int(dim)
    if dim < 1:
        raise ValueError(f"embedding dim must be >= 1, got {dim}")
    if dim > MAX_DIM:
        raise ValueError(f"embedding dim {dim} > {MAX_DIM} is not supported by the binary engine")
    return (dim + 127) // 128 * 128


def binary_bytes(n_rows: int, dim_pad: int, tiled: bool) -> int:
    """``srx_binary_bytes`` restated."""
    rows = -(-int(n_rows) // TILE_ROWS) * TILE_ROWS if tiled else int(n_rows)
    return rows * (int(dim_pad) // 32) * 4


def search_plan(nq: int, n_docs: int, m: int):
    """``(queries per pass, row splits, workspace bytes)`` of ``srx_binary_search``: the formula of the header restated."""
    nq, n_docs, m = int(nq), int(n_docs), int(m)
    ld = -(-n_docs // TILE_ROWS) * TILE_ROWS
    QB = min(max((1 << 32) // (2 * ld) // 32 * 32, 32), PASS_QUERIES)
    qb = min(nq, QB)
    ns = max(1, min(2048 // max(qb, 1), n_docs // SPLIT_DOCS, 4096 // m))
    r256 = lambda x: -(-x // 256) * 256
    return QB, ns, r256(2 * qb * ld) + 2 * r256(4 * qb * ns * m) + r256(4 * qb * ns) + r256(4 * qb * m) + 256


def tiled_word_index(row, word, words: int):
    """Index of word ``word`` of row ``row`` in the tiled corpus (u32 units), for rows of ``words`` words."""
    return (((row >> 6) * (words // 4) + (word >> 2)) * 64 + (row & 63)) * 4 + (word & 3)


def untile_host(tiled: np.ndarray, n_rows: int, words: int) -> np.ndarray:
    """The tiled corpus buffer (any dtype, viewed as u32) -> u32[n_rows, words], row-major."""
    t = np.asarray(tiled).view(np.uint32).reshape(-1, words // 4, 64, 4)  # [tile][piece][row of the tile][word of the piece]
    return np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(-1, words)[: int(n_rows)]


# ---- the arithmetic of a screened search (CPU tensors work: tests/test_binary_cpu.py) ---------------------------------------
def check_oversample(oversample) -> int:
    if isinstance(oversample, bool) or int(oversample) != oversample or int(oversample) < 1:
        raise ValueError(f"oversample must be an integer >= 1, got {oversample!r}")
    return int(oversample)


def screen_pool(k: int, oversample: int, n_docs: int) -> int:
    """Docs the Hamming screen hands to the exact scorer: ``min(max(k, k * oversample), 1024, n_docs)``."""
    return min(max(int(k), int(k) * int(oversample)), MAX_POOL, int(n_docs))


def pool_lists(pool: int, k: int) -> int:
    """The pool viewed as this many lists of k for ``srx_merge_topk`` (the last one may be short)."""
    return -(-int(pool) // int(k))


def sublist_counts(pool_count, n_lists: int, k: int):
    """i32[nq] pool counts -> i32[nq, n_lists]: list j holds entries j k .. j k + k - 1 of the pool, so
    ``count[q, j] = clamp(pool_count[q] - j k, 0, k)``."""
    torch = _torch()
    j = torch.arange(int(n_lists), dtype=torch.int32, device=pool_count.device) * int(k)
    return (pool_count.to(torch.int32)[:, None] - j[None, :]).clamp_(0, int(k)).contiguous()


def pool_as_lists(pool_doc, pool_score, pool_count, k: int):
    """The pool [nq, pool] as (doc i32[nq, L, k], score f32[nq, L, k], count i32[nq, L]): columns past the pool are doc -1 /
    score +0.0 and lie behind every count."""
    torch = _torch()
    nq, pool = int(pool_doc.shape[0]), int(pool_doc.shape[1])
    L = pool_lists(pool, k)
    if L * k != pool:
        pad = L * k - pool
        pool_doc = torch.cat([pool_doc, torch.full((nq, pad), -1, dtype=pool_doc.dtype, device=pool_doc.device)], dim=1)
        pool_score = torch.cat([pool_score, torch.zeros((nq, pad), dtype=pool_score.dtype, device=pool_score.device)], dim=1)
    return pool_doc.reshape(nq, L, k), pool_score.reshape(nq, L, k), sublist_counts(pool_count, L, k)


def _column_means(torch, emb, device, rows: int):
    """f32[dim] column means (fp64 accumulation on the device, chunked for a host array)."""
    n, dim = int(emb.shape[0]), int(emb.shape[1])
    total = torch.zeros(dim, dtype=torch.float64, device=device)
    for lo in range(0, n, rows):
        c = emb[lo: lo + rows]
        c = c.to(device) if isinstance(c, torch.Tensor) else torch.from_numpy(np.array(c, dtype=np.float32)).to(device)
        total += c.double().sum(dim=0)
    return (total / n).float()


class DenseBinaryIndex:
    """1-bit codes of an embedding matrix resident in HBM (include/binary/sparse_rx_binary.h): bit c of a row is
    ``x[c] > center[c]``, kept ONLY in the 64-row tiles the Hamming search reads.  ``hamming_search`` returns, per query, the m
    allowed docs nearest by (Hamming distance ascending, doc ascending); ``hamming_docs`` the distances of given docs."""

    def __init__(self, embeddings, center="mean", device="cuda:0", doc_base: int = 0, chunk_rows=None):
        """``embeddings``: f32[n_docs, dim], a device tensor (one launch) or a host array, possibly a read-only memory map
        (uploaded ``chunk_rows`` rows at a time through one staging tensor, a multiple of 64; default: 64 MB of rows).
        ``center``: "mean" (the column means, computed ONCE here and kept as data), None (zeros) or an array f32[dim]."""
        _require_f32(embeddings, "embeddings")
        torch = _torch()
        if not torch.cuda.is_available():
            raise _capi.SparseRxUnavailable("no HIP device visible: DenseBinaryIndex needs a GPU (there is no CPU fallback)")
        L = _capi.lib()
        self.device = torch.device(device)
        self._ws = None
        self.n_docs, self.dim = int(embeddings.shape[0]), int(embeddings.shape[1])
        if self.n_docs == 0:
            raise ValueError("Empty corpus provided")
        self.dim_pad = pad128(self.dim)
        self.words = self.dim_pad // 32
        self.doc_base = int(doc_base)
        rows = max(TILE_ROWS, ((64 << 20) // (4 * self.dim)) // TILE_ROWS * TILE_ROWS) if chunk_rows is None else int(chunk_rows)
        if rows < TILE_ROWS or rows % TILE_ROWS != 0:
            raise ValueError(f"chunk_rows must be a positive multiple of {TILE_ROWS}, got {chunk_rows}")
        with torch.cuda.device(self.device):
            if center is None:
                self.center = None
            elif isinstance(center, str):
                if center != "mean":
                    raise ValueError(f"center must be 'mean', None or an array of {self.dim} floats, got {center!r}")
                self.center = _column_means(torch, embeddings, self.device, rows)
            else:
                c = center.detach().cpu().numpy() if isinstance(center, torch.Tensor) else np.asarray(center)
                if c.shape != (self.dim,):
                    raise ValueError(f"center must be 'mean', None or an array of {self.dim} floats, got shape {c.shape}")
                self.center = torch.as_tensor(np.ascontiguousarray(c, dtype=np.float32), device=self.device)
            nbytes = _capi.check(L.srx_binary_bytes(self.n_docs, self.dim_pad, 1), "srx_binary_bytes")
            self.bits = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            if isinstance(embeddings, torch.Tensor):
                self._encode(torch, L, embeddings.to(self.device), 0, self.n_docs, 1, self.bits)
            else:
                stage = torch.empty((min(rows, self.n_docs), self.dim), dtype=torch.float32, device=self.device)
                for lo in range(0, self.n_docs, rows):
                    chunk = torch.from_numpy(np.array(embeddings[lo: lo + rows], dtype=np.float32))  # np.array copies the chunk only
                    n = int(chunk.shape[0])
                    stage[:n].copy_(chunk)  # stream-ordered behind the previous chunk's kernel
                    self._encode(torch, L, stage[:n], lo, self.n_docs, 1, self.bits)

    def _encode(self, torch, L, x, row0: int, n_total: int, tiled: int, out) -> None:
        x, ld = _f32_rows(torch, x, "embeddings")
        _capi.check(L.srx_binary_encode(self.device.index or 0, _ptr(x), ld, int(x.shape[0]), self.dim, self.dim_pad, row0, n_total,
                                        _ptr(self.center), tiled, _ptr(out), _stream_ptr(torch, self.device)), "srx_binary_encode")

    @classmethod
    def from_embeddings(cls, emb, center="mean", device="cuda:0", doc_base: int = 0, chunk_rows=None):
        """The constructor under the name the other dense indexes give theirs."""
        return cls(emb, center=center, device=device, doc_base=doc_base, chunk_rows=chunk_rows)

    def device_bytes(self) -> int:
        """Bytes of the resident codes (``srx_binary_bytes``)."""
        return int(self.bits.numel())

    def center_host(self) -> np.ndarray:
        """f32[dim]: the centre the codes were taken against (zeros for ``center=None``)."""
        return np.zeros(self.dim, np.float32) if self.center is None else self.center.cpu().numpy()

    def bits_to_host(self) -> np.ndarray:
        """u32[n_docs, W]: the codes, untiled."""
        _torch().cuda.synchronize(self.device)
        return untile_host(self.bits.cpu().numpy(), self.n_docs, self.words)

    # -- queries ----------------------------------------------------------------------------------------------------
    def encode_queries_device(self, queries_f32):
        """f32[nq, dim] on the device -> i32[nq, W] (the u32 words), encoded against the index's centre; asynchronous."""
        torch = _torch()
        _require_f32(queries_f32, "queries")
        if int(queries_f32.shape[1]) != self.dim:
            raise ValueError(f"queries have {int(queries_f32.shape[1])} columns, the index {self.dim}")
        nq = int(queries_f32.shape[0])
        with torch.cuda.device(self.device):
            out = torch.empty((nq, self.words), dtype=torch.int32, device=self.device)
            if nq > 0:
                self._encode(torch, _capi.lib(), queries_f32.to(self.device), 0, nq, 0, out)
        return out

    def _query_bits(self, torch, queries_f32, q_bits):
        if (queries_f32 is None) == (q_bits is None):
            raise ValueError("give the queries either as f32 rows or as q_bits=, not both")
        if q_bits is None:
            return self.encode_queries_device(queries_f32)
        if not isinstance(q_bits, torch.Tensor) or q_bits.dtype != torch.int32 or q_bits.dim() != 2 or int(q_bits.shape[1]) != self.words \
                or q_bits.device != self.device:
            raise ValueError(f"q_bits must be an int32 tensor [nq, {self.words}] on {self.device}")
        return q_bits.contiguous()

    def _queries_to_device(self, queries):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        return _torch().as_tensor(q, device=self.device)

    # -- search -----------------------------------------------------------------------------------------------------
    def hamming_search_device(self, queries_f32, m: int, q_bits=None, filter=None, q_filter=None):
        """``srx_binary_search``: (doc i32[nq, m], dist i32[nq, m], count i32[nq]), asynchronous.  Row q holds the
        ``count[q] = min(m, allowed docs)`` nearest allowed docs by (distance ascending, doc ascending), then -1 / -1.
        ``filter`` / ``q_filter`` as ``DeviceIndex.search_device``."""
        torch = _torch()
        _check_k(m)
        L = _capi.lib()
        with torch.cuda.device(self.device):
            qb = self._query_bits(torch, queries_f32, q_bits)
            nq = int(qb.shape[0])
            out = (torch.empty((nq, m), dtype=torch.int32, device=self.device), torch.empty((nq, m), dtype=torch.int32, device=self.device),
                   torch.empty((nq,), dtype=torch.int32, device=self.device))
            if nq == 0:
                return out
            ws = _grow_ws(torch, self, _capi.check(L.srx_binary_workspace_bytes(nq, self.n_docs, m), "srx_binary_workspace_bytes"))
            fdesc, keep = resolve_filter(self, filter, q_filter, nq)  # keep: alive until the call has been issued
            _capi.check(L.srx_binary_search(self.device.index or 0, _ptr(self.bits), self.n_docs, self.dim_pad, _ptr(qb), nq, m, self.doc_base,
                                            fdesc, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(ws), ws.numel(), _stream_ptr(torch, self.device)),
                        "srx_binary_search")
            del keep
        return out

    def hamming_search(self, queries, m: int, filter=None, q_filter=None):
        """Host arrays in, host arrays out; ``q_filter``: a host sequence of row numbers, validated here."""
        q = self._queries_to_device(queries)
        qf = host_q_filter(self, filter, q_filter, int(q.shape[0]))
        return _to_host(_torch(), self.device, self.hamming_search_device(q, m, filter=filter, q_filter=qf))

    def hamming_docs_device(self, queries_f32, cand_doc, cand_count=None, q_bits=None):
        """``srx_binary_dist_docs``: i32[nq, m], the distances of the given GLOBAL ids; -1 for padding (-1, entries at or beyond
        ``cand_count[q]``) and ids outside the index; duplicates are legal.  Asynchronous."""
        torch = _torch()
        L = _capi.lib()
        with torch.cuda.device(self.device):
            qb = self._query_bits(torch, queries_f32, q_bits)
            nq = int(qb.shape[0])
            if cand_doc.dim() != 2 or int(cand_doc.shape[0]) != nq or cand_doc.dtype != torch.int32 or int(cand_doc.shape[1]) < 1:
                raise ValueError("hamming_docs_device: cand_doc must be an int32 tensor [nq, m] with m >= 1")
            if cand_count is not None and (cand_count.dtype != torch.int32 or cand_count.numel() != nq):
                raise ValueError("hamming_docs_device: cand_count must be an int32 tensor [nq]")
            m = int(cand_doc.shape[1])
            cand_doc = cand_doc.contiguous()
            cand_count = None if cand_count is None else cand_count.contiguous()
            out = torch.empty((nq, m), dtype=torch.int32, device=self.device)
            if nq > 0:
                _capi.check(L.srx_binary_dist_docs(self.device.index or 0, _ptr(self.bits), self.n_docs, self.dim_pad, _ptr(qb), nq, self.doc_base,
                                                   _ptr(cand_doc), _ptr(cand_count), m, _ptr(out), _stream_ptr(torch, self.device)),
                            "srx_binary_dist_docs")
        return out

    def hamming_docs(self, queries, cand_doc, cand_count=None) -> np.ndarray:
        """Host arrays in (the candidates validated by :func:`validate_candidates`), i32[nq, m] out."""
        torch = _torch()
        q = self._queries_to_device(queries)
        cand_doc, cand_count = validate_candidates(cand_doc, cand_count, int(q.shape[0]))
        cd = torch.as_tensor(cand_doc, device=self.device)
        cc = None if cand_count is None else torch.as_tensor(cand_count, device=self.device)
        return _to_host(torch, self.device, (self.hamming_docs_device(q, cd, cc),))[0]


class ScreenedDenseIndex:
    """A dense index searched in two steps: the Hamming screen of ``binary`` picks
    ``pool = min(max(k, k * oversample), 1024, n_docs)`` docs under the caller's filter, ``exact.score_docs_device`` scores them
    (the exact search's own score bits), and ``srx_merge_topk`` cuts the pool to k by (value descending, doc ascending), values
    > 0 only.  ``search`` has the signature and the (doc, score, count) contract of the exact index; with
    ``k * oversample >= n_docs`` it returns what ``exact.search`` returns, bit for bit.  The exact rows stay resident: the
    screen saves bandwidth, not memory."""

    def __init__(self, exact, binary, oversample: int = 4):
        if not isinstance(exact, (DenseF32Index, DenseHalfIndex)):
            raise ValueError(f"the exact index of a screened search must be a DenseF32Index or a DenseHalfIndex, got {type(exact).__name__}")
        if not isinstance(binary, DenseBinaryIndex):
            raise ValueError(f"the screen must be a DenseBinaryIndex, got {type(binary).__name__}")
        if (exact.n_docs, exact.dim, exact.doc_base) != (binary.n_docs, binary.dim, binary.doc_base) or exact.device != binary.device:
            raise ValueError(f"the screen speaks of {binary.n_docs} x {binary.dim} rows from id {binary.doc_base} on {binary.device}, the exact "
                             f"index of {exact.n_docs} x {exact.dim} from {exact.doc_base} on {exact.device}")
        self.exact, self.binary, self.oversample = exact, binary, check_oversample(oversample)
        self.n_docs, self.dim, self.doc_base, self.device = exact.n_docs, exact.dim, exact.doc_base, exact.device

    def pool(self, k: int) -> int:
        return screen_pool(k, self.oversample, self.n_docs)

    def search_device(self, queries, k: int, score_offset: float = 0.0, filter=None, q_filter=None):
        """f32[nq, dim] queries on the device -> (doc i32[nq,k], score f32[nq,k], count i32[nq]); asynchronous.  Top-k of
        fl32(score + score_offset) > 0 among the Hamming pool; the returned scores carry the offset."""
        torch = _torch()
        _check_k(k)
        queries = queries.to(self.device)
        if int(queries.shape[0]) == 0:
            return self.exact.search_device(queries, k, score_offset, filter=filter, q_filter=q_filter)
        pool_doc, _, pool_count = self.binary.hamming_search_device(queries, self.pool(k), filter=filter, q_filter=q_filter)
        score = self.exact.score_docs_device(queries, pool_doc, pool_count)
        if score_offset != 0.0:
            score = score + torch.tensor(float(score_offset), dtype=torch.float32, device=self.device)  # fl32(score + offset)
        return merge_topk_device(*pool_as_lists(pool_doc, score, pool_count, k), k)

    def search(self, queries, k: int, score_offset: float = 0.0, filter=None, q_filter=None):
        """Host arrays in, host arrays out; ``q_filter``: a host sequence of row numbers, validated here."""
        q = self.exact._queries_to_device(queries)
        qf = host_q_filter(self, filter, q_filter, int(q.shape[0]))
        return _to_host(_torch(), self.device, self.search_device(q, k, score_offset, filter=filter, q_filter=qf))

    # -- what does not involve the screen: the exact index's own ---------------------------------------------------------
    def score_docs_device(self, *args, **kw):
        return self.exact.score_docs_device(*args, **kw)

    def score_docs(self, *args, **kw):
        return self.exact.score_docs(*args, **kw)

    def mmr_device(self, *args, **kw):
        return self.exact.mmr_device(*args, **kw)

    def mmr(self, *args, **kw):
        return self.exact.mmr(*args, **kw)

    def max_row_norm(self) -> float:
        return self.exact.max_row_norm()

    def corpus_to_host(self):
        return self.exact.corpus_to_host()

    def device_bytes(self) -> int:
        """Bytes resident for the pair: the exact rows AND the codes."""
        exact = self.exact.device_bytes() if hasattr(self.exact, "device_bytes") else int(self.exact.emb.numel()) * 4
        return exact + self.binary.device_bytes()
