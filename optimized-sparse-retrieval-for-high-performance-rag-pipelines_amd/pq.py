"""PQ dense index (include/pq/sparse_rx_pq.h): every ``dsub`` consecutive dimensions of a row become one byte, the index of the
nearest of 256 codewords of that subspace; a query scores a row by adding ``M = ceil(dim / dsub)`` entries of a table it computes
once.  No reference counterpart.  :class:`DensePqIndex` keeps ONLY the codes and the codebooks (96 bytes per 768-dim row at
``dsub = 8``) and has the doors of ``DenseHalfIndex`` (filters, ``score_offset``, the scorer of given docs) without the MMR
selection.  The arithmetic has no tolerance: the header states the order of every fp32 operation.  Training
(:func:`train_codebooks`) is Lloyd's iteration on the device: assign (``srx_pq_encode``), then per subspace a stable sort by
code (torch) and the centroid update of the IVF index (``srx_ivf_update``)."""
import numpy as np

from . import _capi, ivf
from .dense import _DenseIndex, _f32_rows, _require_f32
from .filter import host_q_filter, resolve_filter
from .index import _check_k, _empty_topk, _grow_ws, _ptr, _stream_ptr, _torch

TILE_ROWS = _capi.SRX_PQ_TILE       # rows per tile of the corpus layout: one per lane
CODEWORDS = _capi.SRX_PQ_CODEWORDS  # per subspace, always
MAX_M, MAX_DIM = _capi.SRX_PQ_MAX_M, _capi.SRX_PQ_MAX_DIM
OFFSET_MARGIN = 1.01                # over |q|_2 * max_row_norm: what makes every doc rankable (the bound is fp64, the sums fp32)


def subspaces(dim: int, dsub: int) -> int:
    """``M = ceil(dim / dsub)`` after the header's geometry checks."""
    dim, dsub = int(dim), int(dsub)
    if dsub not in (4, 8, 16):
        raise ValueError(f"dsub must be 4, 8 or 16, got {dsub}")
    if not (1 <= dim <= MAX_DIM):
        raise ValueError(f"embedding dim {dim} outside [1, {MAX_DIM}] is not supported by the PQ engine")
    M = -(-dim // dsub)
    if M > MAX_M:
        raise ValueError(f"dim {dim} at dsub {dsub} gives {M} subspaces, more than {MAX_M}: use a larger dsub")
    return M


def pq_bytes(n_rows: int, M: int) -> int:
    """``srx_pq_bytes`` restated."""
    return -(-int(n_rows) // TILE_ROWS) * TILE_ROWS * (-(-int(M) // 16) * 16)


def search_plan(nq: int, n_docs: int, M: int, k: int):
    """``(queries per pass, row splits, workspace bytes)`` of ``srx_pq_search``: the formula of the header restated."""
    nq, n_docs, M, k = int(nq), int(n_docs), int(M), int(k)
    ld = -(-n_docs // 64) * 64
    QB = min(max((1 << 32) // (4 * ld) // 32 * 32, 32), 1024)
    qb = min(nq, QB)
    ns = max(1, min(2048 // max(qb, 1), n_docs // 16384, 4096 // k))
    r256 = lambda x: -(-x // 256) * 256
    return QB, ns, r256(1024 * qb * M) + r256(4 * qb * ld) + 2 * r256(4 * qb * ns * k) + r256(4 * qb * ns) + 256


def untile_host(tiled: np.ndarray, n_rows: int, M: int) -> np.ndarray:
    """The tiled corpus buffer -> u8[n_rows, M], row-major."""
    t = np.asarray(tiled).view(np.uint8).reshape(-1, -(-M // 16), 64, 16)  # [tile][piece][row of the tile][byte of the piece]
    return np.ascontiguousarray(t.transpose(0, 2, 1, 3).reshape(t.shape[0] * 64, -1)[: int(n_rows), :M])


def _check_codebooks(torch, codebooks, M: int, dsub: int, device):
    cb = torch.as_tensor(codebooks if isinstance(codebooks, torch.Tensor) else np.asarray(codebooks), device=device)
    if cb.dtype != torch.float32 or tuple(cb.shape) != (M, CODEWORDS, dsub):
        raise ValueError(f"codebooks must be float32 [{M}, {CODEWORDS}, {dsub}], got {cb.dtype} {tuple(cb.shape)}")
    return cb.contiguous()


def encode_device(rows, codebooks, dim: int, dsub: int):
    """``srx_pq_encode(tiled=0)``: f32[n, >= dim] device rows (the first ``dim`` columns are read) -> u8[n, M]; asynchronous."""
    torch, L = _torch(), _capi.lib()
    x, ld = _f32_rows(torch, rows, "rows")
    n, M = int(x.shape[0]), subspaces(dim, dsub)
    if int(x.shape[1]) < dim:
        raise ValueError(f"rows have {int(x.shape[1])} columns, the codebooks speak of {dim}")
    with torch.cuda.device(x.device):
        out = torch.empty((n, M), dtype=torch.uint8, device=x.device)
        _capi.check(L.srx_pq_encode(x.device.index or 0, _ptr(x), ld, n, dim, dsub, 0, n, _ptr(codebooks), 0, _ptr(out), _stream_ptr(torch, x.device)),
                    "srx_pq_encode")
    return out


def initial_codebooks(x, dsub: int, seed: int = 0):
    """f32[M, 256, dsub]: codeword c of every subspace is the sub-vector of row ``randperm(n, seed)[c]`` of ``x`` (one CPU
    permutation for all subspaces, columns past dim are zeros); with fewer than 256 rows the remaining codewords repeat row 0."""
    torch = _torch()
    n, dim = int(x.shape[0]), int(x.shape[1])
    M = subspaces(dim, dsub)
    pick = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))[:CODEWORDS]
    pick = torch.cat([pick, torch.zeros(CODEWORDS - int(pick.numel()), dtype=pick.dtype)]).to(x.device)
    rows = torch.zeros((CODEWORDS, M * dsub), dtype=torch.float32, device=x.device)
    rows[:, :dim] = x[pick]
    return rows.reshape(CODEWORDS, M, dsub).permute(1, 0, 2).contiguous()


def train_codebooks(x, dsub: int = 8, n_iter: int = 8, seed: int = 0):
    """Lloyd's iteration on f32[n, dim] device rows -> f32[M, 256, dsub] device codebooks.  Starts from
    :func:`initial_codebooks`; each iteration assigns every row in all subspaces with ONE launch (``srx_pq_encode``, ties to the
    lowest code) and updates each subspace with ``ivf.members_of`` + ``ivf.update_device`` on its columns (that call's summation
    order; an empty codeword keeps its previous value).  Deterministic: the same bits every time for a seed."""
    torch = _torch()
    _require_f32(x, "rows")
    n, dim = int(x.shape[0]), int(x.shape[1])
    M = subspaces(dim, dsub)
    if n < 1:
        raise ValueError("training needs at least one row")
    with torch.cuda.device(x.device):
        cb = initial_codebooks(x, dsub, seed)
        if int(n_iter) > 0:
            xp = torch.zeros((n, M * dsub), dtype=torch.float32, device=x.device)  # the zero columns past dim, for the updates
            xp[:, :dim] = x
        for _ in range(int(n_iter)):
            codes = encode_device(xp, cb, dim, dsub)
            nxt = torch.empty_like(cb)
            for m in range(M):
                ptr, member = ivf.members_of(codes[:, m].to(torch.int32), CODEWORDS)
                nxt[m] = ivf.update_device(xp[:, m * dsub: (m + 1) * dsub], ptr, member, cb[m])
            cb = nxt
    return cb


class DensePqIndex(_DenseIndex):
    """8-bit product codes of an embedding matrix resident in HBM (include/pq/sparse_rx_pq.h), kept ONLY in the 64-row tiles the
    scan reads, plus the codebooks f32[M, 256, dsub].  Scores are the sums of the queries' table entries: the inner products of
    the f32 queries with the RECONSTRUCTED rows, in the header's fp32 order.  No MMR selection."""

    _score_entry = "srx_pq_score_docs"

    def __init__(self, embeddings, dsub: int = 8, codebooks=None, n_iter: int = 8, seed: int = 0, train_rows: int = 65536, device="cuda:0",
                 doc_base: int = 0, chunk_rows=None):
        """``embeddings``: f32[n_docs, dim], a device tensor or a host array, possibly a read-only memory map (encoded
        ``chunk_rows`` rows at a time through one staging tensor, a multiple of 64; default: 64 MB of rows).  ``codebooks``
        f32[M, 256, dsub] (host or device) builds with no training; otherwise :func:`train_codebooks` runs ``n_iter`` iterations
        on ``train_rows`` rows picked by a seeded permutation (None: all rows)."""
        _require_f32(embeddings, "embeddings")
        torch = self._open(device)
        self.n_docs, self.dim = int(embeddings.shape[0]), int(embeddings.shape[1])
        if self.n_docs == 0:
            raise ValueError("Empty corpus provided")
        self.dsub = int(dsub)
        self.M = subspaces(self.dim, self.dsub)
        self.doc_base = int(doc_base)
        if isinstance(embeddings, torch.Tensor) and not embeddings.is_cuda:
            embeddings = embeddings.numpy()  # a host tensor is a host array: read in chunks, never uploaded whole
        on_device = isinstance(embeddings, torch.Tensor)
        rows = max(TILE_ROWS, ((64 << 20) // (4 * self.dim)) // TILE_ROWS * TILE_ROWS) if chunk_rows is None else int(chunk_rows)
        if rows < TILE_ROWS or rows % TILE_ROWS != 0:
            raise ValueError(f"chunk_rows must be a positive multiple of {TILE_ROWS}, got {chunk_rows}")
        L = _capi.lib()
        with torch.cuda.device(self.device):
            if codebooks is None:
                m = self.n_docs if train_rows is None else max(1, min(int(train_rows), self.n_docs))
                if on_device and m == self.n_docs:
                    sample = embeddings.to(self.device)
                else:
                    pick = torch.randperm(self.n_docs, generator=torch.Generator().manual_seed(int(seed)))[:m].sort().values
                    sample = embeddings.to(self.device)[pick.to(self.device)] if on_device else \
                        torch.from_numpy(np.asarray(embeddings[pick.numpy()], dtype=np.float32)).to(self.device)
                self.codebooks = train_codebooks(sample, self.dsub, n_iter, seed)
                del sample
            else:
                self.codebooks = _check_codebooks(torch, codebooks, self.M, self.dsub, self.device)
            nbytes = _capi.check(L.srx_pq_bytes(self.n_docs, self.M), "srx_pq_bytes")
            self.codes = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            if on_device:
                self._encode(torch, L, embeddings.to(self.device), 0)
            else:
                stage = torch.empty((min(rows, self.n_docs), self.dim), dtype=torch.float32, device=self.device)
                for lo in range(0, self.n_docs, rows):
                    chunk = torch.from_numpy(np.array(embeddings[lo: lo + rows], dtype=np.float32))  # np.array copies the chunk only
                    n = int(chunk.shape[0])
                    stage[:n].copy_(chunk)  # stream-ordered behind the previous chunk's kernel
                    self._encode(torch, L, stage[:n], lo)
            # the largest norm of a reconstructed row over the columns a query has (fp64), in chunks of tiles
            cw2 = self.codebooks.double().reshape(self.M, CODEWORDS, self.dsub) ** 2
            live = (torch.arange(self.M * self.dsub, device=self.device) < self.dim).reshape(self.M, 1, self.dsub)
            cw2 = (cw2 * live).sum(dim=2)  # [M, 256]
            sub = torch.arange(self.M, device=self.device)[None, :]
            best = torch.zeros((), dtype=torch.float64, device=self.device)
            for lo in range(0, self.n_docs, rows):
                c = self._untiled(torch, lo, min(lo + rows, self.n_docs)).long()
                best = torch.maximum(best, cw2[sub, c].sum(dim=1).max())
            self._max_norm = float(best.item()) ** 0.5

    def _encode(self, torch, L, x, row0: int) -> None:
        x, ld = _f32_rows(torch, x, "embeddings")
        _capi.check(L.srx_pq_encode(self.device.index or 0, _ptr(x), ld, int(x.shape[0]), self.dim, self.dsub, row0, self.n_docs, _ptr(self.codebooks), 1,
                                    _ptr(self.codes), _stream_ptr(torch, self.device)), "srx_pq_encode")

    def _untiled(self, torch, lo: int, hi: int):
        """u8[hi - lo, M] on the device: rows lo .. hi - 1 of the tiled codes (``lo`` a multiple of 64)."""
        np_, t0, t1 = -(-self.M // 16), lo // TILE_ROWS, -(-hi // TILE_ROWS)
        t = self.codes[t0 * np_ * 1024: t1 * np_ * 1024].reshape(t1 - t0, np_, 64, 16).permute(0, 2, 1, 3)
        return t.reshape((t1 - t0) * 64, np_ * 16)[: hi - lo, : self.M]

    @classmethod
    def from_embeddings(cls, emb, dsub: int = 8, codebooks=None, n_iter: int = 8, seed: int = 0, train_rows: int = 65536, device="cuda:0",
                        doc_base: int = 0, chunk_rows=None):
        """The constructor under the name the other dense indexes give theirs."""
        return cls(emb, dsub=dsub, codebooks=codebooks, n_iter=n_iter, seed=seed, train_rows=train_rows, device=device, doc_base=doc_base,
                   chunk_rows=chunk_rows)

    # ---- what the index holds ----
    def device_bytes(self) -> int:
        """Bytes resident: the codes (``srx_pq_bytes``) and the codebooks."""
        return int(self.codes.numel() + 4 * self.codebooks.numel())

    def codes_to_host(self) -> np.ndarray:
        """u8[n_docs, M]: the codes, untiled."""
        _torch().cuda.synchronize(self.device)
        return untile_host(self.codes.cpu().numpy(), self.n_docs, self.M)

    def codebooks_to_host(self) -> np.ndarray:
        """f32[M, 256, dsub]."""
        return self.codebooks.cpu().numpy()

    def reconstruct(self, docs) -> np.ndarray:
        """f32[len(docs), dim]: the rows the scores are of, for LOCAL row numbers ``docs`` (a torch gather, not a hot path)."""
        torch = _torch()
        d = torch.as_tensor(np.asarray(docs, dtype=np.int64), device=self.device)
        if d.numel() and (int(d.min()) < 0 or int(d.max()) >= self.n_docs):
            raise ValueError(f"reconstruct: rows must be in [0, {self.n_docs})")
        np_ = -(-self.M // 16)
        piece = torch.arange(np_, device=self.device)[None, :]
        at = (((d >> 6)[:, None] * np_ + piece) * 64 + (d & 63)[:, None]) * 16  # [n, pieces]: the byte of each piece
        codes = self.codes[(at[:, :, None] + torch.arange(16, device=self.device)).reshape(len(d), -1)[:, : self.M].long()].long()
        rows = self.codebooks[torch.arange(self.M, device=self.device)[None, :], codes]  # [n, M, dsub]
        return rows.reshape(len(d), -1)[:, : self.dim].cpu().numpy()

    def max_row_norm(self) -> float:
        """Largest Euclidean norm of a RECONSTRUCTED row over its ``dim`` columns (fp64), computed in chunks at build."""
        return self._max_norm

    # ---- doors ----
    def _padded(self, torch, queries, dtype):
        """The kernels supply the zero columns themselves: the queries go as they are (row stride = dim)."""
        if int(queries.shape[1]) != self.dim:
            raise ValueError(f"queries have {int(queries.shape[1])} columns, the index {self.dim}")
        return queries.to(device=self.device, dtype=dtype).contiguous()

    def encode_device(self, rows_f32):
        """f32[n, dim] device rows -> u8[n, M], the codes the index would give them (``srx_pq_encode``, plain layout)."""
        return encode_device(self._padded(_torch(), rows_f32, _torch().float32), self.codebooks, self.dim, self.dsub)

    def lut_device(self, queries_f32):
        """``srx_pq_lut``: f32[nq, dim] device queries -> f32[nq, M, 256], the tables the scan adds up; asynchronous."""
        torch = _torch()
        with torch.cuda.device(self.device):
            q = self._padded(torch, queries_f32, torch.float32)
            nq = int(q.shape[0])
            out = torch.empty((nq, self.M, CODEWORDS), dtype=torch.float32, device=self.device)
            _capi.check(_capi.lib().srx_pq_lut(self.device.index or 0, _ptr(self.codebooks), self.dim, self.dsub, _ptr(q), self.dim, nq, _ptr(out),
                                               _stream_ptr(torch, self.device)), "srx_pq_lut")
        return out

    def search_device(self, queries_f32, k: int, score_offset: float = 0.0, filter=None, q_filter=None):
        """f32[nq, dim] queries on the device -> (doc i32[nq,k], score f32[nq,k], count i32[nq]); asynchronous.  Top-k of
        fl32(score + score_offset) > 0, the returned scores carry the offset; ``filter`` / ``q_filter`` as
        ``DeviceIndex.search_device``."""
        torch = _torch()
        _check_k(k)
        L = _capi.lib()
        with torch.cuda.device(self.device):
            q = self._padded(torch, queries_f32, torch.float32)
            nq = int(q.shape[0])
            out = _empty_topk(torch, nq, k, self.device)
            if nq == 0:
                return out
            ws = _grow_ws(torch, self, _capi.check(L.srx_pq_workspace_bytes(nq, self.n_docs, self.M, k), "srx_pq_workspace_bytes"))
            fdesc, keep = resolve_filter(self, filter, q_filter, nq)  # keep: alive until the call has been issued
            _capi.check(L.srx_pq_search(self.device.index or 0, _ptr(self.codes), self.n_docs, self.dim, self.dsub, _ptr(self.codebooks), _ptr(q), self.dim,
                                        nq, k, self.doc_base, fdesc, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(ws), ws.numel(),
                                        _stream_ptr(torch, self.device), float(score_offset)), "srx_pq_search")
            del keep
        return out

    def search(self, queries: np.ndarray, k: int, score_offset: float = 0.0, filter=None, q_filter=None):
        """Host arrays in, host arrays out; ``q_filter``: a host sequence of row numbers, validated here."""
        q = self._queries_to_device(queries)
        return self._host(self.search_device(q, k, score_offset, filter=filter, q_filter=host_q_filter(self, filter, q_filter, int(q.shape[0]))))

    def _queries_to_device(self, queries):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        return _torch().as_tensor(q, device=self.device)

    def score_docs_device(self, queries_f32, cand_doc, cand_count=None, out=None):
        """``srx_pq_score_docs``: as ``DenseF32Index.score_docs_device``; the bits are those of :meth:`search_device` with
        ``score_offset = 0``."""
        return self._score_docs_device(queries_f32, _torch().float32, cand_doc, cand_count, out)

    def _launch_score(self, L, q, nq, cand_doc, cand_count, m, out, stream):
        return L.srx_pq_score_docs(self.device.index or 0, _ptr(self.codes), self.n_docs, self.dim, self.dsub, _ptr(self.codebooks), _ptr(q), self.dim,
                                   nq, self.doc_base, _ptr(cand_doc), _ptr(cand_count), m, _ptr(out), stream)

    def score_docs(self, queries: np.ndarray, cand_doc, cand_count=None) -> np.ndarray:
        """Host arrays in (the candidates validated by :func:`validate_candidates`), f32[nq, m] out."""
        q = self._queries_to_device(queries)
        return self._score_docs(cand_doc, cand_count, int(q.shape[0]), lambda cd, cc: self.score_docs_device(q, cd, cc))
