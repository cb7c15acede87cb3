"""MX dense index (include/mx/sparse_rx_mx.h): MXFP8 / MXFP4 rows, one e8m0 scale per 32 columns, searched by the
block-scaled MFMA of gfx950.  No reference counterpart.  :class:`DenseMxIndex` has the doors of ``DenseHalfIndex`` (filters,
``score_offset``, the scorer of given docs) without the MMR selection."""
import numpy as np

from . import _capi
from .dense import _DenseIndex, _f32_rows, _quantize_corpus, _require_f32
from .filter import host_q_filter
from .index import _ptr, _stream_ptr, _torch

MX_TYPES = {"mxfp8": _capi.SRX_MX_FP8, "mxfp4": _capi.SRX_MX_FP4}
FP4_VALUES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])  # e2m1 codes 0 .. 7; bit 3 is the sign


def check_mx_dtype(dtype) -> str:
    d = str(dtype).lower()
    if d not in MX_TYPES:
        raise ValueError(f"dtype must be 'mxfp8' or 'mxfp4', got {dtype!r}")
    return d


def unpack_mx_host(buf: np.ndarray, dtype: str, n_docs: int, dim_pad: int):
    """``(codes u8[n_docs, dim_pad], scale codes u8[n_docs, dim_pad // 32])`` of a buffer in the order
    include/mx/sparse_rx_mx.h documents (host arrays); an FP4 code is a value 0 .. 15."""
    buf = np.asarray(buf).view(np.uint8)
    ks, tiles = dim_pad // 64, -(-n_docs // 32)
    sg = -(-ks // 4)
    nbytes = tiles * 32 * dim_pad // (1 if dtype == "mxfp8" else 2)
    codes = buf[:nbytes]
    if dtype == "mxfp4":  # [tile][k-step][half h][row][columns 32 h .. + 31]; column 2 i: the low nibble of byte i
        codes = np.stack([codes & 15, codes >> 4], axis=-1).reshape(tiles, ks, 2, 32, 32).transpose(0, 3, 1, 2, 4)
    else:  # [tile][k-step][half h][row][block b][columns 32 b + 16 h .. + 15]
        codes = codes.reshape(tiles, ks, 2, 32, 2, 16).transpose(0, 3, 1, 4, 2, 5)
    codes = codes.reshape(-1, dim_pad)[:n_docs]
    sc = buf[nbytes:].reshape(tiles, sg, 2, 32, 4).transpose(0, 3, 1, 4, 2).reshape(tiles * 32, sg * 8)[:n_docs, : 2 * ks]  # [row][k-step][half]
    return np.ascontiguousarray(codes), np.ascontiguousarray(sc)


def dequantize_mx_host(codes: np.ndarray, scales: np.ndarray, dtype: str) -> np.ndarray:
    """f64[n, columns]: element value * 2^(scale code - 127) (every such value is also exact in float32 unless it is below
    its subnormal range)."""
    c = codes.astype(np.int64)
    if dtype == "mxfp4":
        v = FP4_VALUES[c & 7] * np.where(c & 8, -1.0, 1.0)
    else:
        e, m = (c >> 3) & 15, c & 7
        v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e.astype(np.float64) - 10)) * np.where(c & 128, -1.0, 1.0)
    return v * np.repeat(2.0 ** (scales.astype(np.float64) - 127), 32, axis=1)[:, : c.shape[1]]


class DenseMxIndex(_DenseIndex):
    """Embedding matrix resident in HBM as MXFP8 (e4m3) or MXFP4 (e2m1) codes with a power-of-two scale per 32 columns, kept ONLY
    in the operand order the scaled MFMA reads.  Queries are quantised to MXFP8 by the search.  Scores are the dot products of
    the DEQUANTISED rows and queries, accumulated in fp32 by the instruction.  No MMR selection."""

    _workspace_fn, _entry, _score_entry = "srx_mx_workspace_bytes", "srx_mx_search", "srx_mx_score_docs"
    _filtered_entry = "srx_mx_search"  # one entry point, the filter optional

    def __init__(self, embeddings, dtype="mxfp8", device="cuda:0", doc_base: int = 0, chunk_rows=None):
        """``embeddings``: f32[n_docs, dim], a device tensor (one launch) or a host array, possibly a read-only memory map
        (uploaded ``chunk_rows`` rows at a time, a multiple of 32).  ``ValueError`` for a row with a NaN or an inf, raised
        after the one synchronisation the build needs; every finite row is representable."""
        self.dtype = check_mx_dtype(dtype)
        _require_f32(embeddings, "embeddings")
        torch = self._open(device)
        self.n_docs, self.dim = int(embeddings.shape[0]), int(embeddings.shape[1])
        if self.n_docs == 0:
            raise ValueError("Empty corpus provided")
        self.dim_pad = self._pad64(self.dtype)
        self.doc_base = int(doc_base)
        self._max_norm = None
        L = _capi.lib()
        with torch.cuda.device(self.device):
            nbytes = _capi.check(L.srx_mx_bytes(MX_TYPES[self.dtype], self.n_docs, self.dim_pad), "srx_mx_bytes")
            self.corpus = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _quantize_corpus(self, torch, embeddings, chunk_rows, None, (), convert=lambda x, row0, flag: self._convert(torch, L, x, row0, flag),
                             refusal="embeddings hold a non-finite value (NaN / inf)")

    def _convert(self, torch, L, x, row0: int, flag) -> None:
        x, ld = _f32_rows(torch, x, "embeddings")
        _capi.check(L.srx_mx_convert(self.device.index or 0, MX_TYPES[self.dtype], _ptr(x), ld, int(x.shape[0]), self.dim, self.dim_pad, row0,
                                     self.n_docs, _ptr(self.corpus), _ptr(flag), _stream_ptr(torch, self.device)), "srx_mx_convert")

    @classmethod
    def from_embeddings(cls, emb, dtype="mxfp8", device="cuda:0", doc_base: int = 0, chunk_rows=None):
        """The constructor under the name the quantised indexes give theirs."""
        return cls(emb, dtype=dtype, device=device, doc_base=doc_base, chunk_rows=chunk_rows)

    def device_bytes(self) -> int:
        """Bytes of the resident corpus (``srx_mx_bytes``)."""
        return int(self.corpus.numel())

    def corpus_to_host(self):
        """``(codes u8[n_docs, dim], scale codes u8[n_docs, dim_pad // 32])``, row-major."""
        _torch().cuda.synchronize(self.device)
        codes, scales = unpack_mx_host(self.corpus.cpu().numpy(), self.dtype, self.n_docs, self.dim_pad)
        return np.ascontiguousarray(codes[:, : self.dim]), scales

    def dequantized_to_host(self) -> np.ndarray:
        """f64[n_docs, dim]: the rows the scores are of."""
        return dequantize_mx_host(*self.corpus_to_host(), self.dtype)

    def max_row_norm(self) -> float:
        """Largest Euclidean norm of the DEQUANTISED rows (fp64), computed once from a host copy."""
        if self._max_norm is None:
            x = self.dequantized_to_host()
            self._max_norm = float((x * x).sum(axis=1).max()) ** 0.5
        return self._max_norm

    def search_device(self, queries_f32, k: int, score_offset: float = 0.0, filter=None, q_filter=None):
        """f32[nq, dim] queries on the device (quantised to MXFP8 by the search) -> (doc i32[nq,k], score f32[nq,k],
        count i32[nq]); asynchronous.  Top-k of (score + score_offset) > 0, the returned scores carry the offset; ``filter`` /
        ``q_filter`` as ``DeviceIndex.search_device``."""
        return self._search_device(queries_f32, _torch().float32, k, score_offset, filter=filter, q_filter=q_filter)

    def _launch_filtered(self, L, q, nq, k, out, ws, stream, fdesc, score_offset):
        return L.srx_mx_search(self.device.index or 0, MX_TYPES[self.dtype], _ptr(self.corpus), self.n_docs, self.dim_pad, _ptr(q), nq, k,
                               self.doc_base, fdesc, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(ws), ws.numel(), stream, float(score_offset))

    def _launch(self, L, q, nq, k, out, ws, stream, score_offset):
        return self._launch_filtered(L, q, nq, k, out, ws, stream, None, score_offset)

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
        """``srx_mx_score_docs``: as ``DenseF32Index.score_docs_device``; the bits are those of :meth:`search_device` with
        ``score_offset = 0``."""
        return self._score_docs_device(queries_f32, _torch().float32, cand_doc, cand_count, out)

    def _launch_score(self, L, q, nq, cand_doc, cand_count, m, out, stream):
        return L.srx_mx_score_docs(self.device.index or 0, MX_TYPES[self.dtype], _ptr(self.corpus), self.n_docs, self.dim_pad, _ptr(q), nq,
                                   self.doc_base, _ptr(cand_doc), _ptr(cand_count), m, _ptr(out), stream)

    def score_docs(self, queries: np.ndarray, cand_doc, cand_count=None) -> np.ndarray:
        """Host arrays in (the candidates validated by :func:`validate_candidates`), f32[nq, m] out."""
        q = self._queries_to_device(queries)
        return self._score_docs(cand_doc, cand_count, int(q.shape[0]), lambda cd, cc: self.score_docs_device(q, cd, cc))
