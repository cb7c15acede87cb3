"""Dense INT8 side of the same service: the reference's ``QuantizedEmbeddingRetriever`` hot path,
``quantized_dot_product_batch`` + top-k (rag_system/core/retriever_registry.py:90-117, 435-463, 465-524), on the HIP
engine (``srx_dense_search_i8``: one MFMA int8 GEMM, fp64 scaling like the reference's NumPy scalars, exact top-k), and
its asymmetric uint8 scheme (:449-462, 550-559; ``srx_dense_search_u8``).

Embedding *generation* stays outside (the reference simulates it from ``hash(text)``); this module starts from the
embeddings, like the kernel-level functions of the reference do."""
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import _capi
from .filter import host_q_filter, resolve_filter
from .index import (_candidate_block, _check_k, _empty_topk, _grow_ws, _ptr, _stream_ptr, _to_host, _torch, rows_to_dict,
                    validate_candidates)

DIMS = (32, 64, 96, 128, 192, 256, 384, 512, 768, 1024)  # row lengths the kernel is instantiated for


def quantize_symmetric(embeddings: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """retriever_registry.py:437-447: per-row scale = max |x| (>= 1e-8), int8 = round(x / scale * 127)."""
    e = np.asarray(embeddings)
    scales = np.maximum(np.max(np.abs(e), axis=1, keepdims=True), 1e-8)
    q = np.round(e / scales * 127.0).astype(np.int8)
    return q, scales.flatten().astype(np.float32)


def quantize_query_symmetric(query_embedding: np.ndarray) -> Tuple[np.ndarray, np.float32]:
    """retriever_registry.py:482-485: int8 = round(x / max|x| * 127), query scale = max|x| / 127 (as f32)."""
    x = np.asarray(query_embedding)
    s = np.max(np.abs(x))
    return np.round(x / s * 127.0).astype(np.int8), np.array([s / 127.0], dtype=np.float32)[0]


def quantize_asymmetric(embeddings: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """retriever_registry.py:449-462: per-row min / max, scale = (max - min) / 255 (>= 1e-8), u8 = round((x - min) / scale);
    the table is all scales followed by all mins (f32[2 n]), exactly as the reference stores it."""
    e = np.asarray(embeddings)
    min_vals = np.min(e, axis=1, keepdims=True)
    max_vals = np.max(e, axis=1, keepdims=True)
    scales = np.maximum((max_vals - min_vals) / 255.0, 1e-8)
    q = np.round((e - min_vals) / scales).astype(np.uint8)
    return q, np.concatenate([scales.flatten(), min_vals.flatten()]).astype(np.float32)


def quantize_query_asymmetric(query_embedding: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """retriever_registry.py:486-491: u8 = round((x - min) / ((max - min) / 255)), query_scales = f32[scale, min]."""
    x = np.asarray(query_embedding)
    qmin, qmax = np.min(x), np.max(x)
    scale = (qmax - qmin) / 255.0
    return np.round((x - qmin) / scale).astype(np.uint8), np.array([scale, qmin], dtype=np.float32)


def dequantize_query_asymmetric(query_uint8: np.ndarray, query_scales: np.ndarray) -> np.ndarray:
    """retriever_registry.py:555: query_fp32 = u8.astype(f32) * query_scale + query_min (f32 scalars)."""
    query_scale, query_min = query_scales
    return query_uint8.astype(np.float32) * query_scale + query_min


def check_quantize_arg(quantize) -> str:
    """``quantize=`` of the API mirrors: "host" (the NumPy quantisers above) or "device" (``include/sparse_rx_quant.h``)."""
    q = str(quantize).lower()
    if q not in ("host", "device"):
        raise ValueError(f"quantize must be 'host' or 'device', got {quantize!r}")
    return q


def _require_f32(x, what: str) -> None:
    """The device quantisers take float32 only: no silent cast, because the host functions compute in the dtype they are given."""
    dtype = getattr(x, "dtype", None)
    if dtype is None or str(dtype).split(".")[-1] != "float32":
        raise ValueError(f"{what} must be float32, got {dtype} (the device quantisers do not cast)")
    if len(x.shape) != 2:
        raise ValueError(f"{what} must be 2-D [rows, dim], got shape {tuple(x.shape)}")


def _f32_rows(torch, x, what: str):
    """A 2-D float32 device tensor as the quantisers read it -> (tensor with unit column stride, row stride in elements)."""
    _require_f32(x, what)
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"{what} must be a device tensor")
    n, dim = int(x.shape[0]), int(x.shape[1])
    if dim > 0 and (x.stride(1) != 1 or (n > 1 and x.stride(0) < dim)):
        x = x.contiguous()
    return x, (int(x.stride(0)) if n > 1 else dim)


def _quantize_device(entry: str, x, dim_pad: int, outs, flag=None, row0: int = 0, n_total=None, packed=None):
    """One launch of a quantiser of include/sparse_rx_quant.h on the current stream of ``x``'s device.  ``outs``: the
    entry point's output tensors in its order (None = NULL).  Returns the flag tensor i32[1] (made and zeroed when not given)."""
    torch = _torch()
    x, ld = _f32_rows(torch, x, "embeddings")
    dev = x.device
    n, dim = int(x.shape[0]), int(x.shape[1])
    with torch.cuda.device(dev):
        if flag is None:
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
        args = [dev.index or 0, _ptr(x), ld, n, dim, dim_pad]
        if n_total is not None:  # a corpus call: a chunk of the whole
            args += [row0, n_total] + ([int(packed)] if packed is not None else [])
        args += [_ptr(t) for t in outs] + [_ptr(flag), _stream_ptr(torch, dev)]
        _capi.check(getattr(_capi.lib(), entry)(*args), entry)
    return flag


def _pad64(dim: int, engine: str) -> int:
    dim_pad = (dim + 63) // 64 * 64
    if dim_pad > 1024:
        raise ValueError(f"embedding dim {dim} > 1024 is not supported by the {engine} engine")
    return dim_pad


def quantize_symmetric_device(emb):
    """:func:`quantize_symmetric` on the device (``srx_dense_quantize_i8``): f32[n, dim] device tensor -> (i8[n, dim] -- a view
    of the zero-padded i8[n, dim_pad] the INT8 engine takes --, f32[n] scales, flag i32[1]), bit for bit the host function's.
    Asynchronous on the current stream.  Flag bit 0: a row holds a non-finite value (codes 0, scale 1e-8)."""
    torch = _torch()
    _require_f32(emb, "embeddings")
    n, dim = int(emb.shape[0]), int(emb.shape[1])
    dim_pad = _pad_dim(dim)
    codes = torch.empty((n, dim_pad), dtype=torch.int8, device=emb.device)
    scales = torch.empty((n,), dtype=torch.float32, device=emb.device)
    flag = _quantize_device("srx_dense_quantize_i8", emb, dim_pad, (codes, scales), n_total=n, packed=0)
    return codes[:, :dim], scales, flag


def quantize_asymmetric_device(emb):
    """:func:`quantize_asymmetric` on the device (``srx_dense_quantize_u8``): -> (u8[n, dim] view of u8[n, dim_pad], the
    f32[2 n] table -- all scales, then all minima --, flag i32[1])."""
    torch = _torch()
    _require_f32(emb, "embeddings")
    n, dim = int(emb.shape[0]), int(emb.shape[1])
    dim_pad = _pad64(dim, "uint8")
    codes = torch.empty((n, dim_pad), dtype=torch.uint8, device=emb.device)
    scales = torch.empty((2 * n,), dtype=torch.float32, device=emb.device)
    flag = _quantize_device("srx_dense_quantize_u8", emb, dim_pad, (codes, scales), n_total=n)
    return codes[:, :dim], scales, flag


def quantize_queries_symmetric_device(q):
    """:func:`quantize_query_symmetric` for a batch (``srx_dense_quantize_queries_i8``): f32[nq, dim] device tensor ->
    (i8[nq, dim] view of i8[nq, dim_pad], f32[nq] query scales, flag i32[1]).  Flag bit 0: a non-finite query, bit 1: an
    all-zero one; both get codes 0 and scale 0, so every score of theirs is 0 (the host function divides by zero there)."""
    torch = _torch()
    _require_f32(q, "queries")
    nq, dim = int(q.shape[0]), int(q.shape[1])
    dim_pad = _pad_dim(dim)
    codes = torch.empty((nq, dim_pad), dtype=torch.int8, device=q.device)
    scales = torch.empty((nq,), dtype=torch.float32, device=q.device)
    flag = _quantize_device("srx_dense_quantize_queries_i8", q, dim_pad, (codes, scales))
    return codes[:, :dim], scales, flag


def quantize_queries_asymmetric_device(q, codes: bool = True):
    """:func:`quantize_query_asymmetric` + :func:`dequantize_query_asymmetric` for a batch
    (``srx_dense_quantize_queries_u8``): -> (u8[nq, dim], f32[nq, 2] = (scale, min), de-quantised f32[nq, dim], flag i32[1]);
    the three are views of dim_pad-wide zero-padded tensors.  ``codes=False``: only the de-quantised block is written (the
    first two are None).  Flag bit 0: a non-finite query (block 0), bit 1: a constant one (the block is the query itself)."""
    torch = _torch()
    _require_f32(q, "queries")
    nq, dim = int(q.shape[0]), int(q.shape[1])
    dim_pad = _pad64(dim, "uint8")
    u8 = torch.empty((nq, dim_pad), dtype=torch.uint8, device=q.device) if codes else None
    scales = torch.empty((nq, 2), dtype=torch.float32, device=q.device) if codes else None
    deq = torch.empty((nq, dim_pad), dtype=torch.float32, device=q.device)
    flag = _quantize_device("srx_dense_quantize_queries_u8", q, dim_pad, (u8, scales, deq))
    return (u8[:, :dim] if codes else None), scales, deq[:, :dim], flag


def unpack_i8_host(packed: np.ndarray, n_docs: int, dim_pad: int) -> np.ndarray:
    """The row-major i8[n_docs, dim_pad] of a corpus in the fragment order ``srx_dense_pack_i8`` documents (host arrays)."""
    ks = dim_pad // 32
    t = np.asarray(packed).view(np.int8).reshape(-1, ks, 2, 32, 16)  # [tile][k-step][half][row][16 bytes]
    return np.ascontiguousarray(t.transpose(0, 3, 1, 2, 4)).reshape(-1, dim_pad)[:n_docs]


def unpack_half_host(packed: np.ndarray, n_docs: int, dim_pad: int) -> np.ndarray:
    """The row-major u16[n_docs, dim_pad] codes of a corpus in the fragment order include/sparse_rx_half.h documents (host
    arrays): view them as ``np.float16``, or shift them left by 16 into ``float32`` bits for bf16."""
    ks = dim_pad // 16
    t = np.asarray(packed).view(np.uint16).reshape(-1, ks, 2, 32, 8)  # [tile][k-step][half][row][8 elements]
    return np.ascontiguousarray(t.transpose(0, 3, 1, 2, 4)).reshape(-1, dim_pad)[:n_docs]


def _default_chunk_rows(dim: int) -> int:
    return max(32, ((64 << 20) // (4 * max(1, dim))) // 32 * 32)  # <= 64 MB of f32 rows, a multiple of the 32-row tile


def _quantize_corpus(index, torch, emb, chunk_rows, entry: str, outs, packed=None, convert=None,
                     refusal="embeddings hold a non-finite value (NaN / inf, or a row whose max - min overflows)"):
    """``from_embeddings``' loop: a device tensor is quantised in one launch; a host array (possibly a read-only memory map) is
    copied through ONE staging tensor of ``chunk_rows`` rows, so the device holds the finished corpus plus one chunk.  Ends
    with the build's one synchronisation, the read of the flag word.  ``convert(chunk, row0, flag)``: the per-chunk launch of
    an index whose entry point is not a quantiser of include/sparse_rx_quant.h (``entry`` and ``outs`` are then unused)."""
    _require_f32(emb, "embeddings")
    n = index.n_docs
    flag = torch.zeros(1, dtype=torch.int32, device=index.device)
    if convert is None:
        def convert(chunk, row0, flag):
            _quantize_device(entry, chunk, index.dim_pad, outs, flag, row0, n, packed)
    if isinstance(emb, torch.Tensor):
        convert(emb.to(index.device), 0, flag)
    else:
        rows = _default_chunk_rows(index.dim) if chunk_rows is None else int(chunk_rows)
        if rows < 32 or rows % 32 != 0:
            raise ValueError(f"chunk_rows must be a positive multiple of 32, got {chunk_rows}")
        stage = torch.empty((min(rows, n), index.dim), dtype=torch.float32, device=index.device)
        for lo in range(0, n, rows):
            chunk = torch.from_numpy(np.array(emb[lo: lo + rows], dtype=np.float32))  # np.array copies the chunk only
            m = int(chunk.shape[0])
            stage[:m].copy_(chunk)  # stream-ordered behind the previous chunk's kernel
            convert(stage[:m], lo, flag)
    if int(flag.item()) & _capi.SRX_QUANT_NONFINITE:
        raise ValueError(refusal)


def _pad_dim(dim: int) -> int:
    for d in DIMS:
        if d >= dim:
            return d
    raise ValueError(f"embedding dim {dim} > {DIMS[-1]} is not supported by the INT8 engine")


class _DenseIndex:
    """What the three dense indexes share; each keeps how its corpus is stored and which entry point it calls."""

    _workspace_fn = "srx_dense_f32_workspace_bytes"
    _entry = None  # the search entry point ``_launch`` calls, as ``_capi.check`` names it
    _filtered_entry = None  # the one ``_launch_filtered`` calls, when it is not ``_entry + "_filtered"``

    def _open(self, device):
        """The no-GPU refusal, the library and the device: first step of every constructor."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise _capi.SparseRxUnavailable(f"no HIP device visible: {type(self).__name__} needs a GPU (there is no CPU fallback)")
        _capi.lib()
        self.device = torch.device(device)
        self._ws = None
        return torch

    def _pad64(self, engine: str) -> int:
        """Row length rounded up to the 64 columns the f32 / uint8 kernels step by."""
        return _pad64(self.dim, engine)

    def _search_device(self, queries, dtype, k: int, *extra, filter=None, q_filter=None):
        """k check, the query block zero-padded to ``dim_pad``, the output triple and the workspace, then the class's
        ``_launch(L, q, nq, k, out, ws, stream, *extra)`` -> the entry point's return code.  An empty batch launches nothing.
        With a ``filter`` (a :class:`~.filter.DocFilter` over this index's rows; ``q_filter`` int32 device tensor [nq] or None)
        the class's ``_launch_filtered(L, q, nq, k, out, ws, stream, fdesc, *extra)`` (include/sparse_rx_filter.h)."""
        torch = _torch()
        _check_k(k)
        nq = int(queries.shape[0])
        L = _capi.lib()
        with torch.cuda.device(self.device):
            q = self._padded(torch, queries, dtype)
            out = _empty_topk(torch, nq, k, self.device)
            if nq == 0:
                return out
            ws = _grow_ws(torch, self, _capi.check(getattr(L, self._workspace_fn)(nq, self.n_docs, k), self._workspace_fn))
            fdesc, keep = resolve_filter(self, filter, q_filter, nq)  # keep: alive until the call has been issued
            if fdesc is None:
                _capi.check(self._launch(L, q, nq, k, out, ws, _stream_ptr(torch, self.device), *extra), self._entry)
            else:
                _capi.check(self._launch_filtered(L, q, nq, k, out, ws, _stream_ptr(torch, self.device), fdesc, *extra),
                            self._filtered_entry or self._entry + "_filtered")
        return out

    def _launch_filtered(self, *args):
        raise ValueError(f"{type(self).__name__} has no filtered search")

    def _padded(self, torch, queries, dtype):
        q = torch.zeros((int(queries.shape[0]), self.dim_pad), dtype=dtype, device=self.device)
        q[:, : self.dim] = queries
        return q

    def _score_docs_device(self, queries, dtype, cand_doc, cand_count, out, *extra):
        """The candidate block checked (as ``DeviceIndex.score_docs_device`` checks it), the query block zero-padded to
        ``dim_pad``, then the class's ``_launch_score(L, q, nq, cand_doc, cand_count, m, out, stream, *extra)`` -> the entry
        point's return code.  Asynchronous on the current stream; an empty batch launches nothing.  Returns f32[nq, m]."""
        torch = _torch()
        nq = int(queries.shape[0])
        L = _capi.lib()
        with torch.cuda.device(self.device):
            cand_doc, cand_count, m, out = _candidate_block(torch, nq, cand_doc, cand_count, out, self.device)
            if nq > 0:
                rc = self._launch_score(L, self._padded(torch, queries, dtype), nq, cand_doc, cand_count, m, out,
                                        _stream_ptr(torch, self.device), *extra)
                _capi.check(rc, self._score_entry)
        return out

    def _score_docs(self, cand_doc, cand_count, nq: int, score_fn) -> np.ndarray:
        """Host candidates (:func:`validate_candidates`) through ``score_fn(cand_doc, cand_count)`` on device tensors: one
        launch, one synchronisation, one copy.  Returns f32[nq, m]."""
        torch = _torch()
        cand_doc, cand_count = validate_candidates(cand_doc, cand_count, nq)
        cd = torch.as_tensor(cand_doc, device=self.device)
        cc = None if cand_count is None else torch.as_tensor(cand_count, device=self.device)
        return self._host((score_fn(cd, cc),))[0]

    def _host(self, out):
        return _to_host(_torch(), self.device, out)


class DenseInt8Index(_DenseIndex):
    """INT8 corpus resident in HBM: ``corpus_int8`` i8[n_docs, dim] (rows zero-padded to a supported length) and
    ``corpus_scales`` f32[n_docs] -- the state ``QuantizedEmbeddingRetriever.build_index_from_corpus`` keeps
    (retriever_registry.py:389-392).  By default the matrix is kept in MFMA-fragment order only (``srx_dense_pack_i8``:
    same bytes; a wave's B-fragment loads are contiguous); ``packed=False`` keeps the row-major matrix and searches that."""

    _workspace_fn, _entry, _score_entry = "srx_dense_workspace_bytes", "srx_dense_search_i8", "srx_dense_score_docs_i8"

    def __init__(self, corpus_int8, corpus_scales, device="cuda:0", doc_base: int = 0, packed: bool = True):
        torch = self._open(device)
        c = corpus_int8 if isinstance(corpus_int8, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(corpus_int8, dtype=np.int8))
        assert c.dtype == torch.int8 and c.dim() == 2
        self.n_docs, self.dim = int(c.shape[0]), int(c.shape[1])
        self.dim_pad = _pad_dim(self.dim)
        with torch.cuda.device(self.device):
            rows = torch.zeros((self.n_docs, self.dim_pad), dtype=torch.int8, device=self.device)
            rows[:, : self.dim] = c.to(self.device)
            self.packed = bool(packed)
            if self.packed:
                L = _capi.lib()
                nbytes = _capi.check(L.srx_dense_packed_bytes(self.n_docs, self.dim_pad), "srx_dense_packed_bytes")
                self.corpus = torch.empty(nbytes, dtype=torch.int8, device=self.device)
                _capi.check(L.srx_dense_pack_i8(self.device.index or 0, _ptr(rows), self.n_docs, self.dim_pad, _ptr(self.corpus),
                                                _stream_ptr(torch, self.device)), "srx_dense_pack_i8")
                torch.cuda.synchronize(self.device)
                del rows
            else:
                self.corpus = rows
            s = corpus_scales if isinstance(corpus_scales, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(corpus_scales, dtype=np.float32))
            self.scales = s.to(device=self.device, dtype=torch.float32).contiguous()
        assert self.scales.numel() == self.n_docs
        self.doc_base = int(doc_base)

    @classmethod
    def from_embeddings(cls, emb, device="cuda:0", doc_base: int = 0, packed: bool = True, chunk_rows=None):
        """The index of f32[n_docs, dim] embeddings quantised ON THE DEVICE (``srx_dense_quantize_i8``): the corpus and scale
        tensors are bit for bit those of ``DenseInt8Index(*quantize_symmetric(emb))``; with ``packed`` the kernel writes the
        fragment order directly (no row-major intermediate).  ``emb``: a float32 device tensor (one launch) or host array
        (uploaded ``chunk_rows`` rows at a time, a multiple of 32; default: 64 MB of rows).  ``ValueError`` for a non-finite
        value, raised after the one synchronisation the build needs."""
        _require_f32(emb, "embeddings")
        self = cls.__new__(cls)
        torch = self._open(device)
        self.n_docs, self.dim = int(emb.shape[0]), int(emb.shape[1])
        if self.n_docs == 0:
            raise ValueError("Empty corpus provided")
        self.dim_pad = _pad_dim(self.dim)
        self.packed, self.doc_base = bool(packed), int(doc_base)
        with torch.cuda.device(self.device):
            if self.packed:
                nbytes = _capi.check(_capi.lib().srx_dense_packed_bytes(self.n_docs, self.dim_pad), "srx_dense_packed_bytes")
                self.corpus = torch.empty(nbytes, dtype=torch.int8, device=self.device)
            else:
                self.corpus = torch.empty((self.n_docs, self.dim_pad), dtype=torch.int8, device=self.device)
            self.scales = torch.empty((self.n_docs,), dtype=torch.float32, device=self.device)
            _quantize_corpus(self, torch, emb, chunk_rows, "srx_dense_quantize_i8", (self.corpus, self.scales), int(self.packed))
        return self

    def corpus_to_host(self):
        """(i8[n_docs, dim], f32[n_docs]) host copies of the resident corpus: what ``quantize_symmetric`` returned for it."""
        torch = _torch()
        torch.cuda.synchronize(self.device)
        c = self.corpus.cpu().numpy()
        rows = unpack_i8_host(c, self.n_docs, self.dim_pad) if self.packed else c
        return np.ascontiguousarray(rows[:, : self.dim]), self.scales.cpu().numpy()

    def search_f32_device(self, queries_f32, k: int):
        """f32[nq, dim] query vectors on the device: quantised there (:func:`quantize_queries_symmetric_device`), then
        :meth:`search_device`.  Asynchronous; a non-finite or all-zero query returns an empty row."""
        q, qs, _ = quantize_queries_symmetric_device(queries_f32.to(self.device))
        return self.search_device(q, qs, k)

    def score_docs_f32_device(self, queries_f32, cand_doc, cand_count=None, out=None):
        """:meth:`score_docs_device` for f32[nq, dim] query vectors on the device, quantised there."""
        q, qs, _ = quantize_queries_symmetric_device(queries_f32.to(self.device))
        return self.score_docs_device(q, qs, cand_doc, cand_count, out)

    def search_device(self, queries_int8, query_scales, k: int, filter=None, q_filter=None):
        """queries i8[nq, dim] + f32[nq] on the device -> (doc i32[nq,k], score f32[nq,k], count i32[nq]); asynchronous.
        A ``filter`` raises ValueError: the fused screen of this search takes its thresholds from a sample of ALL docs, so a
        doc filter is not a test that can be added to it (filter the f32 or the uint8 index)."""
        if filter is not None or q_filter is not None:
            raise ValueError("the INT8 dense search takes no doc filter (its screen thresholds come from a sample of all docs): "
                             "use DenseF32Index or DenseUint8Index")
        return self._search_device(queries_int8, _torch().int8, k, query_scales)

    def _launch(self, L, q, nq, k, out, ws, stream, query_scales):
        qs = query_scales.to(device=self.device, dtype=_torch().float32).contiguous()
        fn = L.srx_dense_search_i8_packed if self.packed else L.srx_dense_search_i8
        return fn(self.device.index or 0, _ptr(self.corpus), _ptr(self.scales), self.n_docs, self.dim_pad, _ptr(q), _ptr(qs), nq, k,
                  self.doc_base, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(ws), ws.numel(), stream)

    def search(self, queries_int8: np.ndarray, query_scales: np.ndarray, k: int):
        """Host arrays in, host arrays out."""
        return self._host(self.search_device(*self._queries_to_device(queries_int8, query_scales), k))

    def _queries_to_device(self, queries_int8, query_scales):
        torch = _torch()
        return (torch.as_tensor(np.ascontiguousarray(queries_int8, dtype=np.int8), device=self.device),
                torch.as_tensor(np.ascontiguousarray(query_scales, dtype=np.float32), device=self.device))

    def score_docs_device(self, queries_int8, query_scales, cand_doc, cand_count=None, out=None):
        """``srx_dense_score_docs_i8`` (include/sparse_rx_rescore.h): the score of every (query, candidate) pair with the
        arithmetic of :meth:`search_device` -- a row it returned scores to its own bits.  cand_doc i32[nq, m] GLOBAL ids,
        cand_count i32[nq] or None: the triple of any search can be passed as it is.  Returns f32[nq, m] (``out`` when
        given): ``+0`` for padding and ids outside the index, no ``score > 0`` filter.  Asynchronous on the current stream."""
        return self._score_docs_device(queries_int8, _torch().int8, cand_doc, cand_count, out, query_scales)

    def _launch_score(self, L, q, nq, cand_doc, cand_count, m, out, stream, query_scales):
        qs = query_scales.to(device=self.device, dtype=_torch().float32).contiguous()
        return L.srx_dense_score_docs_i8(self.device.index or 0, _ptr(self.corpus), int(self.packed), _ptr(self.scales), self.n_docs,
                                         self.dim_pad, _ptr(q), _ptr(qs), nq, self.doc_base, _ptr(cand_doc), _ptr(cand_count), m,
                                         _ptr(out), stream)

    def score_docs(self, queries_int8: np.ndarray, query_scales: np.ndarray, cand_doc, cand_count=None) -> np.ndarray:
        """Host arrays in (the candidates validated by :func:`validate_candidates`), f32[nq, m] out."""
        q, qs = self._queries_to_device(queries_int8, query_scales)
        return self._score_docs(cand_doc, cand_count, int(q.shape[0]), lambda cd, cc: self.score_docs_device(q, qs, cd, cc))


class DenseUint8Index(_DenseIndex):
    """Asymmetric-scheme corpus resident in HBM: ``corpus_uint8`` u8[n_docs, dim] and the reference's ``corpus_scales``
    table f32[2 n_docs] unchanged (retriever_registry.py:449-462); ``search`` replaces the de-quantize + ``np.dot`` loop of
    ``_numpy_quantized_similarity`` (:550-559) + the top-k for a batch of de-quantized query vectors
    (``srx_dense_search_u8``, which indexes the table the way the reference's reader does)."""

    _entry, _score_entry = "srx_dense_search_u8", "srx_dense_score_docs_u8"

    def __init__(self, corpus_uint8, corpus_scales, device="cuda:0", doc_base: int = 0):
        torch = self._open(device)
        c = torch.as_tensor(np.ascontiguousarray(corpus_uint8, dtype=np.uint8))
        assert c.dim() == 2
        self.n_docs, self.dim = int(c.shape[0]), int(c.shape[1])
        self.dim_pad = self._pad64("uint8")
        s = np.ascontiguousarray(corpus_scales, dtype=np.float32).reshape(-1)
        if s.size != 2 * self.n_docs:
            raise ValueError("corpus_scales must hold 2 * n_docs floats (retriever_registry.py:459)")
        with torch.cuda.device(self.device):
            self.corpus = torch.zeros((self.n_docs, self.dim_pad), dtype=torch.uint8, device=self.device)
            self.corpus[:, : self.dim] = c.to(self.device)
            self.scales = torch.as_tensor(s).to(self.device)
        self.doc_base = int(doc_base)

    @classmethod
    def from_embeddings(cls, emb, device="cuda:0", doc_base: int = 0, chunk_rows=None):
        """As ``DenseInt8Index.from_embeddings`` for the asymmetric scheme (``srx_dense_quantize_u8``): the tensors of
        ``DenseUint8Index(*quantize_asymmetric(emb))``."""
        _require_f32(emb, "embeddings")
        self = cls.__new__(cls)
        torch = self._open(device)
        self.n_docs, self.dim = int(emb.shape[0]), int(emb.shape[1])
        if self.n_docs == 0:
            raise ValueError("Empty corpus provided")
        self.dim_pad = self._pad64("uint8")
        self.doc_base = int(doc_base)
        with torch.cuda.device(self.device):
            self.corpus = torch.empty((self.n_docs, self.dim_pad), dtype=torch.uint8, device=self.device)
            self.scales = torch.empty((2 * self.n_docs,), dtype=torch.float32, device=self.device)
            _quantize_corpus(self, torch, emb, chunk_rows, "srx_dense_quantize_u8", (self.corpus, self.scales))
        return self

    def corpus_to_host(self):
        """(u8[n_docs, dim], f32[2 n_docs]) host copies of the resident corpus: what ``quantize_asymmetric`` returned for it."""
        _torch().cuda.synchronize(self.device)
        return np.ascontiguousarray(self.corpus.cpu().numpy()[:, : self.dim]), self.scales.cpu().numpy()

    def search_raw_device(self, queries_f32, k: int):
        """RAW f32[nq, dim] query vectors on the device: quantised and de-quantised there as the reference's search does
        (``srx_dense_quantize_queries_u8``'s out_deq), then :meth:`search_device`.  Asynchronous."""
        return self.search_device(quantize_queries_asymmetric_device(queries_f32.to(self.device), codes=False)[2], k)

    def score_docs_raw_device(self, queries_f32, cand_doc, cand_count=None, out=None):
        """:meth:`score_docs_device` for RAW query vectors, as :meth:`search_raw_device`."""
        return self.score_docs_device(quantize_queries_asymmetric_device(queries_f32.to(self.device), codes=False)[2], cand_doc, cand_count, out)

    def search_device(self, queries_f32, k: int, filter=None, q_filter=None):
        """De-quantized queries f32[nq, dim] on the device; ``filter`` / ``q_filter`` as ``DeviceIndex.search_device``
        (``srx_dense_search_u8_filtered``)."""
        return self._search_device(queries_f32, _torch().float32, k, filter=filter, q_filter=q_filter)

    def _launch_filtered(self, L, q, nq, k, out, ws, stream, fdesc):
        return L.srx_dense_search_u8_filtered(self.device.index or 0, _ptr(self.corpus), _ptr(self.scales), self.n_docs, self.dim_pad,
                                              _ptr(q), nq, k, self.doc_base, fdesc, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(ws),
                                              ws.numel(), stream)

    def _launch(self, L, q, nq, k, out, ws, stream):
        return L.srx_dense_search_u8(self.device.index or 0, _ptr(self.corpus), _ptr(self.scales), self.n_docs, self.dim_pad, _ptr(q),
                                     nq, k, self.doc_base, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(ws), ws.numel(), stream)

    def search(self, queries_uint8: np.ndarray, query_scales: np.ndarray, k: int, filter=None, q_filter=None):
        """queries u8[nq, dim] + f32[nq, 2] (scale, min) as the reference's search builds them (:486-491); host arrays out.
        ``q_filter``: a host sequence of row numbers, validated here."""
        q = self._queries_to_device(queries_uint8, query_scales)
        return self._host(self.search_device(q, k, filter=filter, q_filter=host_q_filter(self, filter, q_filter, int(q.shape[0]))))

    def _queries_to_device(self, queries_uint8, query_scales):
        """The de-quantized f32 query block on the device"""
        qf = np.stack([dequantize_query_asymmetric(q, s) for q, s in zip(np.asarray(queries_uint8), np.asarray(query_scales))])
        return _torch().as_tensor(np.ascontiguousarray(qf, dtype=np.float32), device=self.device)

    def score_docs_device(self, queries_f32, cand_doc, cand_count=None, out=None):
        """``srx_dense_score_docs_u8`` for de-quantized queries f32[nq, dim]: as ``DenseInt8Index.score_docs_device``."""
        return self._score_docs_device(queries_f32, _torch().float32, cand_doc, cand_count, out)

    def _launch_score(self, L, q, nq, cand_doc, cand_count, m, out, stream):
        return L.srx_dense_score_docs_u8(self.device.index or 0, _ptr(self.corpus), _ptr(self.scales), self.n_docs, self.dim_pad, _ptr(q),
                                         nq, self.doc_base, _ptr(cand_doc), _ptr(cand_count), m, _ptr(out), stream)

    def score_docs(self, queries_uint8: np.ndarray, query_scales: np.ndarray, cand_doc, cand_count=None) -> np.ndarray:
        """queries as in :meth:`search`, host candidates (:func:`validate_candidates`); f32[nq, m] out."""
        q = self._queries_to_device(queries_uint8, query_scales)
        return self._score_docs(cand_doc, cand_count, int(q.shape[0]), lambda cd, cc: self.score_docs_device(q, cd, cc))


def stack_queries_f32(index, embs):
    """Query vectors for the device quantisers as ONE f32[nq, dim] tensor on ``index.device``: a list of host rows is stacked
    once and uploaded once, a 2-D host array is uploaded, a device tensor is taken as it is.  float32 only (``ValueError``
    otherwise: the host quantisers compute in the dtype they are given)."""
    torch = _torch()
    if isinstance(embs, torch.Tensor):
        _require_f32(embs, "query embeddings")
        return embs.to(index.device)
    q = np.stack([np.asarray(e) for e in embs]) if isinstance(embs, (list, tuple)) else np.asarray(embs)
    _require_f32(q, "query embeddings")
    return torch.as_tensor(np.ascontiguousarray(q), device=index.device)


class QuantizedEmbeddingIndex:
    """The search half of the reference's ``QuantizedEmbeddingRetriever`` (symmetric INT8) over given embeddings:
    ``build(doc_ids, embeddings)`` quantizes like :435-447, ``search(query_embeddings, top_k)`` quantizes each query like
    :482-485 and returns ``{doc_id: score}`` ranked, ``score > 0`` only (:515-519), for every query at once."""

    def __init__(self, device="cuda:0", quantize: str = "host"):
        self.device = device
        self.quantize = check_quantize_arg(quantize)  # "device": build and search quantise in HIP (float32 embeddings only)
        self.doc_ids: List[str] = []
        self.index = None

    def build(self, doc_ids: Sequence[str], embeddings) -> None:
        if len(doc_ids) == 0:
            raise ValueError("Empty corpus provided")
        if self.quantize == "device":
            self.index = DenseInt8Index.from_embeddings(embeddings, device=self.device)
        else:
            q, scales = quantize_symmetric(embeddings)
            self.index = DenseInt8Index(q, scales, device=self.device)
        self.doc_ids = list(doc_ids)

    def search(self, query_embeddings: Dict[str, np.ndarray], top_k: int = 10) -> Dict[str, Dict[str, float]]:
        if self.index is None:
            raise ValueError("Index not built. Call build_index_from_corpus() first.")
        qids = list(query_embeddings)
        if not qids:
            return {}
        k = min(top_k, len(self.doc_ids))
        if self.quantize == "device":
            d, s, n = self.index._host(self.index.search_f32_device(stack_queries_f32(self.index, [query_embeddings[q] for q in qids]), k))
        else:
            qq = [quantize_query_symmetric(query_embeddings[q]) for q in qids]
            d, s, n = self.index.search(np.stack([a for a, _ in qq]), np.array([b for _, b in qq], dtype=np.float32), k)
        return {qid: rows_to_dict(self.doc_ids, d, s, n, i) for i, qid in enumerate(qids)}


MMR_SIMILARITIES = {"dot": _capi.SRX_MMR_DOT, "cosine": _capi.SRX_MMR_COSINE}
MMR_CALL_BYTES = 256 << 20  # the Gram matrices of one ``srx_mmr_select_*`` call: a larger batch is split


def check_mmr_args(lambda_, similarity) -> Tuple[int, float, float]:
    """The argument rules of the MMR selection on the host: (sim_mode, w_rel, w_div) or ``ValueError``.  ``w_rel =
    float32(lambda_)`` and ``w_div = float32(1.0 - lambda_)``, the difference computed in double."""
    sim = str(similarity).lower()
    if sim not in MMR_SIMILARITIES:
        raise ValueError(f"similarity must be one of {sorted(MMR_SIMILARITIES)}, got {similarity!r}")
    try:
        lam = float(lambda_)
    except (TypeError, ValueError):
        raise ValueError(f"mmr lambda must be a number in [0, 1], got {lambda_!r}") from None
    if not (0.0 <= lam <= 1.0):  # false for a NaN
        raise ValueError(f"mmr lambda must be in [0, 1], got {lambda_!r}")
    return MMR_SIMILARITIES[sim], float(np.float32(lam)), float(np.float32(1.0 - lam))


def check_mmr_shape(m: int, k) -> int:
    """``k`` as an int for a list of ``m`` candidates, or ``ValueError``: 1 <= m <= 256 (no silent truncation), 1 <= k <= m."""
    if not (1 <= m <= _capi.SRX_MMR_MAX_M):
        raise ValueError(f"an MMR pool holds 1 .. {_capi.SRX_MMR_MAX_M} candidates per query, got m={m}")
    k = int(k)
    if not (1 <= k <= m):
        raise ValueError(f"k must be in [1, m={m}] for the MMR selection, got {k}")
    return k


class _MmrSelect:
    """Diversified top-k over candidate lists (include/sparse_rx_mmr.h) for the indexes that keep rows a similarity can be
    read from: :class:`DenseF32Index` and :class:`DenseHalfIndex`.  The uint8 / INT8 indexes have no such method."""

    def mmr_device(self, cand_doc, cand_rel, cand_count, k: int, lambda_: float = 0.5, similarity: str = "cosine", return_sim: bool = False):
        """Maximal Marginal Relevance on the device: ``k`` of the ``m`` candidates of every query, picked greedily, each pick
        maximising ``lambda_ * relevance - (1 - lambda_) * (largest similarity to a doc already picked)``; ties go to the
        lowest position.  ``cand_doc`` i32[nq, m] GLOBAL ids, ``cand_rel`` f32[nq, m], ``cand_count`` i32[nq] or None: the
        (doc, score, count) triple of any search or of the fusion as it is (m <= 256).  A position at or past the count,
        an id outside the index or a NaN relevance is not a candidate.  ``similarity`` "dot" or "cosine" of this index's
        rows (the rounded rows of a half index), to the bit the scores ``score_docs_device`` returns for a query that equals
        a row.  Returns device tensors ``(doc i32[nq, k], rel f32[nq, k], mmr f32[nq, k], count i32[nq])`` -- the docs in
        SELECTION order with their relevance as given and the value they were picked with, rows padded with -1 / 0 -- plus
        ``sim`` f32[nq, m, m] (the dot products, 0 for a dead row or column) with ``return_sim``.  Asynchronous on the
        current stream; a batch whose Gram matrices exceed 256 MiB is split into several calls."""
        torch = _torch()
        sim_mode, w_rel, w_div = check_mmr_args(lambda_, similarity)
        if cand_doc.dim() != 2 or cand_doc.dtype != torch.int32:
            raise ValueError("mmr_device: cand_doc must be an int32 tensor [nq, m]")
        nq, m = int(cand_doc.shape[0]), int(cand_doc.shape[1])
        k = check_mmr_shape(m, k)
        if cand_rel.dtype != torch.float32 or tuple(cand_rel.shape) != (nq, m):
            raise ValueError("mmr_device: cand_rel must be a float32 tensor of cand_doc's shape")
        if cand_count is not None and (cand_count.dtype != torch.int32 or cand_count.numel() != nq):
            raise ValueError("mmr_device: cand_count must be an int32 tensor [nq]")
        L = _capi.lib()
        with torch.cuda.device(self.device):
            cand_doc, cand_rel = cand_doc.contiguous(), cand_rel.contiguous()
            cand_count = None if cand_count is None else cand_count.contiguous()
            doc, rel, count = _empty_topk(torch, nq, k, self.device)
            mmr = torch.empty((nq, k), dtype=torch.float32, device=self.device)
            sim = torch.empty((nq, m, m), dtype=torch.float32, device=self.device) if return_sim else None
            per_call = max(1, MMR_CALL_BYTES // (m * m * 4))
            stream = _stream_ptr(torch, self.device)
            for lo in range(0, nq, per_call):
                n = min(per_call, nq - lo)
                if return_sim:
                    ws = sim[lo: lo + n]  # out_sim IS the Gram buffer: it serves as the workspace
                else:
                    ws = _grow_ws(torch, self, _capi.check(L.srx_mmr_workspace_bytes(n, m), "srx_mmr_workspace_bytes"))
                rc = self._launch_mmr(L, _ptr(cand_doc[lo: lo + n]), _ptr(cand_rel[lo: lo + n]), 0 if cand_count is None else _ptr(cand_count[lo: lo + n]),
                                      n, m, k, sim_mode, w_rel, w_div, _ptr(doc[lo: lo + n]), _ptr(rel[lo: lo + n]), _ptr(mmr[lo: lo + n]),
                                      _ptr(count[lo: lo + n]), 0 if sim is None else _ptr(ws), _ptr(ws), ws.numel() * ws.element_size(), stream)
                _capi.check(rc, self._mmr_entry)
        return (doc, rel, mmr, count, sim) if return_sim else (doc, rel, mmr, count)

    def mmr(self, cand_doc, cand_rel, cand_count, k: int, lambda_: float = 0.5, similarity: str = "cosine", return_sim: bool = False):
        """Host arrays in (the candidates validated by :func:`validate_candidates`), host arrays out: :meth:`mmr_device`
        with one synchronisation and one copy back."""
        torch = _torch()
        check_mmr_args(lambda_, similarity)
        d = np.asarray(cand_doc)
        cand_doc, cand_count = validate_candidates(d, cand_count, int(d.shape[0]) if d.ndim == 2 else 0)
        check_mmr_shape(int(cand_doc.shape[1]), k)
        r = np.ascontiguousarray(cand_rel, dtype=np.float32)
        if r.shape != cand_doc.shape:
            raise ValueError("cand_rel must have cand_doc's shape")
        cc = None if cand_count is None else torch.as_tensor(cand_count, device=self.device)
        return self._host(self.mmr_device(torch.as_tensor(cand_doc, device=self.device), torch.as_tensor(r, device=self.device), cc, k, lambda_,
                                          similarity, return_sim))


class DenseF32Index(_DenseIndex, _MmrSelect):
    """f32 embedding matrix resident in HBM: the ``embedding_index`` of ``RetrievalService`` (retrieval.py:329-335);
    ``search`` replaces ``np.dot(self.embedding_index, query_vector)`` + top-k of ``search_by_vector`` (:411-423) for a
    batch of query vectors (``srx_dense_search_f32``)."""

    _entry, _score_entry, _mmr_entry = "srx_dense_search_f32", "srx_dense_score_docs_f32", "srx_mmr_select_f32"

    def _launch_mmr(self, L, *tail):
        return L.srx_mmr_select_f32(self.device.index or 0, _ptr(self.emb), self.n_docs, self.dim_pad, self.doc_base, *tail)

    def __init__(self, embeddings, device="cuda:0", doc_base: int = 0):
        torch = self._open(device)
        e = embeddings
        assert len(e.shape) == 2 and (not isinstance(e, torch.Tensor) or e.dtype == torch.float32)
        self.n_docs, self.dim = int(e.shape[0]), int(e.shape[1])
        self.dim_pad = self._pad64("f32")
        with torch.cuda.device(self.device):
            self.emb = torch.zeros((self.n_docs, self.dim_pad), dtype=torch.float32, device=self.device)
            if isinstance(e, torch.Tensor):
                self.emb[:, : self.dim] = e.to(self.device)
            else:
                # host array, possibly a read-only memory map of embedding_path (retrieval.py:329-335): streamed to the device
                # in chunks of <= 64 MB (np.array copies a chunk: a whole-file host copy is never made, and the map itself is
                # never wrapped in a tensor)
                rows = max(1, (64 << 20) // max(1, 4 * self.dim))
                for lo in range(0, self.n_docs, rows):
                    chunk = np.array(e[lo: lo + rows], dtype=np.float32)
                    self.emb[lo: lo + chunk.shape[0], : self.dim] = torch.from_numpy(chunk).to(self.device)
        self.doc_base = int(doc_base)
        self._max_norm = None

    def max_row_norm(self) -> float:
        """Largest Euclidean row norm (fp64 accumulation), computed once on the device from the resident matrix in row
        chunks of <= 64 MB -- never a host-side temporary of the (possibly memory-mapped) matrix."""
        if self._max_norm is None:
            torch = _torch()
            rows = max(1, (64 << 20) // (4 * self.dim_pad))
            best = 0.0
            with torch.cuda.device(self.device):
                for lo in range(0, self.n_docs, rows):
                    c = self.emb[lo: lo + rows].double()
                    best = max(best, float((c * c).sum(dim=1).max().item()))
            self._max_norm = best ** 0.5
        return self._max_norm

    def search_device(self, queries, k: int, score_offset: float = 0.0, filter=None, q_filter=None):
        """Top-k of (score + score_offset) > 0 per query (include/sparse_rx.h); the returned scores carry the offset.
        ``filter`` / ``q_filter`` as ``DeviceIndex.search_device`` (``srx_dense_search_f32_filtered``)."""
        return self._search_device(queries, _torch().float32, k, score_offset, filter=filter, q_filter=q_filter)

    def _launch_filtered(self, L, q, nq, k, out, ws, stream, fdesc, score_offset):
        return L.srx_dense_search_f32_filtered(self.device.index or 0, _ptr(self.emb), self.n_docs, self.dim_pad, _ptr(q), nq, k,
                                               self.doc_base, fdesc, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(ws), ws.numel(), stream,
                                               float(score_offset))

    def _launch(self, L, q, nq, k, out, ws, stream, score_offset):
        return L.srx_dense_search_f32(self.device.index or 0, _ptr(self.emb), self.n_docs, self.dim_pad, _ptr(q), nq, k, self.doc_base,
                                      _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(ws), ws.numel(), stream, float(score_offset))

    def search(self, queries: np.ndarray, k: int, score_offset: float = 0.0, filter=None, q_filter=None):
        q = self._queries_to_device(queries)
        return self._host(self.search_device(q, k, score_offset, filter=filter, q_filter=host_q_filter(self, filter, q_filter, int(q.shape[0]))))

    def _queries_to_device(self, queries):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        return _torch().as_tensor(q, device=self.device)

    def score_docs_device(self, queries, cand_doc, cand_count=None, out=None):
        """``srx_dense_score_docs_f32``: as ``DenseInt8Index.score_docs_device``; the bits are those of :meth:`search_device`
        with ``score_offset = 0``."""
        return self._score_docs_device(queries, _torch().float32, cand_doc, cand_count, out)

    def _launch_score(self, L, q, nq, cand_doc, cand_count, m, out, stream):
        return L.srx_dense_score_docs_f32(self.device.index or 0, _ptr(self.emb), self.n_docs, self.dim_pad, _ptr(q), nq, self.doc_base,
                                          _ptr(cand_doc), _ptr(cand_count), m, _ptr(out), stream)

    def score_docs(self, queries: np.ndarray, cand_doc, cand_count=None) -> np.ndarray:
        """Host arrays in (the candidates validated by :func:`validate_candidates`), f32[nq, m] out."""
        q = self._queries_to_device(queries)
        return self._score_docs(cand_doc, cand_count, int(q.shape[0]), lambda cd, cc: self.score_docs_device(q, cd, cc))


HALF_TYPES = {"f16": _capi.SRX_HALF_F16, "bf16": _capi.SRX_HALF_BF16}


def check_half_dtype(dtype) -> str:
    d = str(dtype).lower()
    if d not in HALF_TYPES:
        raise ValueError(f"dtype must be 'f16' or 'bf16', got {dtype!r}")
    return d


class DenseHalfIndex(_DenseIndex, _MmrSelect):
    """Half-precision embedding matrix resident in HBM (include/sparse_rx_half.h): the rows rounded to f16 or bf16 (nearest
    even) and kept ONLY in the MFMA-fragment order the search reads.  A whole query batch is one GEMM
    (``srx_dense_search_half``); filters, ``score_offset`` and the scorer of given docs are those of :class:`DenseF32Index`.
    Scores are the dot products of the ROUNDED rows and the rounded queries, accumulated in fp32 by the MFMA instruction."""

    _workspace_fn, _entry, _score_entry = "srx_dense_half_workspace_bytes", "srx_dense_search_half", "srx_dense_score_docs_half"
    _filtered_entry = "srx_dense_search_half"  # one entry point, the filter optional
    _mmr_entry = "srx_mmr_select_half"

    def _launch_mmr(self, L, *tail):
        return L.srx_mmr_select_half(self.device.index or 0, HALF_TYPES[self.dtype], _ptr(self.corpus), self.n_docs, self.dim_pad, self.doc_base, *tail)

    def __init__(self, embeddings, dtype="f16", device="cuda:0", doc_base: int = 0, chunk_rows=None):
        """``embeddings``: f32[n_docs, dim], a device tensor (one launch) or a host array, possibly a read-only memory map
        (uploaded ``chunk_rows`` rows at a time through one staging tensor, a multiple of 32; default: 64 MB of rows).
        ``ValueError`` for a row with a non-finite value or one that does not round to a finite value (|x| >= 65520 for
        f16), raised after the one synchronisation the build needs."""
        self.dtype = check_half_dtype(dtype)
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
            nbytes = _capi.check(L.srx_dense_half_bytes(self.n_docs, self.dim_pad), "srx_dense_half_bytes")
            self.corpus = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _quantize_corpus(self, torch, embeddings, chunk_rows, None, (), convert=lambda x, row0, flag: self._convert(torch, L, x, row0, flag),
                             refusal=f"embeddings hold a value that is not finite as {self.dtype} (NaN / inf, or too large for the type)")

    def _convert(self, torch, L, x, row0: int, flag) -> None:
        x, ld = _f32_rows(torch, x, "embeddings")
        _capi.check(L.srx_dense_convert_half(self.device.index or 0, HALF_TYPES[self.dtype], _ptr(x), ld, int(x.shape[0]), self.dim, self.dim_pad,
                                             row0, self.n_docs, _ptr(self.corpus), _ptr(flag), _stream_ptr(torch, self.device)),
                    "srx_dense_convert_half")

    @classmethod
    def from_embeddings(cls, emb, dtype="f16", device="cuda:0", doc_base: int = 0, chunk_rows=None):
        """The constructor under the name the quantised indexes give theirs."""
        return cls(emb, dtype=dtype, device=device, doc_base=doc_base, chunk_rows=chunk_rows)

    def device_bytes(self) -> int:
        """Bytes of the resident corpus (``srx_dense_half_bytes``)."""
        return int(self.corpus.numel())

    def corpus_to_host(self) -> np.ndarray:
        """u16[n_docs, dim]: the 16-bit codes of the rounded rows, row-major (f16: ``.view(np.float16)``; bf16: the upper
        halves of the float32 bit patterns)."""
        _torch().cuda.synchronize(self.device)
        return np.ascontiguousarray(unpack_half_host(self.corpus.cpu().numpy(), self.n_docs, self.dim_pad)[:, : self.dim])

    def max_row_norm(self) -> float:
        """Largest Euclidean norm of the ROUNDED rows (fp64 accumulation), computed once from a host copy in row chunks."""
        if self._max_norm is None:
            c = self.corpus_to_host()
            rows = max(1, (64 << 20) // (8 * self.dim))
            best = 0.0
            for lo in range(0, self.n_docs, rows):
                x = c[lo: lo + rows]
                x = (x.view(np.float16) if self.dtype == "f16" else (x.astype(np.uint32) << 16).view(np.float32)).astype(np.float64)
                best = max(best, float((x * x).sum(axis=1).max()))
            self._max_norm = best ** 0.5
        return self._max_norm

    def search_device(self, queries_f32, k: int, score_offset: float = 0.0, filter=None, q_filter=None):
        """f32[nq, dim] queries on the device (rounded to the index's type by the search) -> (doc i32[nq,k], score f32[nq,k],
        count i32[nq]); asynchronous.  Top-k of (score + score_offset) > 0, the returned scores carry the offset; ``filter`` /
        ``q_filter`` as ``DeviceIndex.search_device``."""
        return self._search_device(queries_f32, _torch().float32, k, score_offset, filter=filter, q_filter=q_filter)

    def _launch_filtered(self, L, q, nq, k, out, ws, stream, fdesc, score_offset):
        return L.srx_dense_search_half(self.device.index or 0, HALF_TYPES[self.dtype], _ptr(self.corpus), self.n_docs, self.dim_pad, _ptr(q), nq, k,
                                       self.doc_base, fdesc, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(ws), ws.numel(), stream,
                                       float(score_offset))

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
        """``srx_dense_score_docs_half``: as ``DenseF32Index.score_docs_device``; the bits are those of :meth:`search_device`
        with ``score_offset = 0``."""
        return self._score_docs_device(queries_f32, _torch().float32, cand_doc, cand_count, out)

    def _launch_score(self, L, q, nq, cand_doc, cand_count, m, out, stream):
        return L.srx_dense_score_docs_half(self.device.index or 0, HALF_TYPES[self.dtype], _ptr(self.corpus), self.n_docs, self.dim_pad, _ptr(q),
                                           nq, self.doc_base, _ptr(cand_doc), _ptr(cand_count), m, _ptr(out), stream)

    def score_docs(self, queries: np.ndarray, cand_doc, cand_count=None) -> np.ndarray:
        """Host arrays in (the candidates validated by :func:`validate_candidates`), f32[nq, m] out."""
        q = self._queries_to_device(queries)
        return self._score_docs(cand_doc, cand_count, int(q.shape[0]), lambda cd, cc: self.score_docs_device(q, cd, cc))
