"""Hybrid retrieval, the parts that need no GPU: the C-ABI entry point's declaration and argument checks, the registry
and service doors (errors only: there is no CPU path behind them) and the fixed points of the NumPy restatement the
GPU tests compare against (tests/hybrid_ref.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import hybrid_ref
import sparse_rx
from sparse_rx import _capi

# the reference's own experiment block (rag_system/configs/ms_marco_paper_results.yaml:108-120, `msmarco_hybrid_sparse`)
REFERENCE_HYBRID_BLOCK = {
    "type": "hybrid",
    "model": {"sparse": "bm25_custom", "dense": "sentence-transformers/msmarco-distilbert-base-tas-b"},
    "params": {"top_k": 100, "sparse_weight": 0.3, "dense_weight": 0.7, "use_numba": True, "cache_matrices": True},
}


def _fuse(L, *, a=(1 << 20, 1 << 21, 1 << 22), ka=10, b=(1 << 23, 1 << 24, 1 << 25), kb=10, nq=1, k=10, mode=0, wa=0.3, wb=0.7,
          rrf_c=60.0, out=(1 << 26, 1 << 27, 1 << 28)):
    """srx_fuse_topk with made-up non-null addresses: every call here must be refused before anything touches a device."""
    return L.srx_fuse_topk(0, a[0], a[1], a[2], ka, b[0], b[1], b[2], kb, nq, k, mode, wa, wb, rrf_c, out[0], out[1], out[2], None)


def test_fuse_entry_point_declared_exported_typed():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sparse_rx.h")).read()
    assert "srx_fuse_topk" in set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr))
    assert re.search(r"SRX_FUSE_WEIGHTED\s*=\s*0", hdr) and re.search(r"SRX_FUSE_RRF\s*=\s*1", hdr)
    assert (_capi.SRX_FUSE_WEIGHTED, _capi.SRX_FUSE_RRF) == (0, 1)
    res, args = _capi.SYMBOLS["srx_fuse_topk"]
    assert res is ctypes.c_int and len(args) == 19
    assert args[12:15] == [ctypes.c_float] * 3 and args[4] is ctypes.c_int32 and args[8] is ctypes.c_int32
    L = _capi.lib()
    assert L.srx_fuse_topk.argtypes == args
    assert L.srx_version() == 301  # added without a version bump


def test_fuse_refused_arguments():
    L = _capi.lib()

    def refused(**kw):
        assert _fuse(L, **kw) == -1, kw
        msg = L.srx_last_error()
        assert b"srx_fuse_topk" in msg, (kw, msg)
        return msg

    assert b"null" in refused(a=(None, 1 << 21, 1 << 22))
    assert b"null" in refused(b=(1 << 23, 1 << 24, None))
    assert b"null" in refused(out=(1 << 26, None, 1 << 28))
    for kx in (0, -1, 1025):
        refused(ka=kx)
        refused(kb=kx)
        refused(k=kx)
    assert b"mode" in refused(mode=2)
    refused(mode=-1)
    for w in (-0.5, float("nan"), float("inf")):
        assert b"weight" in refused(wa=w)
        assert b"weight" in refused(wb=w)
    assert b"both" in refused(wa=0.0, wb=0.0)
    for c in (0.0, -1.0, float("nan"), float("inf")):
        assert b"rrf_c" in refused(mode=1, rrf_c=c)
    refused(nq=-1)
    # rrf_c is ignored in mode weighted, a single zero weight is legal, and nq == 0 is OK without a launch (null pointers too)
    assert _fuse(L, nq=0, rrf_c=float("nan")) == 0
    assert _fuse(L, nq=0, wa=0.0) == 0 and _fuse(L, nq=0, wb=0.0, mode=1) == 0
    assert _fuse(L, nq=0, a=(None, None, None), b=(None, None, None), out=(None, None, None)) == 0
    assert _fuse(L, nq=0, ka=1024, kb=1024, k=1024) == 0 and _fuse(L, nq=0, ka=1, kb=1, k=1) == 0


def test_python_side_argument_checks():
    from sparse_rx.index import check_fuse_args, hybrid_depths
    assert check_fuse_args("weighted", (0.3, 0.7), 60.0) == (0, 0.3, 0.7, 60.0)
    assert check_fuse_args("rrf", (1, 0), 1.5)[0] == 1
    for bad in (("nope", (0.3, 0.7), 60.0), ("weighted", (-1, 1), 60.0), ("weighted", (0, 0), 60.0), ("weighted", (float("nan"), 1), 60.0),
                ("rrf", (1, 1), 0.0), ("rrf", (1, 1), float("inf")), ("weighted", (1,), 60.0)):
        with pytest.raises(ValueError):
            check_fuse_args(*bad)
    assert hybrid_depths(10, None, 1000) == (10, 10) and hybrid_depths(10, 5000, 1000) == (10, 1000)
    assert hybrid_depths(100, 5000, 1 << 20) == (100, 1024) and hybrid_depths(50, None, 20) == (20, 20)
    assert hybrid_depths(0, None, 100)[0] == 0
    with pytest.raises(ValueError, match="1024"):
        hybrid_depths(1025, None, 1 << 20)
    with pytest.raises(ValueError, match="candidates"):
        hybrid_depths(10, 0, 100)


def test_registry_routes_the_reference_hybrid_block():
    r = sparse_rx.RetrieverRegistry.create(REFERENCE_HYBRID_BLOCK)
    assert isinstance(r, sparse_rx.HybridRetriever)
    assert (r.sparse_weight, r.dense_weight, r.fusion, r.rrf_c, r.candidates) == (0.3, 0.7, "weighted", 60.0, None)
    assert isinstance(r.sparse, sparse_rx.OptimizedBM25Retriever) and isinstance(r.dense, sparse_rx.QuantizedEmbeddingRetriever)
    assert r.sparse.method == "bm25_custom" and r.dense.model_name.endswith("tas-b")
    assert isinstance(sparse_rx.RetrieverRegistry.create({"type": "HYBRID"}), sparse_rx.HybridRetriever)  # case, no model, no params
    d = sparse_rx.RetrieverRegistry.create({"type": "hybrid", "params": {"fusion": "RRF", "rrf_c": 10, "candidates": 500}})
    assert (d.fusion, d.rrf_c, d.candidates, d.sparse_weight, d.dense_weight) == ("rrf", 10.0, 500, 0.3, 0.7)
    assert "hybrid" in sparse_rx.RetrieverRegistry.list_available()["hybrid"]
    for params in ({"fusion": "minmax"}, {"sparse_weight": -1}, {"sparse_weight": 0, "dense_weight": 0}, {"fusion": "rrf", "rrf_c": 0},
                   {"candidates": 0}):
        with pytest.raises(ValueError):
            sparse_rx.RetrieverRegistry.create({"type": "hybrid", "params": params})
    with pytest.raises(ValueError, match="Index not built"):
        r.search({"q": "hello"})
    with pytest.raises(ValueError, match="Empty corpus"):
        r.build_index_from_corpus({})
    with pytest.raises(ValueError, match="one row per document"):
        r.build_index_from_corpus({"d": {"text": "hello world"}}, embeddings=np.zeros((2, 64), np.float32))


def test_hybrid_has_no_cpu_path():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = sparse_rx.RetrieverRegistry.create(REFERENCE_HYBRID_BLOCK)
    with pytest.raises(sparse_rx.SparseRxUnavailable):
        r.build_index_from_corpus({"d": {"text": "hello world"}})
    with pytest.raises(ValueError, match="device tensors"):
        t = torch.zeros((1, 4), dtype=torch.int32)
        sparse_rx.fuse_topk_device((t, t.float(), t[:, 0].contiguous()), (t, t.float(), t[:, 0].contiguous()), 4)


def test_service_search_hybrid_argument_errors():
    svc = sparse_rx.RetrievalService()
    q, v = {"a": "hello"}, {"a": np.ones(64, np.float32)}
    with pytest.raises(ValueError, match="BM25 index not built"):
        svc.search_hybrid(q, v)
    with pytest.raises(ValueError, match="1024"):
        svc.search_hybrid(q, v, top_k=1025)
    with pytest.raises(ValueError, match="fusion"):
        svc.search_hybrid(q, v, fusion="borda")
    with pytest.raises(ValueError, match="weights"):
        svc.search_hybrid(q, v, sparse_weight=0.0, dense_weight=0.0)
    with pytest.raises(ValueError, match="weights"):
        svc.search_hybrid(q, v, dense_weight=float("nan"))
    with pytest.raises(ValueError, match="rrf_c"):
        svc.search_hybrid(q, v, fusion="rrf", rrf_c=-1.0)
    with pytest.raises(ValueError, match="candidates"):
        svc.search_hybrid(q, v, candidates=0)


def test_hybrid_refuses_a_sharded_index(tmp_path):
    """hybrid search needs the whole index on one GPU: the doors say so on a sharded service (a gloo group of one rank with
    sharded=True takes the sharded path), before anything is built or searched."""
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        r = sparse_rx.RetrieverRegistry.create({"type": "hybrid", "params": {"sharded": True}})
        with pytest.raises(ValueError, match="whole index on one GPU"):
            r.build_index_from_corpus({"d": {"text": "hello world"}})
        with pytest.raises(ValueError, match="whole index on one GPU"):
            r.search({"q": "hello"})
        svc = sparse_rx.RetrievalService(sharded=True)
        with pytest.raises(ValueError, match="whole index on one GPU"):
            svc.search_hybrid({"a": "hello"}, {"a": np.ones(64, np.float32)})
    finally:
        dist.destroy_process_group()


# ---- the restatement's own fixed points (these guard the checker, not the product) ----------------------------------
def _row(docs, scores, kx=None):
    kx = kx or len(docs)
    d = np.full(kx, -1, np.int32)
    s = np.zeros(kx, np.float32)
    d[: len(docs)], s[: len(docs)] = docs, scores
    return d, s, len(docs)


def test_restatement_rrf_tie_breaks_by_doc():
    a, b = _row([5, 9], [3.0, 2.0]), _row([9, 5, 7], [0.9, 0.8, 0.7])
    rows = hybrid_ref.fuse_row(*a, *b, 10, hybrid_ref.RRF, 1.0, 1.0, 60.0)
    assert [d for d, _ in rows] == [5, 9, 7]
    assert rows[0][1].view(np.uint32) == rows[1][1].view(np.uint32)  # 1/61 + 1/62 either way round
    assert rows[0][1] == np.float32(np.float32(1) / np.float32(61)) + np.float32(np.float32(1) / np.float32(62))
    assert f"{rows[0][1]:.8f}" == "0.03252247"
    assert rows[2][1] == np.float32(np.float32(1) / np.float32(63))
    assert [d for d, _ in hybrid_ref.fuse_row(*a, *b, 2, hybrid_ref.RRF, 1.0, 1.0, 60.0)] == [5, 9]


def test_restatement_zero_weight_keeps_the_other_lists_set():
    rng = np.random.default_rng(5)
    a, b = hybrid_ref.make_lists(rng, 6, 40, 50, overlap=0.5, garbage=True)
    for mode in ("weighted", "rrf"):
        d, s, n = hybrid_ref.fuse(a, b, 100, mode, (0.0, 1.0))
        for q in range(6):
            assert set(d[q, : n[q]].tolist()) == set(b[0][q, : b[2][q]].tolist()) and n[q] == b[2][q]
        d, s, n = hybrid_ref.fuse(a, b, 100, mode, (2.0, 0.0))
        for q in range(6):
            assert set(d[q, : n[q]].tolist()) == set(a[0][q, : a[2][q]].tolist())
            assert np.all(d[q, n[q]:] == -1) and np.all(s[q, n[q]:] == 0)


def test_restatement_weighted_heads_sum_the_weights():
    a, b = _row([4, 1], [7.25, 3.0]), _row([4, 2], [0.8125, 0.5])
    rows = hybrid_ref.fuse_row(*a, *b, 5, hybrid_ref.WEIGHTED, 0.3, 0.7)
    assert rows[0][0] == 4 and rows[0][1].view(np.uint32) == np.float32(np.float32(0.3) + np.float32(0.7)).view(np.uint32)
    # entries beyond count, negative docs and non-positive scores are not used; an unused head empties a weighted list
    a2 = (np.array([4, 1, 8], np.int32), np.array([7.25, 3.0, 9.0], np.float32), 2)
    assert hybrid_ref.fuse_row(*a2, *b, 5, hybrid_ref.WEIGHTED, 0.3, 0.7) == rows
    a3 = (np.array([-1, 1], np.int32), np.array([7.25, 3.0], np.float32), 2)
    assert [d for d, _ in hybrid_ref.fuse_row(*a3, *b, 5, hybrid_ref.WEIGHTED, 0.3, 0.7)] == [4, 2]
    assert [d for d, _ in hybrid_ref.fuse_row(*a3, *b, 5, hybrid_ref.RRF, 1.0, 1.0)] == [4, 1, 2]  # rank 2 of A keeps its rank
    assert hybrid_ref.form(512, 512, 128) == "wave" and hybrid_ref.form(512, 513, 128) == "block" and hybrid_ref.form(100, 100, 129) == "block"
