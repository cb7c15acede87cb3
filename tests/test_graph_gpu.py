"""The graph dense index on the GPU (include/graph/sparse_rx_graph.h) against tests/graph_ref.py: the walk bit for bit on small
integers over graphs of arbitrary contents and on Gaussian rows over the scorer's bits; a walk that reaches everything against the
exhaustive search; prune and merge against their restatements; the build by hand; the service.  No tolerances anywhere."""
import json
import os

import numpy as np
import pytest

import graph_ref as ref
import half_ref
from test_gpu_parity import _assert_exact

pytestmark = pytest.mark.gpu
DTYPES = list(half_ref.TYPES)
BASE = 7_000_000


def _dev(x):
    import torch
    return torch.as_tensor(x, device="cuda:0")


def _check(ix, V, graph, q, L, p, T, k, label, seeds=None, n_seed=None, masks=None, q_filter=None, score_offset=0.0):
    import sparse_rx
    kw, allowed = {}, None
    if masks is not None:
        kw = {"filter": sparse_rx.DocFilter.from_masks(masks, doc_base=ix.doc_base), "q_filter": q_filter}
        allowed = np.stack([np.ones(V.shape[1], bool) if r < 0 else masks[r] for r in q_filter])
    got = ix.search(q, k, itopk=L, width=p, max_iter=T, seeds=seeds if seeds is not None else n_seed, score_offset=score_offset, with_stats=True, **kw)
    exp = ref.search(V, graph, L, p, T, k, seeds=seeds, n_seed=n_seed, doc_base=ix.doc_base, allowed=allowed, score_offset=score_offset)
    _assert_exact(got[:3], exp[:3], label)
    assert np.array_equal(got[3], exp[3]), f"{label}: steps / docs scored differ at {np.flatnonzero((got[3] != exp[3]).any(axis=1))[:8]}"
    return got


# ---- 1. integers: every score exact, ties everywhere, graphs of arbitrary contents -------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,dim,degree", [(1, 64, 16), (33, 200, 32), (700, 1024, 64), (700, 200, 16), (700, 64, 32)])
def test_integers_bit_for_bit(dtype, n, dim, degree):
    import sparse_rx
    rng = np.random.default_rng(1000 * dim + n + degree)
    emb = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    g = rng.integers(-1, n + 3, (n, degree)).astype(np.int32)  # -1, ids >= n_docs, and by chance repeats and self loops
    g[::7] = -1
    g[1::5, 1] = g[1::5, 0]
    g[2::5, 2] = np.arange(n, dtype=np.int32)[2::5]
    ix = sparse_rx.GraphHalfIndex(_dev(emb), degree=degree, dtype=dtype, graph=g, doc_base=BASE)
    assert np.array_equal(ix.graph_to_host(), g) and np.array_equal(ix.corpus_to_host(), half_ref.round_codes(emb, dtype))
    queries = rng.integers(-2, 3, (300, dim)).astype(np.float32)
    S = (queries.astype(np.int64) @ emb.astype(np.int64).T).astype(np.float32)
    masks = rng.random((2, n)) < np.array([[0.5], [0.05]])
    per_step = 128 // degree  # parents whose rows are 128 entries
    # (L, p, T, k, n_seed, nq): L = k = 32 with p = 1 and T = 1; L = 512 with p = 8 (p * degree = 512 at degree 64) and k = 1; a budget of
    # exactly 8192 = 128 + 63 * 128
    for L, p, T, k, n_seed, nq in [(32, 1, 1, 32, 1, 300), (512, 8, 8, 1, 512, 1), (64, per_step, 63, 10, 128, 33)]:
        _check(ix, S[:nq], g, queries[:nq], L, p, T, k, f"{dtype} n={n} dim={dim} degree={degree} L={L} p={p} T={T}", n_seed=n_seed)
    seeds = rng.integers(BASE - 2, BASE + n + 2, (33, 9)).astype(np.int32)  # ids on both sides of the corpus
    seeds[:, 3], seeds[::2, 5] = seeds[:, 0], -1
    q_filter = np.array([(-1, 0, 1)[i % 3] for i in range(33)], np.int32)
    _check(ix, S[:33], g, queries[:33], 96, 4, 5, 7, f"{dtype} n={n} given seeds", seeds=seeds)
    _check(ix, S[:33], g, queries[:33], 96, 4, 5, 96, f"{dtype} n={n} filtered, offset", seeds=seeds, masks=masks, q_filter=q_filter, score_offset=3.0)


# ---- 2. Gaussian rows: the scorer's bits, and a graph the index built ----------------------------------------------------------
class _Case:
    def __init__(self, dtype):
        import sparse_rx
        rng = np.random.default_rng(5)
        self.n, self.dim, self.nq = 3000, 200, 40
        self.emb = rng.standard_normal((self.n, self.dim)).astype(np.float32)
        self.q = rng.standard_normal((self.nq, self.dim)).astype(np.float32)
        self.half = sparse_rx.DenseHalfIndex(_dev(self.emb), dtype=dtype, doc_base=BASE)
        self.ix = sparse_rx.GraphHalfIndex(_dev(self.emb), degree=32, dtype=dtype, builder="exact", doc_base=BASE)
        all_docs = np.ascontiguousarray(np.broadcast_to(np.arange(self.n, dtype=np.int32) + BASE, (self.nq, self.n)))
        self.V = self.half.score_docs(self.q, all_docs)  # the scorer's bits of every pair


@pytest.fixture(scope="module", params=DTYPES)
def case(request):
    return _Case(request.param)


def test_gaussian_walk_has_the_scorer_bits(case):
    c = case
    g = c.ix.graph_to_host()
    got = _check(c.ix, c.V, g, c.q, 64, 4, 20, 10, f"{c.ix.dtype} gaussian", n_seed=64)
    assert (got[3][:, 0] <= 20).all() and (got[3][:, 1] <= 64 + 20 * 4 * 32).all(), "steps and docs scored stay within the call's budget"
    assert np.array_equal(c.half.score_docs(c.q, got[0], got[2]).view(np.uint32), got[1].view(np.uint32))
    for i in (0, 1, 39):  # alone as in the batch
        alone = c.ix.search(c.q[i: i + 1], 10, itopk=64, width=4, max_iter=20, seeds=64)
        _assert_exact(alone, tuple(x[i: i + 1] for x in got[:3]), f"query {i} alone")
    off = float(np.ceil(np.abs(c.V).max()) + 1.0)
    _check(c.ix, c.V, g, c.q, 128, 2, 30, 128, f"{c.ix.dtype} gaussian, offset", n_seed=32, score_offset=off)


# ---- 3. a walk that reaches everything is the exhaustive search ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_walk_that_reaches_everything_is_the_half_search(dtype):
    import sparse_rx
    rng = np.random.default_rng(7)
    n, dim = 300, 200
    emb = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((20, dim)).astype(np.float32)
    g = rng.integers(0, n, (n, 16)).astype(np.int32)  # random chords ...
    g[:, 0] = (np.arange(n) + 1) % n                   # ... and a ring
    half = sparse_rx.DenseHalfIndex(_dev(emb), dtype=dtype, doc_base=BASE)
    ix = sparse_rx.GraphHalfIndex(_dev(emb), degree=16, dtype=dtype, graph=g, doc_base=BASE)
    masks = rng.random((2, n)) < np.array([[0.5], [0.02]])
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    q_filter = np.array([(-1, 0, 1)[i % 3] for i in range(20)], np.int32)
    all_docs = np.ascontiguousarray(np.broadcast_to(np.arange(n, dtype=np.int32) + BASE, (20, n)))
    off = float(np.ceil(np.abs(half.score_docs(q, all_docs)).max()) + 1.0)
    for kw in ({}, {"filter": flt, "q_filter": q_filter}, {"score_offset": off}):
        for k in (10, 300):
            got = ix.search(q, k, itopk=512, width=4, max_iter=64, seeds=1, with_stats=True, **kw)  # from row 0 alone
            assert (got[3][:, 1] == n).all(), "the walk scored every doc"
            _assert_exact(got[:3], half.search(q, k, **kw), f"{dtype} k={k} {sorted(kw)}")


# ---- 4. prune and merge against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,degree", [(1, 16), (65, 32), (65, 64), (2000, 16)])
@pytest.mark.parametrize("wide", [1, 2, 0])  # d0 = degree, 2 * degree, 128
def test_prune_and_merge(n, degree, wide):
    import sparse_rx.graph as graph
    d0 = wide * degree if wide else 128
    rng = np.random.default_rng(n + degree + d0)
    knn = rng.integers(-2, n + 2, (n, d0)).astype(np.int32)  # invalid ids on both sides; at n = 65 every row repeats itself
    near = (np.arange(n)[:, None] + rng.integers(1, 2 * degree, (n, d0))) % n  # neighbours of neighbours overlap: real detours, and
    knn[::2] = near[::2]                                                       # a target that sits in a neighbour's row more than once
    knn[1::4, 3] = knn[1::4, 1]
    knn[knn == n - 1] = -1  # nobody points at the last node: no reverse edges
    knn[::2, 0] = 0         # every other node points at node 0: more than degree / 2 of them
    pruned = graph.prune_device(_dev(knn), degree).cpu().numpy()
    assert np.array_equal(pruned, ref.prune(knn, degree)), np.flatnonzero((pruned != ref.prune(knn, degree)).any(axis=1))[:8]
    for fwd in (pruned, knn[:, :degree].copy()):  # the pruned graph, and rows with invalid and repeated entries
        merged = graph.merge_device(_dev(fwd)).cpu().numpy()
        exp = ref.merge(fwd)
        assert np.array_equal(merged, exp), np.flatnonzero((merged != exp).any(axis=1))[:8]
    if n > 1:
        incoming = np.bincount(pruned[(pruned >= 0)], minlength=n)
        assert incoming[n - 1] == 0 and incoming[0] > degree // 2


# ---- 5. the build by hand ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_build_is_the_steps_by_hand(dtype):
    import torch
    import sparse_rx
    import sparse_rx.graph as graph
    x = np.random.default_rng(10).standard_normal((2000, 72)).astype(np.float32)
    ix = sparse_rx.GraphHalfIndex(_dev(x), degree=16, dtype=dtype, builder="exact", build_degree=40)
    half = sparse_rx.DenseHalfIndex(_dev(x), dtype=dtype)
    knn = half.search(x, 41, score_offset=graph.knn_score_offset(half.max_row_norm()))[0]
    by_hand = graph.merge_device(graph.prune_device(_dev(knn), 16))
    assert torch.equal(ix.graph, by_hand) and (knn[:, 0] == np.arange(2000)).mean() > 0.99  # the self hit leads its list
    again = sparse_rx.GraphHalfIndex(_dev(x), degree=16, dtype=dtype, builder="exact", build_degree=40)
    assert torch.equal(ix.graph, again.graph) and ix.device_bytes() == half.device_bytes() + 2000 * 16 * 4
    via_knn = sparse_rx.GraphHalfIndex(_dev(x), degree=16, dtype=dtype, knn=knn)
    assert torch.equal(via_knn.graph, ix.graph) and set(ix.build_seconds) == {"knn", "prune", "merge"}


# ---- 6. the service ------------------------------------------------------------------------------------------------------------------
def test_service_with_a_beam_as_wide_as_the_corpus_is_the_half_storage(golden_dir):
    import sparse_rx
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    n = len(j["corpus"])
    assert n <= 512, "the golden corpus fits a beam"
    out = []
    for kw in ({}, {"ann": "graph", "graph_degree": 16, "itopk": -(-n // 32) * 32, "search_width": 8}):
        svc = sparse_rx.RetrievalService()
        svc.build_bm25_index(j["corpus"])
        emb = np.random.default_rng(12).standard_normal((len(svc.doc_ids), 48)).astype(np.float32)
        svc.set_embeddings(emb, storage="f16", **kw)
        rng = np.random.default_rng(11)
        vecs = {qid: rng.standard_normal(48).astype(np.float32) for qid in list(j["queries"])[:6]}
        out.append(([svc.search_by_vector(v, 7) for v in vecs.values()], svc.search_hybrid({q: j["queries"][q] for q in vecs}, vecs, top_k=5, rescore=True),
                    svc.get_stats().get("embedding_ann"), svc.get_stats().get("graph_degree"), svc.get_stats().get("itopk")))
        if kw:
            stat = svc._dense.search(np.stack(list(vecs.values())), 7, with_stats=True)[3]
            assert (stat[:, 1] == n).all(), "every doc was reached"
            with pytest.raises(ValueError, match="not offered"):
                svc.search_hybrid({q: j["queries"][q] for q in vecs}, vecs, top_k=5, mmr_lambda=0.5)
            with pytest.raises(ValueError, match="not offered"):
                svc.diversify(out[-1][1], top_k=3)
        svc.close()
    assert out[0][:2] == out[1][:2] and out[0][2:] == (None, None, None) and out[1][2:] == ("graph", 16, -(-n // 32) * 32)
