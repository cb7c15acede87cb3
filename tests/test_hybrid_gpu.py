"""Hybrid retrieval on the GPU: srx_fuse_topk and the API doors above it against the NumPy restatement
(tests/hybrid_ref.py) fed with the same input rows.  Every comparison is on doc ids, counts and fp32 score BITS."""
import json
import os

import numpy as np
import pytest

import hybrid_ref
import oracle
import sparse_rx
from oracle import np_oracle

pytestmark = pytest.mark.gpu

MODES = ("weighted", "rrf")


def _dev(t):
    import torch
    return tuple(torch.as_tensor(np.ascontiguousarray(x), device="cuda:0") for x in t)


def _run(a, b, k, mode, weights=(0.3, 0.7), rrf_c=60.0):
    import torch
    d, s, n = sparse_rx.fuse_topk_device(_dev(a), _dev(b), k, mode=mode, weights=weights, rrf_c=rrf_c)
    torch.cuda.synchronize()
    return d.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()


def _check(a, b, k, mode, weights=(0.3, 0.7), rrf_c=60.0, tag=None):
    got = _run(a, b, k, mode, weights, rrf_c)
    exp = hybrid_ref.fuse(a, b, k, mode, weights, rrf_c)
    tag = (tag, mode, a[0].shape, b[0].shape, k, weights)
    assert got[0].shape == (len(a[2]), k) and got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert np.array_equal(got[2], exp[2]), tag
    bad = np.nonzero((got[0] != exp[0]).any(axis=1) | (got[1].view(np.uint32) != exp[1].view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (tag, "first differing query", int(bad[0]), got[0][bad[0]][:8], exp[0][bad[0]][:8],
                           got[1][bad[0]][:8], exp[1][bad[0]][:8])
    return got


# (ka, kb, k, the form the host's dispatch rule gives it, queries)
SHAPES = [
    (1, 1, 1, "wave", 5), (10, 10, 10, "wave", 9), (100, 100, 100, "wave", 7), (512, 512, 128, "wave", 5),
    (512, 513, 128, "block", 5), (100, 100, 128, "wave", 5), (100, 100, 129, "block", 5), (1000, 1000, 1000, "block", 3),
    (1024, 1024, 1024, "block", 3), (1024, 3, 1024, "block", 3), (3, 1024, 50, "block", 3), (1023, 1, 128, "wave", 3),
    (10, 10, 100, "wave", 5), (300, 200, 1024, "block", 3),  # k > ka + kb
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ka,kb,k,form,nq", SHAPES)
def test_kernel_shapes_and_overlaps(ka, kb, k, form, nq, mode):
    assert hybrid_ref.form(ka, kb, k) == form  # the case sits on the side of the dispatch boundary it was written for
    for overlap in (0.0, 0.5, 1.0):
        rng = np.random.default_rng(1000 * ka + kb + k + int(10 * overlap))
        a, b = hybrid_ref.make_lists(rng, nq, ka, kb, overlap=overlap)
        got = _check(a, b, k, mode, tag=("overlap", overlap))
        if overlap == 0.0:
            assert np.array_equal(got[2], np.minimum(k, a[2] + b[2]))
        if overlap == 1.0 and ka >= kb:  # full rows: every doc of B is one of A's
            assert got[2][-1] == min(k, ka)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq", [1, 3, 4, 5, 1000])
def test_kernel_partly_filled_last_workgroup(nq, mode):
    assert hybrid_ref.form(24, 16, 10) == "wave"  # four queries per workgroup in this form
    a, b = hybrid_ref.make_lists(np.random.default_rng(nq), nq, 24, 16, overlap=0.5)
    _check(a, b, 10, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ka,kb,k", [(60, 70, 40), (600, 700, 400)])
def test_kernel_empty_sides_and_zero_weights(ka, kb, k, mode):
    assert hybrid_ref.form(ka, kb, k) == ("wave" if ka == 60 else "block")
    rng = np.random.default_rng(ka)
    a, b = hybrid_ref.make_lists(rng, 6, ka, kb, overlap=0.5)
    zero = lambda t: (t[0], t[1], np.zeros_like(t[2]))                       # counts 0: the junk in the rows must be ignored
    neg = lambda t: (t[0], t[1], np.full_like(t[2], -3))                     # negative counts clamp to 0
    mixed = lambda t, m: (t[0], t[1], np.where(np.arange(len(t[2])) % m == 0, 0, t[2]).astype(np.int32))  # per query
    for aa, bb in ((zero(a), b), (a, zero(b)), (zero(a), zero(b)), (neg(a), b), (mixed(a, 2), mixed(b, 3))):
        got = _check(aa, bb, k, mode, tag="empty side")
        if aa[2].max() <= 0 and bb[2].max() <= 0:
            assert not got[2].any() and np.all(got[0] == -1) and np.all(got[1] == 0)
    for w in ((0.0, 1.0), (2.5, 0.0)):
        got = _check(a, b, k, mode, weights=w, tag="zero weight")
        other = b if w[0] == 0.0 else a
        big = _run(a, b, 1024, mode, weights=w)
        for q in range(6):  # the fused SET is the other list's
            assert set(big[0][q, : big[2][q]].tolist()) == set(other[0][q, : other[2][q]].tolist())
    # counts above the row width clamp to it
    over = lambda t: (t[0], np.abs(t[1]) + np.float32(1e-3), np.full_like(t[2], 5000))
    a2, b2 = hybrid_ref.make_lists(rng, 4, ka, kb, overlap=0.3, fill=(1.0, 1.0), garbage=False)
    _check(over(a2), over(b2), k, mode, tag="count > width")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ka,kb,k", [(200, 150, 100), (700, 800, 300)])
def test_kernel_wide_dynamic_range(ka, kb, k, mode):
    """weights and scores over several orders of magnitude inside the normal fp32 range; and a range whose quotients and
    contributions fall into the denormals, which the contract keeps (no flush to zero)."""
    rng = np.random.default_rng(kb)
    a, b = hybrid_ref.make_lists(rng, 6, ka, kb, overlap=0.5, score_range=(1e-3, 1e4))
    for w in ((1e-6, 1e5), (3e4, 2e-5), (1.0, 1e-7)):
        _check(a, b, k, mode, weights=w, rrf_c=0.5, tag="normal range")
    a, b = hybrid_ref.make_lists(rng, 6, ka, kb, overlap=0.5, score_range=(1e-20, 1e18))
    for w in ((1.0, 1.0), (1e-3, 1e-37), (1e-36, 1e-37)):  # the last pair: most contributions are denormal or underflow to 0
        _check(a, b, k, mode, weights=w, rrf_c=1e-3, tag="denormal range")


@pytest.mark.parametrize("n,k", [(50, 50), (50, 7), (500, 100), (600, 600), (1024, 1024)])
def test_kernel_rrf_mirrored_ranks_tie_by_doc(n, k):
    """equal weights, list B = list A reversed: ranks r and n - 1 - r get the same two terms, so the fused scores tie in
    pairs exactly (the sum has two operands: its order does not matter) and doc order must break every tie."""
    rng = np.random.default_rng(n)
    nq = 3
    docs = np.stack([rng.permutation(1 << 16)[:n].astype(np.int32) for _ in range(nq)])
    score = np.tile(np.linspace(9.0, 1.0, n, dtype=np.float32), (nq, 1))
    cnt = np.full(nq, n, np.int32)
    a, b = (docs, score, cnt), (np.ascontiguousarray(docs[:, ::-1]), score, cnt)
    got = _check(a, b, k, "rrf", weights=(1.0, 1.0), tag="mirrored")
    if k >= 2:
        assert got[1][0, 0].view(np.uint32) == got[1][0, 1].view(np.uint32) and got[0][0, 0] < got[0][0, 1]
    # the issue's own example
    a = (np.array([[5, 9]], np.int32), np.array([[3.0, 2.0]], np.float32), np.array([2], np.int32))
    b = (np.array([[9, 5, 7]], np.int32), np.array([[0.9, 0.8, 0.7]], np.float32), np.array([3], np.int32))
    got = _check(a, b, 10, "rrf", weights=(1.0, 1.0))
    assert got[0][0, :3].tolist() == [5, 9, 7] and got[2][0] == 3


def test_device_entry_point_refuses_bad_arguments():
    a, b = hybrid_ref.make_lists(np.random.default_rng(0), 2, 8, 8)
    da, db = _dev(a), _dev(b)
    for kw in (dict(k=0), dict(k=1025), dict(k=4, mode="minmax"), dict(k=4, weights=(0, 0)), dict(k=4, weights=(-1, 1)),
               dict(k=4, mode="rrf", rrf_c=0.0)):
        with pytest.raises(ValueError):
            sparse_rx.fuse_topk_device(da, db, **kw)
    with pytest.raises(ValueError):
        sparse_rx.fuse_topk_device(da, (db[0][:1], db[1][:1], db[2][:1]), 4)
    with pytest.raises(ValueError):
        sparse_rx.fuse_topk_device(da, (db[0].long(), db[1], db[2]), 4)


# ---- end to end, INT8: HybridRetriever against oracle rows fused by the restatement --------------------------------------
@pytest.fixture(scope="module")
def text_corpus():
    from sparse_rx import synth
    return synth.fiqa_shaped_text(n_docs=20_000, vocab=20_000, mean_doc_len=60, n_queries=24, seed=77)


def _expected_int8(r, texts, embs, ka, kb, k, mode, weights, rrf_c):
    h = r.sparse.host
    q_ptr, q_term, q_w = sparse_rx.encode_queries(texts, h.vocabulary)
    sparse = oracle.search_batch(h.indptr, h.indices, h.data, h.doc_lengths, h.idf, q_ptr, q_term, q_w, ka, 1.2, 0.75, h.avgdl)
    qq = [sparse_rx.quantize_query_symmetric(e) for e in embs]
    sims = np_oracle.int8_similarities(np.stack([x for x, _ in qq]), r.dense.corpus_embeddings_int8,
                                       np.array([s for _, s in qq], np.float32), r.dense.corpus_scales)
    dense = np_oracle.dense_topk(sims, kb)
    return hybrid_ref.fuse(sparse, dense, k, mode, weights, rrf_c)


def _assert_dicts(got, qids, exp, doc_ids):
    ed, es, en = exp
    for i, qid in enumerate(qids):
        assert list(got[qid]) == [doc_ids[j] for j in ed[i, : en[i]]], qid  # dict order = rank order
        assert [np.float32(v).view(np.uint32) for v in got[qid].values()] == [x.view(np.uint32) for x in es[i, : en[i]]], qid


@pytest.mark.parametrize("dim,own_embeddings", [(64, False), (48, True)])
def test_hybrid_retriever_int8_end_to_end(text_corpus, dim, own_embeddings):
    corpus, queries = text_corpus
    queries = dict(queries)
    queries["oov"] = "zzzunknown qqqmissing"   # sparse side empty: the dense list re-scored
    queries["blank"] = ""
    r = sparse_rx.RetrieverRegistry.create({"type": "hybrid", "model": {"sparse": "bm25_custom", "dense": "dpr"},
                                            "params": {"top_k": 100, "sparse_weight": 0.3, "dense_weight": 0.7, "embedding_dim": dim}})
    emb = None
    if own_embeddings:  # caller-supplied rows whose length (48) the INT8 engine pads
        emb = np.random.default_rng(3).standard_normal((len(corpus), dim)).astype(np.float32)
    r.build_index_from_corpus(corpus, embeddings=emb)
    assert r.doc_ids == list(corpus) and r.dense._index.dim == dim and r.dense._index.dim_pad == 64
    live = [q for q in queries if queries[q]]
    qemb = {qid: r.dense.query_embedding_from_seed(1000 + i) for i, qid in enumerate(live)}
    texts, embs = [queries[q] for q in live], [qemb[q] for q in live]
    for mode in MODES:
        for top_k, cand in ((10, 100), (100, 100), (10, 1000), (100, 1000)):
            r.fusion, r.candidates = mode, cand
            got = r.search(queries, top_k=top_k, query_embeddings=qemb)
            assert got["blank"] == {} and list(got) == list(queries)
            exp = _expected_int8(r, texts, embs, cand, cand, top_k, mode, (0.3, 0.7), 60.0)
            _assert_dicts(got, live, exp, r.doc_ids)
            assert len(got["oov"]) == top_k and exp[2].max() == top_k
    # candidates default to top_k; a sparse-only weight leaves the out-of-vocabulary query empty
    r.fusion, r.candidates, r.sparse_weight, r.dense_weight = "weighted", None, 1.0, 0.0
    got = r.search(queries, top_k=20, query_embeddings=qemb)
    _assert_dicts(got, live, _expected_int8(r, texts, embs, 20, 20, 20, "weighted", (1.0, 0.0), 60.0), r.doc_ids)
    assert got["oov"] == {}
    # without query_embeddings the mirror's own simulated vectors are used (process-dependent seed: shape check only)
    sim = r.search({"q": queries[live[0]]}, top_k=5)
    assert len(sim["q"]) == 5
    assert r.search(queries, top_k=0) == {q: {} for q in queries}
    with pytest.raises(ValueError, match="1024"):
        r.search(queries, top_k=1025)
    with pytest.raises(ValueError, match="no query embedding"):
        r.search(queries, top_k=5, query_embeddings={})
    with pytest.raises(ValueError, match="shape"):
        r.search(queries, top_k=5, query_embeddings={q: np.ones(dim + 1, np.float32) for q in queries})
    r.close()


# ---- end to end, service: BM25 index + f32 embedding index ---------------------------------------------------------------
def _rows_from_dicts(res, qids, row_of, k):
    d = np.full((len(qids), k), -1, np.int32)
    s = np.zeros((len(qids), k), np.float32)
    n = np.zeros(len(qids), np.int32)
    for i, q in enumerate(qids):
        items = list(res[q].items())
        n[i] = len(items)
        for j, (doc, sc) in enumerate(items):
            d[i, j], s[i, j] = row_of[doc], np.float32(sc)
    return d, s, n


def test_service_search_hybrid_end_to_end(golden_dir):
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    queries = dict(j["queries"])
    queries["blank"] = "   "
    queries["oov"] = "zzzunknown qqqmissing"
    dim = 96
    rng = np.random.default_rng(11)
    svc = sparse_rx.RetrievalService()
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    with pytest.raises(ValueError, match="BM25 index not built"):
        svc.search_hybrid(queries, vecs)
    svc.build_bm25_index(j["corpus"])
    with pytest.raises(ValueError, match="No embedding index"):
        svc.search_hybrid(queries, vecs)
    n_docs = len(j["corpus"])
    svc.set_embeddings(rng.standard_normal((n_docs, dim)).astype(np.float32))
    row_of = {d: i for i, d in enumerate(svc.doc_ids)}
    live = [q for q in queries if queries[q].strip()]
    for mode in MODES:
        for top_k, cand, w in ((10, None, (0.3, 0.7)), (10, 100, (0.3, 0.7)), (100, 1000, (0.5, 0.5)), (1024, 5, (2.0, 1.0))):
            k = min(top_k, n_docs)
            c = min(cand or top_k, n_docs, 1024)
            got = svc.search_hybrid(queries, vecs, top_k=top_k, sparse_weight=w[0], dense_weight=w[1], fusion=mode, candidates=cand)
            assert list(got) == list(queries) and got["blank"] == {}
            sparse = _rows_from_dicts(svc.search_bm25({q: queries[q] for q in live}, top_k=c), live, row_of, c)
            dense = svc._dense.search(np.stack([vecs[q] for q in live]), c)
            _assert_dicts(got, live, hybrid_ref.fuse(sparse, dense, k, mode, w), svc.doc_ids)
            assert sparse[2][live.index("oov")] == 0 and 0 < len(got["oov"]) <= k  # the dense list re-scored
    assert svc.search_hybrid(queries, vecs, top_k=0) == {q: {} for q in queries}
    assert svc.search_hybrid(queries, vecs, top_k=-5) == {q: {} for q in queries}
    with pytest.raises(ValueError, match="1024"):
        svc.search_hybrid(queries, vecs, top_k=1025)
    with pytest.raises(ValueError, match="no query vector"):
        svc.search_hybrid(queries, {q: v for q, v in vecs.items() if q != "q3"})
    with pytest.raises(ValueError, match="shape"):
        svc.search_hybrid(queries, dict(vecs, q3=np.ones(dim + 1, np.float32)))
    svc.search_hybrid({"blank": ""}, {})  # a blank query needs no vector
    svc.close()


def test_fusion_is_stream_ordered():
    """sparse search, dense search and fusion enqueued on a non-default stream, one synchronisation at the end: the same
    rows as the restatement gives for the two engines' own rows (read back afterwards)."""
    import torch
    from sparse_rx import synth
    c = synth.uniform_corpus_np(30_000, 3_000, 20, seed=5)
    _, idf, avgdl = synth.corpus_stats(c)
    q = synth.queries_np(200, c.vocab, 6, seed=6)
    ix = sparse_rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, device="cuda:0", tile_log2=12)
    rng = np.random.default_rng(8)
    c8 = rng.integers(-127, 128, (30_000, 64), dtype=np.int8)
    q8 = rng.integers(-127, 128, (200, 64), dtype=np.int8)
    dx = sparse_rx.DenseInt8Index(c8, rng.uniform(0.5, 1.5, 30_000).astype(np.float32) / 127)
    qs = torch.as_tensor(rng.uniform(0.5, 1.5, 200).astype(np.float32) / 127, device="cuda:0")
    qp, qt, qw = _dev((q[0].astype(np.int32), q[1].astype(np.int32), q[2].astype(np.float32)))
    tq8 = torch.as_tensor(q8, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    for ka, kb, k in ((100, 100, 100), (600, 600, 200)):
        with torch.cuda.stream(side):
            a = ix.search_device(qp, qt, qw, ka)
            b = dx.search_device(tq8, qs, kb)
            f = sparse_rx.fuse_topk_device(a, b, k, mode="rrf", weights=(1.0, 1.0))
        side.synchronize()
        host = lambda t: tuple(x.cpu().numpy() for x in t)
        exp = hybrid_ref.fuse(host(a), host(b), k, "rrf", (1.0, 1.0))
        got = host(f)
        assert np.array_equal(got[2], exp[2]) and np.array_equal(got[0], exp[0])
        assert np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32))
        assert np.all(host(a)[2] > 0) and np.all(host(b)[2] == kb)
    ix.close()
