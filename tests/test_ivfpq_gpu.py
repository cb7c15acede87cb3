"""The IVF-PQ dense index on the GPU (include/ivfpq/sparse_rx_ivfpq.h): codes and scores bit for bit against ivfpq_ref with the
coarse term made exact (integer centroids and queries), slices that cut lists, the assignment, training as the steps by hand,
the screened pairing and both service spellings."""
import json
import os

import numpy as np
import pytest

import ivf_ref
import ivfpq_ref as ref
from test_gpu_parity import _assert_exact

pytestmark = pytest.mark.gpu
BASE = 3_000_000
SIZES = (0, 1, 63, 64, 65, 200)  # docs per list: none, one, a tile less one, a tile, a tile and one, several tiles
SHAPES = [(4, 3, "f16"), (8, 200, "bf16"), (8, 768, "f16"), (16, 1024, "bf16")]  # 1, 2, 6 and 4 pieces per row


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _dev(x):
    import torch
    return torch.as_tensor(x, device="cuda:0")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _data(rng, sizes, dim, dsub, nq=33):
    """Integer centroids and queries (exact in f16 and bf16), rows = centroid + Gaussian noise scaled by powers of two, lists in
    shuffled doc order, untrained codebooks with a duplicated codeword."""
    nlist, n = len(sizes), sum(sizes)
    cent = rng.integers(-4, 5, (nlist, dim)).astype(np.float32)
    lists = rng.permutation(np.repeat(np.arange(nlist), sizes)).astype(np.int32)
    x = (cent[lists] + rng.standard_normal((n, dim)) * np.exp2(rng.integers(-3, 2, (n, 1)))).astype(np.float32)
    cb = rng.standard_normal((-(-dim // dsub), 256, dsub)).astype(np.float32)
    cb[:, 200] = cb[:, 17]  # a tie: the lower code wins
    q = rng.integers(-3, 4, (nq, dim)).astype(np.float32)
    return cent, lists, x, cb, q


def _build(cent, lists, x, cb, dsub, dtype, **kw):
    import sparse_rx
    return sparse_rx.IvfPqIndex(_dev(x), len(cent), dsub=dsub, dtype=dtype, centroids=cent, codebooks=cb, lists=lists, **kw)


@pytest.mark.parametrize("dsub,dim,dtype", SHAPES)
def test_bit_for_bit(dsub, dim, dtype):
    import sparse_rx
    cent, lists, x, cb, q = _data(np.random.default_rng(dim + dsub), SIZES, dim, dsub)
    n, nlist = len(x), len(SIZES)
    ix = _build(cent, lists, x, cb, dsub, dtype, doc_base=BASE)
    codes = ref.codes(x, lists, cent, dtype, cb)
    assert np.array_equal(ix.codes_to_host(), codes) and np.array_equal(ix.list_sizes(), SIZES) and np.array_equal(ix.list_of_docs(), lists)
    assert np.array_equal(ix.reconstruct(np.arange(n)), ref.reconstruct(codes, lists, cent, dtype, cb, dim))
    coarse = ivf_ref.int_scores(q, cent)
    S = ref.scores(q, coarse, lists, codes, cb)
    assert np.array_equal(_bits(ix.probe(q, 3)[1]), _bits(ref.probe(coarse, 3)[1])) and np.array_equal(ix.probe(q, 3)[0], ref.probe(coarse, 3)[0])
    masks = np.stack([np.random.default_rng(9).random(n) < 0.5, np.zeros(n, bool)])
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    off = np.float32(np.ceil(np.abs(S).max()) + 1.0)  # above max |S|: every doc is rankable
    for i, nq in enumerate((1, 5, 33)):
        k, nprobe = (1, 10, 1024)[(i + dsub // 4) % 3], (1, 3, nlist)[(i + dim) % 3]
        label = f"dsub={dsub} dim={dim} nq={nq} k={k} nprobe={nprobe}"
        pl = ref.probe(coarse[:nq], nprobe)[0]
        _assert_exact(ix.search(q[:nq], k, nprobe), ref.search(S[:nq], lists, pl, k, doc_base=BASE), label)
        q_filter = np.array([(-1, 0, 1)[j % 3] for j in range(nq)], np.int32)
        allowed = np.stack([np.ones(n, bool) if r < 0 else masks[r] for r in q_filter])
        _assert_exact(ix.search(q[:nq], k, nprobe, filter=flt, q_filter=q_filter), ref.search(S[:nq], lists, pl, k, allowed=allowed, doc_base=BASE),
                      label + " filtered")
        _assert_exact(ix.search(q[:nq], k, nprobe, score_offset=float(off)), ref.search(S[:nq], lists, pl, k, score_offset=off, doc_base=BASE), label + " offset")
    given = np.array([[5, -1, 5, 2, nlist] if j % 2 else [3, 3, 0, 1, 4] for j in range(33)], np.int32)  # -1, a repeat, out of range, an empty list
    _assert_exact(ix.search(q, 10, 5, probe_list=given, score_offset=float(off)), ref.search(S, lists, given, 10, score_offset=off, doc_base=BASE), "probe_list")
    # the scorer of given docs: a duplicate, padding, before and past the corpus, entries behind the count
    cand = np.array([[BASE, BASE, -1, BASE - 1, BASE + n, BASE + n - 1, 0] + [BASE + j % n for j in range(30)], [BASE + n // 2] * 37], np.int32)
    count = np.array([37, 4], np.int32)
    assert np.array_equal(_bits(ix.score_docs(q[:2], cand, count)), _bits(ref.score_docs(S[:2], cand, count, BASE)))
    d, s, c = ix.search(q, n, nlist, score_offset=float(off))  # the search's own bits, offset taken back out where exact
    assert (c == n).all() and np.array_equal(_bits(ix.score_docs(q, d, c) + off), _bits(s))
    full = ref.search(S, lists, ref.probe(coarse, 3)[0], 10, doc_base=BASE)
    _assert_exact(ix.search(q[7:8], 10, 3), tuple(a[7:8] for a in full), "a query alone")


def test_slices_cut_lists():
    sizes = (3, 40 * 64 + 5, 70)  # one list of 41 tiles beside short ones
    cent, lists, x, cb, q = _data(np.random.default_rng(5), sizes, 8, 4, nq=2)
    ix = _build(cent, lists, x, cb, 4, "f16")
    P, S, L, _ = ix.search_plan(1, 10, 3)
    assert (P, L) == (1, 16) and S == 8 >= 2  # 44 tiles in slices of 6: boundaries inside the long list and at list ends
    codes, coarse = ref.codes(x, lists, cent, "f16", cb), ivf_ref.int_scores(q, cent)
    assert np.array_equal(ix.codes_to_host(), codes)
    Sc = ref.scores(q, coarse, lists, codes, cb)
    off = np.float32(np.ceil(np.abs(Sc).max()) + 1.0)
    for nprobe, k in ((3, 1024), (1, 10), (2, 100)):
        for one in (q[:1], q[1:2]):
            c = ivf_ref.int_scores(one, cent)
            exp = ref.search(ref.scores(one, c, lists, codes, cb), lists, ref.probe(c, nprobe)[0], k, score_offset=off)
            _assert_exact(ix.search(one, k, nprobe, score_offset=float(off)), exp, f"nprobe={nprobe} k={k}")
    given = np.array([[1, -1, 1]], np.int32)  # the long list alone
    _assert_exact(ix.search(q[:1], 10, 3, probe_list=given, score_offset=float(off)), ref.search(Sc[:1], lists, given, 10, score_offset=off), "the long list")


def test_assignment():
    import sparse_rx
    rng = np.random.default_rng(6)
    cent = rng.integers(-4, 5, (7, 40)).astype(np.float32)
    x = rng.integers(-3, 4, (300, 40)).astype(np.float32)
    cb = rng.standard_normal((5, 256, 8)).astype(np.float32)
    ix = sparse_rx.IvfPqIndex(x, 7, dsub=8, dtype="bf16", centroids=cent, codebooks=cb, chunk_rows=64)  # a host array, several chunks
    lists = ivf_ref.assign(ivf_ref.int_scores(x, cent))
    assert np.array_equal(ix.list_of_docs(), lists) and np.array_equal(ix.codes_to_host(), ref.codes(x, lists, cent, "bf16", cb))


def test_training():
    import torch
    import sparse_rx
    from sparse_rx import ivf, pq
    x = _dev(np.random.default_rng(10).standard_normal((2000, 30)).astype(np.float32))
    ix = sparse_rx.IvfPqIndex(x, 8, dsub=8, n_iter=2, seed=3, train_rows=None)
    cent = ivf.train_centroids(x, 8, "f16", 2, 3)
    own = ivf.assign_device(ivf.pack_half_device(cent, "f16")[0], 8, "f16", x).long()
    cb = pq.train_codebooks(x - cent.half().float()[own], 8, 2, 3)  # the residual: one f32 subtraction
    assert torch.equal(ix.centroids_f32, cent) and torch.equal(ix.codebooks, cb) and torch.equal(ix.lists.long(), own)
    again = sparse_rx.IvfPqIndex(x, 8, dsub=8, n_iter=2, seed=3, train_rows=None)
    assert torch.equal(ix.codes, again.codes) and torch.equal(ix.row_doc, again.row_doc)
    sub = sparse_rx.IvfPqIndex(x, 8, dsub=8, n_iter=1, seed=3, train_rows=500)  # a sample: the same rows every time
    assert torch.equal(sub.codes, sparse_rx.IvfPqIndex(x.cpu().numpy(), 8, dsub=8, n_iter=1, seed=3, train_rows=500).codes)


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_screen_that_covers_the_corpus_is_the_exact_search(storage):
    import sparse_rx
    x = np.random.default_rng(4).standard_normal((193, 72)).astype(np.float32)
    q = np.random.default_rng(5).standard_normal((5, 72)).astype(np.float32)
    exact = sparse_rx.DenseF32Index(x) if storage == "f32" else sparse_rx.DenseHalfIndex(x, dtype="f16")
    screen = sparse_rx.IvfPqIndex(x, 5, dsub=8, n_iter=2)
    screen.default_nprobe = 5
    pair = sparse_rx.ScreenedDenseIndex(exact, screen, oversample=20)
    assert pair.pool(10) == 193
    _assert_exact(pair.search(q, 10), exact.search(q, 10), storage)
    flt = sparse_rx.DocFilter.from_masks(np.stack([np.arange(193) % 3 == 0]))
    _assert_exact(pair.search(q, 10, filter=flt), exact.search(q, 10, filter=flt), storage + " filtered")


def test_service(golden_dir):
    import sparse_rx
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    svc = sparse_rx.RetrievalService()
    svc.build_bm25_index(j["corpus"])
    n = len(svc.doc_ids)
    emb = np.random.default_rng(12).standard_normal((n, 48)).astype(np.float32)
    vecs = {qid: np.random.default_rng(11 + i).standard_normal(48).astype(np.float32) for i, qid in enumerate(list(j["queries"])[:4])}
    svc.set_embeddings(emb, storage="pq", ann="ivfpq", nlist=4, nprobe=2, pq_dsub=8)
    st = svc.get_stats()
    assert (st["embedding_storage"], st["embedding_ann"], st["nlist"], st["nprobe"], st["pq_dsub"]) == ("pq", "ivfpq", 4, 2, 8)
    ix = sparse_rx.IvfPqIndex(emb, 4, dsub=8)  # training is deterministic: the same index
    assert np.array_equal(ix.codes_to_host(), svc._dense.codes_to_host())
    cand = {qid: [svc.doc_ids[0], svc.doc_ids[n - 1]] for qid in vecs}
    by_vec = svc.score_by_vector(vecs, cand)
    for qid, v in vecs.items():
        d, s, c = ix.search(v, 7, 2)
        assert c[0] == 7 and svc.search_by_vector(v, 7) == [{"doc_id": svc.doc_ids[a], "score": float(b)} for a, b in zip(d[0], s[0])]
        direct = ix.score_docs(v, np.array([[0, n - 1]], np.int32))[0]
        assert [by_vec[qid][doc] for doc in cand[qid]] == [float(a) for a in direct]
    texts = {qid: j["queries"][qid] for qid in vecs}
    assert all(len(r) == 5 for r in svc.search_hybrid(texts, vecs, top_k=5, rescore=True).values())
    with pytest.raises(ValueError, match="not offered"):
        svc.search_hybrid(texts, vecs, top_k=5, mmr_lambda=0.5)
    svc.set_embeddings(emb, storage="f16", screen="pq", ann="ivfpq", nlist=4, nprobe=4, oversample=3, pq_dsub=4)
    st = svc.get_stats()
    assert (st["embedding_storage"], st["embedding_screen"], st["embedding_ann"], st["nlist"], st["nprobe"]) == ("f16", "pq", "ivfpq", 4, 4)
    half = sparse_rx.DenseHalfIndex(emb, dtype="f16")
    for qid, v in vecs.items():
        got = svc.search_by_vector(v, 7)
        assert len(got) == 7 and all(r["score"] == float(half.score_docs(v, np.array([[svc.doc_ids.index(r["doc_id"])]], np.int32))[0, 0]) for r in got)
    assert svc.score_by_vector(vecs, cand)[next(iter(vecs))][svc.doc_ids[0]] == float(half.score_docs(next(iter(vecs.values())), np.array([[0]], np.int32))[0, 0])
    svc.close()
