"""The PQ dense index on the GPU (include/pq/sparse_rx_pq.h): codes, tables and scores bit for bit against pq_ref, the ranking
rules, training as the steps by hand, the screened pairing and the service."""
import json
import os

import numpy as np
import pytest

import pq_ref as ref
from test_gpu_parity import _assert_exact

pytestmark = pytest.mark.gpu
BASE = 3_000_000
SHAPES = [(dsub, dim) for dsub in (4, 8, 16) for dim in (3, 200, 512, 1024) if -(-dim // dsub) <= 128]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _dev(x):
    import torch
    return torch.as_tensor(x, device="cuda:0")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _data(rng, n, dim, dsub, nq=33):
    """Gaussian rows scaled by powers of two, untrained codebooks with a duplicated codeword, some rows equal to a codeword."""
    M = ref.subspaces(dim, dsub)
    cb = rng.standard_normal((M, 256, dsub)).astype(np.float32)
    cb[:, 200] = cb[:, 17]  # a tie: the lower code wins
    x = (rng.standard_normal((n, dim)) * np.exp2(rng.integers(-3, 4, (n, 1)))).astype(np.float32)
    flat = cb.transpose(1, 0, 2).reshape(256, -1)[:, :dim]  # codeword c of every subspace as a row
    x[::7] = flat[rng.integers(0, 256, len(x[::7]))]
    x[0] = flat[200]
    q = (rng.standard_normal((nq, dim)) * np.exp2(rng.integers(-2, 3, (nq, 1)))).astype(np.float32)
    return x, cb, q


@pytest.mark.parametrize("n", [1, 193])
@pytest.mark.parametrize("dsub,dim", SHAPES)
def test_bit_for_bit(dsub, dim, n):
    import sparse_rx
    x, cb, q = _data(np.random.default_rng(dim * 100 + dsub + n), n, dim, dsub)
    codes, table = ref.encode(x, cb), ref.lut(q, cb)
    assert (codes[0, : dim // dsub] == 17).all()  # row 0 is codeword 200 = codeword 17 in every whole subspace: the lower code
    ix = sparse_rx.DensePqIndex(_dev(x), dsub=dsub, codebooks=cb, doc_base=BASE)
    assert np.array_equal(ix.encode_device(_dev(x)).cpu().numpy(), codes) and np.array_equal(ix.codes_to_host(), codes)
    assert ix.device_bytes() == -(-n // 64) * 64 * (-(-codes.shape[1] // 16) * 16) + cb.nbytes
    assert np.array_equal(_bits(ix.lut_device(_dev(q)).cpu().numpy()), _bits(table))
    assert np.array_equal(ix.reconstruct(np.arange(n)), ref.reconstruct(codes, cb, dim))
    S = ref.scores(table, codes)
    masks = np.stack([np.random.default_rng(9).random(n) < 0.5, np.zeros(n, bool)])
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    off = np.float32(np.ceil(np.abs(S).max()) + 1.0)  # above max |S|: every doc is rankable
    for i, nq in enumerate((1, 5, 33)):
        k = (1, 10, 1024)[(i + n + dsub) % 3]
        label = f"dsub={dsub} dim={dim} n={n} nq={nq} k={k}"
        _assert_exact(ix.search(q[:nq], k), ref.search(S[:nq], k, doc_base=BASE), label)
        q_filter = np.array([(-1, 0, 1)[j % 3] for j in range(nq)], np.int32)
        allowed = np.stack([np.ones(n, bool) if r < 0 else masks[r] for r in q_filter])
        _assert_exact(ix.search(q[:nq], k, filter=flt, q_filter=q_filter), ref.search(S[:nq], k, allowed=allowed, doc_base=BASE), label + " filtered")
        exp = ref.search(S[:nq], k, score_offset=off, doc_base=BASE)
        assert (exp[2] == min(k, n)).all()
        _assert_exact(ix.search(q[:nq], k, score_offset=float(off)), exp, label + " offset")
    # the scorer of given docs: a duplicate, padding, before and past the corpus, entries behind the count
    cand = np.array([[BASE, BASE, -1, BASE - 1, BASE + n, BASE + n - 1, 0] + [BASE + j % n for j in range(30)], [BASE + n // 2] * 37], np.int32)
    count = np.array([37, 4], np.int32)
    assert np.array_equal(_bits(ix.score_docs(q[:2], cand, count)), _bits(ref.score_docs(S[:2], cand, count, BASE)))
    d, s, c = ix.search(q, min(n, 1024), score_offset=float(off))  # the search's own bits, offset taken back out where exact
    assert np.array_equal(_bits(ix.score_docs(q, d, c) + off), _bits(s))
    _assert_exact(ix.search(q[7:8], 10), tuple(a[7:8] for a in ref.search(S, 10, doc_base=BASE)), "a query alone")


def test_split_rows_and_query_groups():
    import sparse_rx
    x, cb, q = _data(np.random.default_rng(2), 40_000, 64, 16, nq=70)
    codes = ref.encode(x, cb)
    ix = sparse_rx.DensePqIndex(x, dsub=16, codebooks=cb, chunk_rows=16_384)  # a host array: three chunks
    assert np.array_equal(ix.codes_to_host(), codes)
    assert sparse_rx.pq.search_plan(70, 40_000, 4, 10)[1] == 2  # the score row is split and the rank merge runs
    S = ref.scores(ref.lut(q, cb), codes)
    _assert_exact(ix.search(q, 10), ref.search(S, 10), "split rows")
    rec = ref.reconstruct(codes, cb, 64).astype(np.float64)
    assert ix.max_row_norm() == pytest.approx(float((rec * rec).sum(axis=1).max()) ** 0.5, rel=1e-12)  # fp64 sums in two orders


def _mse(x, cb, dsub):
    import sparse_rx.pq as pq
    codes = pq.encode_device(_dev(x), cb, x.shape[1], dsub).cpu().numpy()
    return float(((x.astype(np.float64) - ref.reconstruct(codes, cb.cpu().numpy(), x.shape[1]).astype(np.float64)) ** 2).mean())


def test_training():
    import torch
    import sparse_rx.ivf as ivf
    import sparse_rx.pq as pq
    xh = np.random.default_rng(10).standard_normal((2000, 30)).astype(np.float32)  # dim 30 at dsub 8: a ragged last subspace
    x = _dev(xh)
    got = pq.train_codebooks(x, 8, n_iter=2, seed=3)
    xp = torch.zeros((2000, 32), device=x.device)
    xp[:, :30] = x
    cb = xp[torch.randperm(2000, generator=torch.Generator().manual_seed(3))[:256].to(x.device)].reshape(256, 4, 8).permute(1, 0, 2).contiguous()
    assert torch.equal(cb, pq.initial_codebooks(x, 8, 3))
    for _ in range(2):
        codes = pq.encode_device(x, cb, 30, 8)
        cb = torch.stack([ivf.update_device(xp[:, 8 * m: 8 * m + 8], *ivf.members_of(codes[:, m].int(), 256), cb[m]) for m in range(4)])
    assert torch.equal(got, cb) and torch.equal(got, pq.train_codebooks(x, 8, n_iter=2, seed=3))
    few = pq.initial_codebooks(x[:100], 8, 3)  # fewer than 256 rows: the remaining codewords repeat row 0
    assert torch.equal(few[:, 100:], xp[0].reshape(4, 1, 8).expand(4, 156, 8))
    y = np.random.default_rng(11).standard_normal((2000, 32)).astype(np.float32)
    assert _mse(y, pq.train_codebooks(_dev(y), 8, n_iter=4, seed=0), 8) <= _mse(y, pq.train_codebooks(_dev(y), 8, n_iter=0, seed=0), 8)


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_screen_that_covers_the_corpus_is_the_exact_search(storage):
    import sparse_rx
    x, _, q = _data(np.random.default_rng(4), 193, 72, 8, nq=5)
    exact = sparse_rx.DenseF32Index(x) if storage == "f32" else sparse_rx.DenseHalfIndex(x, dtype="f16")
    pair = sparse_rx.ScreenedDenseIndex(exact, sparse_rx.DensePqIndex(x, dsub=8, n_iter=2), oversample=20)
    assert pair.pool(10) == 193
    _assert_exact(pair.search(q, 10), exact.search(q, 10), storage)
    masks = np.stack([np.arange(193) % 3 == 0])
    flt = sparse_rx.DocFilter.from_masks(masks)
    _assert_exact(pair.search(q, 10, filter=flt), exact.search(q, 10, filter=flt), storage + " filtered")


def test_service(golden_dir):
    import sparse_rx
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    svc = sparse_rx.RetrievalService()
    svc.build_bm25_index(j["corpus"])
    n = len(svc.doc_ids)
    emb = np.random.default_rng(12).standard_normal((n, 48)).astype(np.float32)
    svc.set_embeddings(emb, storage="pq", pq_dsub=8)
    st = svc.get_stats()
    assert (st["embedding_storage"], st["pq_dsub"], st["embedding_screen"]) == ("pq", 8, None)
    ix = sparse_rx.DensePqIndex(emb, dsub=8)  # training is deterministic: the same index
    assert np.array_equal(ix.codes_to_host(), svc._dense.codes_to_host())
    rng = np.random.default_rng(11)
    vecs = {qid: rng.standard_normal(48).astype(np.float32) for qid in list(j["queries"])[:6]}
    for v in vecs.values():
        d, s, c = ix.search(v, 7)
        assert c[0] == 7 and svc.search_by_vector(v, 7) == [{"doc_id": svc.doc_ids[a], "score": float(b)} for a, b in zip(d[0], s[0])]
    texts = {qid: j["queries"][qid] for qid in vecs}
    fused = svc.search_hybrid(texts, vecs, top_k=5, rescore=True)
    with pytest.raises(ValueError, match="not offered"):
        svc.search_hybrid(texts, vecs, top_k=5, mmr_lambda=0.5)
    svc._dense = ix
    assert fused == svc.search_hybrid(texts, vecs, top_k=5, rescore=True) and all(len(r) == 5 for r in fused.values())
    svc.set_embeddings(emb, storage="f16", screen="pq", oversample=3, pq_dsub=4)
    st = svc.get_stats()
    assert (st["embedding_storage"], st["embedding_screen"], st["embedding_oversample"], st["pq_dsub"]) == ("f16", "pq", 3, 4)
    assert all(len(svc.search_by_vector(v, 7)) == 7 for v in vecs.values())
    svc.close()
