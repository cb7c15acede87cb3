"""The IVF dense index on the GPU (include/ivf/sparse_rx_ivf.h) against tests/ivf_ref.py: assign, probe and search bit for bit on
small integers with crafted list sizes; on Gaussian rows the search against DenseHalfIndex and its scorer's bits; the centroid
update in the stated order; training by hand; the service."""
import json
import os

import numpy as np
import pytest

import half_ref
import ivf_ref as ref
from test_gpu_parity import _assert_exact

pytestmark = pytest.mark.gpu
DTYPES = list(half_ref.TYPES)
BASE = 7_000_000
SIZES = [140, 0, 33, 1, 31, 32]  # of lists 0 .. 5 where they exist; list c >= 6 gets c % 5 rows


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _dev(x):
    import torch
    return torch.as_tensor(x, device="cuda:0")


# ---- 1. integers: every product and sum exact, ties everywhere ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [64, 200, 768])
@pytest.mark.parametrize("nlist", [1, 3, 33, 130])
def test_integers_bit_for_bit(dtype, dim, nlist):
    import sparse_rx
    rng = np.random.default_rng(1000 * dim + nlist)
    cent = rng.choice([-1.0, 1.0], (nlist, dim)).astype(np.float32)  # equal norms: a copy of a centroid, scaled, belongs to it
    want = [SIZES[c] if c < len(SIZES) else c % 5 for c in range(nlist)]
    owner = rng.permutation(np.repeat(np.arange(nlist), want))
    emb = (cent[owner] * rng.choice([1.0, 2.0], (len(owner), 1))).astype(np.float32)
    ix = sparse_rx.IvfHalfIndex(_dev(emb), nlist, dtype=dtype, centroids=cent, doc_base=BASE)
    doc_list = ref.assign(ref.int_scores(emb, cent))
    assert np.array_equal(ix.list_sizes(), np.bincount(doc_list, minlength=nlist)) and np.array_equal(ix.list_sizes(), want)
    lists, best = ix.assign_device(_dev(emb), with_score=True)
    assert np.array_equal(lists.cpu().numpy(), doc_list) and np.array_equal(best.cpu().numpy(), ref.int_scores(emb, cent).max(axis=1))
    assert np.array_equal(ix.corpus_to_host(), half_ref.round_codes(emb, dtype))
    for i, nq in enumerate((1, 33, 129)):
        q = rng.integers(-2, 3, (nq, dim)).astype(np.float32)
        S, C = ref.int_scores(q, emb), ref.int_scores(q, cent)
        for j, nprobe in enumerate(sorted({1, min(2, nlist), nlist})):
            k = (1, 10, 1024)[(i + j) % 3]
            pl, ps = ix.probe(q, nprobe)
            el, es = ref.probe(C, nprobe)
            assert np.array_equal(pl, el) and np.array_equal(ps.view(np.uint32), es.view(np.uint32)), (nq, nprobe)
            _assert_exact(ix.search(q, k, nprobe), ref.search(S, doc_list, el, k, doc_base=BASE), f"{dtype} dim={dim} nlist={nlist} nq={nq} nprobe={nprobe} k={k}")


# ---- 2. Gaussian rows: the half index's bits --------------------------------------------------------------------------------------
class _Case:
    def __init__(self, dtype):
        import sparse_rx
        rng = np.random.default_rng(5)
        self.n, self.dim, self.nlist, self.nq = 3000, 200, 33, 40
        self.emb = rng.standard_normal((self.n, self.dim)).astype(np.float32)
        self.q = rng.standard_normal((self.nq, self.dim)).astype(np.float32)
        self.cent = self.emb[rng.choice(self.n, self.nlist, replace=False)]
        self.half = sparse_rx.DenseHalfIndex(_dev(self.emb), dtype=dtype, doc_base=BASE)
        self.ix = sparse_rx.IvfHalfIndex(self.emb, self.nlist, dtype=dtype, centroids=self.cent, doc_base=BASE, chunk_rows=1024)  # host rows, in chunks
        all_docs = np.ascontiguousarray(np.broadcast_to(np.arange(self.n, dtype=np.int32) + BASE, (self.nq, self.n)))
        self.S = self.half.score_docs(self.q, all_docs)  # the scorer's bits of every pair


@pytest.fixture(scope="module", params=DTYPES)
def case(request):
    return _Case(request.param)


def test_all_lists_is_the_half_search(case):
    import sparse_rx
    c = case
    masks = np.random.default_rng(6).random((2, c.n)) < np.array([[0.5], [0.01]])
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    q_filter = np.array([(-1, 0, 1)[i % 3] for i in range(c.nq)], np.int32)
    off = float(np.ceil(np.abs(c.S).max()) + 1.0)
    for kw in ({}, {"filter": flt, "q_filter": q_filter}, {"score_offset": off}):
        for k in (10, 1024):
            _assert_exact(c.ix.search(c.q, k, c.nlist, **kw), c.half.search(c.q, k, **kw), f"{c.ix.dtype} k={k} {sorted(kw)}")
    assert np.array_equal(c.ix.score_docs(c.q, np.arange(c.n, dtype=np.int32)[None].repeat(c.nq, 0) + BASE).view(np.uint32), c.S.view(np.uint32))


def test_given_probe_lists(case):
    c = case
    rng = np.random.default_rng(8)
    pl = rng.integers(0, c.nlist, (c.nq, 4)).astype(np.int32)
    pl[::3, 1] = -1         # padding
    pl[1::3, 2] = pl[1::3, 0]  # a repeated list
    doc_list = c.ix.assign(c.emb)
    exp = ref.search(c.S, doc_list, pl, 50, doc_base=BASE)
    got = c.ix.search(c.q, 50, 4, probe_list=pl)
    _assert_exact(got, exp, f"{c.ix.dtype} given lists")
    assert np.array_equal(c.half.score_docs(c.q, got[0], got[2]).view(np.uint32), got[1].view(np.uint32))
    for i in (0, 1, 2):  # alone as in the batch
        _assert_exact(c.ix.search(c.q[i: i + 1], 50, 4, probe_list=pl[i: i + 1]), tuple(x[i: i + 1] for x in exp), f"query {i} alone")


def test_assign_is_the_argmax_of_the_scorer_bits(case):
    import sparse_rx
    c = case
    cix = sparse_rx.DenseHalfIndex(_dev(c.cent), dtype=c.ix.dtype)
    bits = cix.score_docs(c.emb, np.ascontiguousarray(np.broadcast_to(np.arange(c.nlist, dtype=np.int32), (c.n, c.nlist))))
    lists, best = c.ix.assign_device(_dev(c.emb), with_score=True)
    lists, best = lists.cpu().numpy(), best.cpu().numpy()
    assert np.array_equal(lists, ref.assign(bits)) and np.array_equal(best.view(np.uint32), bits.max(axis=1).view(np.uint32))
    qc, dc = half_ref.convert(c.emb, c.ix.dtype, 256)[0], half_ref.convert(c.cent, c.ix.dtype, 256)[0]
    exact, tol = half_ref.exact_scores(qc, dc, c.ix.dtype), half_ref.tol(qc, dc, c.ix.dtype)
    # engine(chosen) >= engine(best) >= exact(best) - tol[best] and engine(chosen) <= exact(chosen) + tol[chosen] <= exact(best) + tol[chosen]
    rows, top = np.arange(c.n), exact.argmax(axis=1)
    err = np.abs(best - exact.max(axis=1)) / np.maximum(tol[rows, lists], tol[rows, top])
    print("assign: largest |chosen score - best fp64 score| / tol =", float(err.max()))
    assert (err <= 1.0).all()


# ---- 3. the centroid update, bit for bit ----------------------------------------------------------------------------------------------
def test_update_in_the_stated_order():
    import sparse_rx.ivf as ivf
    rng = np.random.default_rng(9)
    lens = [0, 1, 255, 256, 257, 513, 0, 5, 1023, 1024, 1025, 2305]  # up to three rounds of four chunks, the last one ragged
    n, dim = sum(lens) + 17, 200
    rows = (rng.standard_normal((n, dim)) * np.exp2(rng.integers(-8, 9, (n, 1)))).astype(np.float32)
    member = np.concatenate([np.sort(m) for m in np.split(rng.permutation(n)[: sum(lens)], np.cumsum(lens)[:-1])]).astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    prev = rng.standard_normal((len(lens), dim)).astype(np.float32)
    got = ivf.update_device(_dev(rows), _dev(ptr), _dev(member), _dev(prev)).cpu().numpy()
    exp = ref.update(rows, ptr, member, prev)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)) and np.array_equal(got[0], prev[0]) and np.array_equal(got[6], prev[6])


@pytest.mark.parametrize("dtype", DTYPES)
def test_training_is_the_steps_by_hand(dtype):
    import torch
    import sparse_rx.ivf as ivf
    x = _dev(np.random.default_rng(10).standard_normal((2000, 72)).astype(np.float32))
    got = ivf.train_centroids(x, 20, dtype, n_iter=2, seed=3)
    cent = x[torch.randperm(2000, generator=torch.Generator().manual_seed(3))[:20].to(x.device)]
    for _ in range(2):
        lists = ivf.assign_device(ivf.pack_half_device(cent, dtype)[0], 20, dtype, x)
        cent = ivf.update_device(x, *ivf.members_of(lists, 20), cent)
    assert torch.equal(got, cent) and torch.equal(got, ivf.train_centroids(x, 20, dtype, n_iter=2, seed=3))
    ix = ivf.IvfHalfIndex(x, 20, dtype=dtype, n_iter=2, seed=3, train_rows=None)
    assert np.array_equal(ix.centroids_to_host(), ivf.train_centroids(x, 20, dtype, n_iter=2, seed=3).cpu().numpy()) and ix.list_sizes().sum() == 2000


# ---- 4. the service -----------------------------------------------------------------------------------------------------------------------
def test_service_with_every_list_probed_is_the_half_storage(golden_dir):
    import sparse_rx
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    out = []
    for kw in ({}, {"ann": "ivf", "nlist": 8, "nprobe": 8}):
        svc = sparse_rx.RetrievalService()
        svc.build_bm25_index(j["corpus"])
        emb = np.random.default_rng(12).standard_normal((len(svc.doc_ids), 48)).astype(np.float32)
        svc.set_embeddings(emb, storage="f16", **kw)
        rng = np.random.default_rng(11)
        vecs = {qid: rng.standard_normal(48).astype(np.float32) for qid in list(j["queries"])[:6]}
        out.append(([svc.search_by_vector(v, 7) for v in vecs.values()], svc.search_hybrid({q: j["queries"][q] for q in vecs}, vecs, top_k=5, rescore=True),
                    svc.get_stats().get("embedding_ann"), svc.get_stats().get("nlist"), svc.get_stats().get("nprobe")))
        if kw:
            with pytest.raises(ValueError, match="not offered"):
                svc.search_hybrid({q: j["queries"][q] for q in vecs}, vecs, top_k=5, mmr_lambda=0.5)
            with pytest.raises(ValueError, match="not offered"):
                svc.diversify(out[-1][1], top_k=3)
        svc.close()
    assert out[0][:2] == out[1][:2] and out[0][2:] == (None, None, None) and out[1][2:] == ("ivf", 8, 8)
