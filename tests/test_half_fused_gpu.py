"""srx_dense_search_half_fused on the GPU (include/fused/sparse_rx_half_fused.h): the same words as srx_dense_search_half, and on
operands whose products and sums are exact the lists of a float64 NumPy ranking.  The shapes sit just past the edges of the
header's constants: the smallest corpus that gets a sample, the largest that gets none, one row more than a candidate buffer."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import parity  # noqa: E402
from test_gpu_parity import _assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ["f16", "bf16"]
BASE = 3_000_000


def _index(emb, dtype):
    import torch
    import sparse_rx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return sparse_rx.DenseHalfIndex(torch.as_tensor(emb, device="cuda:0"), dtype=dtype, doc_base=BASE)


def _numpy_rows(emb, q, k, offset=0.0):
    """(value descending, doc ascending) of fl32(score + offset) > 0 from float64 dot products: exact operands only"""
    S = (q.astype(np.float64) @ emb.astype(np.float64).T).astype(np.float32) + np.float32(offset)
    d, s, c = parity.dense_topk_rows(S, k)
    return np.where(d >= 0, d + BASE, d).astype(np.int32), s, c


def _small_ints(rng, shape):
    return rng.integers(-2, 3, shape).astype(np.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_small_integers_on_the_sample_side(dtype):
    from sparse_rx import _capi
    n, nq, dim, k = _capi.SRX_HALF_FUSED_MIN_DOCS + 7, 130, 80, 10  # two query blocks, a ragged last tile of queries and of docs
    assert _capi.half_fused_sample(n, k) > 0 == _capi.half_fused_sample(_capi.SRX_HALF_FUSED_MIN_DOCS - 1, k) and n % 32
    rng = np.random.default_rng(71)
    emb, q = _small_ints(rng, (n, dim)), _small_ints(rng, (nq, dim))  # scores in a narrow integer range: many ties on every threshold
    exp = _numpy_rows(emb, q, k)
    assert (exp[2] == k).all()
    _assert_exact(_index(emb, dtype).search(q, k, fused=True), exp, f"{dtype} small integers")


GAUSSIAN = [(31, 3, 64, 1024), (100, 5, 64, 10),                                  # no sample: n < MIN_DOCS, one with k > n
            (65537, 1, 64, 1), (65600, 33, 1024, 100), (65700, 257, 192, 1024)]  # sampled; three query blocks at the largest k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,nq,dim,k", GAUSSIAN)
def test_word_for_word_with_the_matrix_route(dtype, n, nq, dim, k):
    from sparse_rx import _capi
    assert (_capi.half_fused_sample(n, k) > 0) == (n >= _capi.SRX_HALF_FUSED_MIN_DOCS)
    rng = np.random.default_rng(n + k)
    ix = _index(rng.standard_normal((n, dim), dtype=np.float32), dtype)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    exp = ix.search(q, k)
    _assert_exact(ix.search(q, k, fused=True), exp, f"{dtype} n={n} nq={nq} dim={dim} k={k}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_overflow_takes_the_fallback(dtype):
    from sparse_rx import _capi
    n, dim, k = _capi.SRX_HALF_FUSED_CAP + 200, 64, 10
    rng = np.random.default_rng(73)
    emb = _small_ints(rng, (n, dim))
    emb[:, 0] = 1.0
    q = np.clip(np.rint(rng.standard_normal((6, dim)) * 8) / 8, -3.875, 3.875).astype(np.float32)  # Gaussian on a grid of 1 / 8: still exact
    q[1], q[4] = 0.0, 0.0
    q[1, 0], q[4, 0] = 1.0, -1.0  # e0: every doc ties at 1.0, more survivors than a buffer holds; -e0: no result
    exp = _numpy_rows(emb, q, k)
    assert exp[0][1].tolist() == list(range(BASE, BASE + k)) and exp[2].tolist() == [k, k, k, k, 0, k]
    ix = _index(emb, dtype)
    first, again = ix.search(q, k, fused=True), ix.search(q, k, fused=True)
    _assert_exact(first, exp, f"{dtype} overflow")
    _assert_exact(again, first, f"{dtype} overflow, second run")  # the buffers fill in no fixed order; the result is fixed


@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_and_offset(dtype):
    import sparse_rx
    n, nq, dim, k = 66001, 12, 64, 100
    rng = np.random.default_rng(74)
    ix = _index(rng.standard_normal((n, dim), dtype=np.float32), dtype)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    masks = np.stack([np.ones(n, bool), rng.random(n) < 0.5, rng.random(n) < 0.01, np.zeros(n, bool)])
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    q_filter = np.array([(-1, 0, 1, 2, 3)[i % 5] for i in range(nq)], np.int32)
    for offset in (0.0, -6.0, 1000.0):  # fewer results than k for some rows; then every allowed doc ranks
        for kw in (dict(), dict(filter=flt, q_filter=q_filter), dict(filter=flt)):
            exp = ix.search(q, k, score_offset=offset, **kw)
            _assert_exact(ix.search(q, k, score_offset=offset, fused=True, **kw), exp, f"{dtype} offset={offset} {sorted(kw)}")
            if "q_filter" in kw:
                assert (exp[2][q_filter == 3] == 0).all() and (offset < 1000.0 or (exp[2][q_filter != 3] == k).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_second_pass_reads_its_own_filter_rows(dtype):
    import sparse_rx
    from sparse_rx import _capi
    n, nq, dim, k = 65600, _capi.SRX_HALF_FUSED_PASS + 1, 64, 10  # sampled; the second pass is one query, over a reused workspace
    rng = np.random.default_rng(76)
    ix = _index(rng.standard_normal((n, dim), dtype=np.float32), dtype)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.01, np.zeros(n, bool)])
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    q_filter = np.array([(-1, 0, 1, 2, 0)[i % 5] for i in range(nq)], np.int32)  # 1024 % 5 != 0: the passes start on different rows
    q_filter[-1] = 1  # the last query alone in its pass, on the sparse row: only docs of that row
    got, exp = ix.search(q, k, filter=flt, q_filter=q_filter, fused=True), ix.search(q, k, filter=flt, q_filter=q_filter)
    _assert_exact(got, exp, f"{dtype} two passes")
    assert exp[2][-1] == k and masks[1][exp[0][-1] - BASE].all() and (exp[2][q_filter == 2] == 0).all()


def test_service_keyword(golden_dir):
    import sparse_rx
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    queries = dict(j["queries"])
    rng = np.random.default_rng(75)
    emb = rng.standard_normal((len(j["corpus"]), 96)).astype(np.float32)
    vecs = {q: rng.standard_normal(96).astype(np.float32) for q in queries}
    got = []
    for fused in (False, True):
        svc = sparse_rx.RetrievalService(device="cuda:0", tile_log2=6)
        svc.build_bm25_index(j["corpus"])
        svc.set_embeddings(emb, storage="f16", fused=fused)
        assert svc._dense.fused is fused
        allowed = svc.doc_ids[::3]
        got.append(([svc.search_by_vector(v, k=7, allowed_docs=allowed) for v in vecs.values()],
                    svc.search_hybrid(queries, vecs, top_k=10, candidates=20, excluded_docs=allowed, rescore=True)))
        svc.close()
    assert got[0] == got[1] and any(got[1][0]) and any(got[1][1].values())
