"""srx_dense_search_f32_batched on the GPU (include/batched/sparse_rx_f32_batched.h): word for word the rows of srx_dense_search_f32 /
_filtered, and on integer operands (every product and sum exact) the rows of a float64 NumPy ranking.  The shapes sit at the edges
of the kernel's tile (128 x 128, chunks of 32 columns), of a pass (1024 queries) and of the header's sample rule."""
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
from sparse_rx import _capi  # noqa: E402
from test_gpu_parity import _assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu
BIG = _capi.SRX_F32_BATCHED_MIN_DOCS + 77  # the smallest corpus with a sample, plus a ragged tail
# n_docs, nq, dim, k, keywords: offset, base, and "filter" (one row for all) / "q_filter" (rows by query, some unfiltered)
SHAPES = [(1, 1, 64, 1, {}), (31, 33, 100, 10, {}), (129, 129, 192, 1024, {}), (1000, 1025, 64, 10, {}), (1000, 33, 1024, 1024, {}),
          (BIG, 129, 192, 10, {}), (BIG, 33, 1024, 1024, {}), (BIG, 1, 100, 1, {}),
          (BIG, 33, 64, 10, dict(filter=True)), (BIG, 33, 64, 10, dict(q_filter=True)), (BIG, 33, 64, 10, dict(offset=-40.0)),
          (BIG, 33, 64, 10, dict(offset=1048576.0)), (BIG, 33, 64, 10, dict(base=3_000_000))]
IDS = [f"n{n}-nq{nq}-d{dim}-k{k}-{'-'.join(kw) or 'plain'}" for n, nq, dim, k, kw in SHAPES]


def _case(emb, q, kw):
    """The index, the search keywords and the allowed-doc mask per query (None: all) of a case"""
    import torch
    import sparse_rx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    n, nq, base = emb.shape[0], q.shape[0], kw.get("base", 0)
    ix = sparse_rx.DenseF32Index(torch.as_tensor(emb, device="cuda:0"), doc_base=base)
    search, allowed = dict(score_offset=kw.get("offset", 0.0)), None
    if "filter" in kw or "q_filter" in kw:
        rng = np.random.default_rng(5)
        masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.01])
        search["filter"] = sparse_rx.DocFilter.from_masks(masks, doc_base=base)
        rows = np.zeros(nq, np.int32)
        if "q_filter" in kw:
            rows = np.array([(-1, 0, 1)[i % 3] for i in range(nq)], np.int32)
            search["q_filter"] = rows
        allowed = np.where((rows >= 0)[:, None], masks[np.maximum(rows, 0)], True)
    return ix, search, allowed


@pytest.mark.parametrize("n,nq,dim,k,kw", SHAPES, ids=IDS)
def test_integer_rows_match_a_float64_ranking(n, nq, dim, k, kw):
    rng = np.random.default_rng(n + nq + dim + k)
    emb, q = (rng.integers(-8, 9, s).astype(np.float32) for s in ((n, dim), (nq, dim)))  # narrow integer scores: ties on every threshold
    ix, search, allowed = _case(emb, q, kw)
    S = (q.astype(np.float64) @ emb.astype(np.float64).T).astype(np.float32) + np.float32(search["score_offset"])
    if allowed is not None:
        S[~allowed] = 0.0
    d, s, c = parity.dense_topk_rows(S, k)
    exp = (np.where(d >= 0, d + kw.get("base", 0), d).astype(np.int32), s, c)
    _assert_exact(ix.search(q, k, batched=True, **search), exp, "integers")


@pytest.mark.parametrize("n,nq,dim,k,kw", SHAPES, ids=IDS)
def test_gaussian_rows_match_the_matvec_route(n, nq, dim, k, kw):
    rng = np.random.default_rng(n + nq + dim + k + 1)
    emb, q = rng.standard_normal((n, dim), dtype=np.float32), rng.standard_normal((nq, dim), dtype=np.float32)
    ix, search, _ = _case(emb, q, {**kw, **({"offset": kw["offset"] / 8} if "offset" in kw else {})})
    _assert_exact(ix.search(q, k, batched=True, **search), ix.search(q, k, **search), "gaussian")


@pytest.mark.parametrize("k", [10, 1024])
def test_scores_within_ulps_of_the_threshold(k):
    """Every row is one vector plus noise of a few ulps: thousands of scores sit within the GEMM's rounding of tau."""
    rng = np.random.default_rng(k)
    base = rng.standard_normal(192, dtype=np.float32)
    emb = (base[None, :].view(np.int32) + rng.integers(-3, 4, (BIG, 192), dtype=np.int32)).view(np.float32)
    q = np.concatenate([base[None, :], rng.standard_normal((4, 192), dtype=np.float32)])
    ix, search, _ = _case(emb, q, {})
    _assert_exact(ix.search(q, k, batched=True), ix.search(q, k), "margin")


@pytest.mark.parametrize("starved", [False, True], ids=["all-tied", "filter-starved"])
def test_overflow_takes_the_fallback(starved):
    import sparse_rx
    n, dim, k = _capi.SRX_F32_BATCHED_CAP + 4500, 64, 10
    S = _capi.f32_batched_sample(n, k)
    assert S == 4096
    rng = np.random.default_rng(9)
    emb = np.tile(rng.standard_normal(dim, dtype=np.float32), (n, 1))  # more identical rows than a candidate buffer holds
    q = rng.standard_normal((3, dim), dtype=np.float32)
    q[0], q[2] = emb[0], -emb[0]  # every doc ties above zero; a Gaussian query; no result
    ix, search, _ = _case(emb, q, {})
    if starved:  # fewer than k docs of the sample are allowed, more than a buffer holds overall
        mask = np.arange(n) >= S - 5
        assert mask[:S].sum() < k and mask.sum() > _capi.SRX_F32_BATCHED_CAP
        search["filter"] = sparse_rx.DocFilter.from_masks(mask[None, :], doc_base=0)
    exp = ix.search(q, k, **search)
    assert exp[2].tolist()[::2] == [k, 0] and exp[0][0].tolist() == list(range(S - 5 if starved else 0, (S - 5 if starved else 0) + k))
    first, again = ix.search(q, k, batched=True, **search), ix.search(q, k, batched=True, **search)
    _assert_exact(first, exp, "overflow")
    _assert_exact(again, first, "overflow, second run")  # the buffers fill in no fixed order; the result is fixed


def test_service_keyword(golden_dir):
    import sparse_rx
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    queries = dict(j["queries"])
    rng = np.random.default_rng(75)
    emb = rng.standard_normal((len(j["corpus"]), 96)).astype(np.float32)
    vecs = {q: rng.standard_normal(96).astype(np.float32) for q in queries}
    got = []
    for batched in (False, True):
        svc = sparse_rx.RetrievalService(device="cuda:0", tile_log2=6)
        svc.build_bm25_index(j["corpus"])
        svc.set_embeddings(emb, storage="f32", batched=batched)
        assert svc._dense.batched is batched
        allowed = svc.doc_ids[::3]
        got.append(([svc.search_by_vector(v, k=7, allowed_docs=allowed) for v in vecs.values()], [svc.search_by_vector(v, k=7) for v in vecs.values()],
                    svc.search_hybrid(queries, vecs, top_k=10, candidates=20, excluded_docs=allowed, rescore=True)))
        svc.close()
    assert got[0] == got[1] and any(got[1][0]) and any(got[1][1]) and any(got[1][2].values())
