"""Late-interaction search on the GPU (include/late/sparse_rx_maxsim_search.h), both half types.  Small-integer stores give
expected scores from float64 NumPy (every sum exact in any order), ranked by tests/late_search_ref.py and compared word for
word; on Gaussian rows the scores must be the bits of the existing scorer of given docs and lie within tests/late_ref.py's
bound of the fp64 score.  All comparisons are exact unless stated."""
import json
import os

import numpy as np
import pytest

import half_ref
import late_ref
import late_search_ref

pytestmark = pytest.mark.gpu
F = np.float32
TYPES = ["f16", "bf16"]
DEV = "cuda:0"


def _same(got, exp, label):
    for g, e, what in zip(got, exp, ("doc", "score", "count")):
        g, e = np.ascontiguousarray(g), np.ascontiguousarray(e)
        assert g.shape == e.shape and g.dtype == e.dtype, (label, what, g.shape, e.shape, g.dtype, e.dtype)
        bad = np.argwhere(g.view(np.uint32) != e.view(np.uint32))
        assert len(bad) == 0, f"{label}: {len(bad)} {what} words differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]!r} exp {e[tuple(bad[0])]!r}"


def _scores64(T, ptr, Q, q_cnt=None):
    """f64[nq, n_docs] from the definition: sum over the live query tokens of the largest dot product with a token of the doc"""
    out = np.zeros((len(Q), len(ptr) - 1))
    ne = np.flatnonzero(np.diff(ptr) > 0)  # a doc without tokens scores 0
    for q in range(len(Q)):
        live = late_ref.live_tokens(None if q_cnt is None else q_cnt[q], Q.shape[1])
        if live > 0 and len(ne):
            sim = Q[q, :live].astype(np.float64) @ T.astype(np.float64).T
            out[q, ne] = np.maximum.reduceat(sim, ptr[ne], axis=1).sum(axis=0)
    return out


def _store(counts, dim, seed, lo=-3, hi=4):
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return np.random.default_rng(seed).integers(lo, hi, (int(ptr[-1]), dim)).astype(F), ptr


def _index(T, ptr, dtype, doc_base=0):
    import sparse_rx
    return sparse_rx.TokenIndex.from_token_embeddings(T, np.diff(ptr), dtype=dtype, device=DEV, doc_base=doc_base)


# (dim, tq): NAB 1 / 2 / 4 and the LDS-limited group sizes, then the instances (NAB, QG) = (1, 2), (2, 1), (3, 1)
SHAPES = [(64, 1), (64, 32), (128, 33), (256, 128), (1024, 32), (512, 32), (512, 64), (320, 96)]


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("dim,tq", SHAPES)
def test_exact_integers(dtype, dim, tq):
    rng = np.random.default_rng(dim + tq)
    T, ptr = _store(rng.integers(0, 70, 150), dim, seed=dim)
    ix = _index(T, ptr, dtype)
    for nq in (1, 5, 33):  # one query, a partial group, more than one group
        Q = rng.integers(-3, 4, (nq, tq, dim)).astype(F)
        q_cnt = None if nq == 1 else rng.integers(0, tq + 1, nq).astype(np.int32)
        exp = _scores64(T, ptr, Q, q_cnt)
        assert np.abs(exp).max() < 2 ** 24
        _same(ix.search(Q, q_cnt, 20), late_search_ref.expected(exp.astype(F), None, 20), f"{dtype} dim {dim} tq {tq} nq {nq}")
    ix.close()


# docs without tokens first, last and in a run; 1-token docs; 31 .. 65 tokens; a doc that ends at a block end (row 256); one
# longer than a workgroup's range (4 waves x 4 blocks x 32 rows); n_tok = 1201: three workgroups
EDGE_COUNTS = [0, 3, 0, 0, 0, 1, 1, 1, 1, 1, 31, 32, 33, 64, 65, 23, 900, 5, 40, 0]


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("negative", [False, True])
def test_doc_boundaries(dtype, negative):
    T, ptr = _store(EDGE_COUNTS, 64, seed=3, **(dict(lo=1, hi=4) if negative else {}))
    assert ptr[16] == 256 and ptr[-1] % 32 != 0 and ptr[-1] > 2 * 512
    rng = np.random.default_rng(4)
    Q = (rng.integers(-3, 0, (3, 5, 64)) if negative else rng.integers(-3, 4, (3, 5, 64))).astype(F)
    exp = _scores64(T, ptr, Q)
    n = len(EDGE_COUNTS)
    got = _index(T, ptr, dtype).search(Q, None, n)
    _same(got, late_search_ref.expected(exp.astype(F), None, n), f"{dtype} negative={negative}")
    if negative:  # the docs without tokens score +0.0f and outrank every other doc
        assert (exp[:, np.diff(ptr) > 0] < 0).all() and got[0][0, :5].tolist() == [0, 2, 3, 4, n - 1] and not got[1][0, :5].view(np.uint32).any()


@pytest.mark.parametrize("dtype", TYPES)
def test_bits_of_the_existing_scorer_and_fp64_bound(dtype):
    rng = np.random.default_rng(8)
    counts = rng.integers(0, 40, 120)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    T = rng.standard_normal((int(ptr[-1]), 96)).astype(F)  # dim 96: padded to 128
    ix = _index(T, ptr, dtype)
    nq, tq = 3, 33
    Q, q_cnt = rng.standard_normal((nq, tq, 96)).astype(F), np.array([33, 32, 7], np.int32)
    scores = ix.score_docs(Q, q_cnt, np.tile(np.arange(ix.n_docs, dtype=np.int32), (nq, 1)))
    got = ix.search(Q, q_cnt, ix.n_docs)
    _same(got, late_search_ref.expected(scores, None, ix.n_docs), f"against score_docs over all docs, {dtype}")
    codes = np.zeros((len(T), ix.dim_pad), np.uint16)
    codes[:, :96] = half_ref.round_codes(T, dtype)
    for q in range(nq):
        qc = np.zeros((tq, ix.dim_pad), np.uint16)
        qc[:, :96] = half_ref.round_codes(Q[q], dtype)
        for j in range(ix.n_docs):
            dc = codes[ptr[got[0][q, j]]: ptr[got[0][q, j] + 1]]
            ref, bound = late_ref.score_f64(qc, dc, dtype, int(q_cnt[q])), late_ref.tol(qc, dc, dtype, int(q_cnt[q]))
            assert abs(float(got[1][q, j]) - ref) <= bound, (dtype, q, j, float(got[1][q, j]), ref, bound)


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("n_docs", [1, 1024, 1025, 5000, 20000])  # above 8 192 docs a score row is split over workgroups and merged
def test_selection_edges(dtype, n_docs):
    """1-token docs drawn from 40 distinct rows: many identical docs, so ties break by doc ascending; doc_base > 0; two filter
    rows, one of which allows fewer docs than k"""
    import sparse_rx
    import torch
    rng = np.random.default_rng(n_docs)
    rows = rng.integers(-3, 4, (40, 64)).astype(F)
    T, ptr = rows[rng.integers(0, 40, n_docs)], np.arange(n_docs + 1, dtype=np.int64)
    ix = _index(T, ptr, dtype, doc_base=7)
    Q = rng.integers(-3, 4, (4, 3, 64)).astype(F)
    exp = _scores64(T, ptr, Q).astype(F)
    masks = np.stack([rng.random(n_docs) < 0.5, np.arange(n_docs) % 97 == 0])
    flt = sparse_rx.DocFilter.from_masks(masks, device=DEV, doc_base=7)
    q_filter = np.array([0, 1, -1, 1], np.int32)
    allowed = np.stack([masks[r] if r >= 0 else np.ones(n_docs, bool) for r in q_filter])
    for k in (1, 10, 1024):
        _same(ix.search(Q, None, k), late_search_ref.expected(exp, None, k, doc_base=7), f"{dtype} n_docs {n_docs} k {k}")
        got = ix.search(Q, None, k, filter=flt, q_filter=q_filter)
        _same(got, late_search_ref.expected(exp, allowed, k, doc_base=7), f"{dtype} n_docs {n_docs} k {k} filtered")
        assert got[2].tolist() == [min(k, int(a.sum())) for a in allowed]
    if n_docs == 20000:  # the minimum workspace (three passes of one group, one workgroup per row) gives the words of the preferred one
        Q9 = rng.integers(-3, 4, (9, 3, 64)).astype(F)
        qg, lo, hi = sparse_rx.late_search_plan(9, 3, 64, n_docs, 10)
        assert qg == 4 and lo + 4 * n_docs * 4 < hi
        few = [t.cpu().numpy() for t in ix.search_device(torch.as_tensor(Q9, device=DEV), None, 10, workspace_bytes=lo)]
        _same(few, ix.search(Q9, None, 10), f"{dtype} passes")
        _same(few, late_search_ref.expected(_scores64(T, ptr, Q9).astype(F), None, 10, doc_base=7), f"{dtype} minimum workspace")


@pytest.mark.parametrize("dtype", TYPES)
def test_filter_rows_and_batch_independence(dtype):
    import sparse_rx
    rng = np.random.default_rng(12)
    T, ptr = _store(rng.integers(0, 50, 300), 128, seed=13)
    ix = _index(T, ptr, dtype)
    Q = rng.integers(-3, 4, (33, 33, 128)).astype(F)
    q_cnt = rng.integers(0, 34, 33).astype(np.int32)
    exp = _scores64(T, ptr, Q, q_cnt).astype(F)
    masks = np.stack([rng.random(300) < 0.3, np.zeros(300, bool), np.arange(300) == 123])  # some docs, nothing, one doc
    q_filter = (np.arange(33) % 4 - 1).astype(np.int32)
    allowed = np.stack([masks[r] if r >= 0 else np.ones(300, bool) for r in q_filter])
    flt = sparse_rx.DocFilter.from_masks(masks, device=DEV)
    got = ix.search(Q, q_cnt, 25, filter=flt, q_filter=q_filter)
    _same(got, late_search_ref.expected(exp, allowed, 25), f"{dtype} filter rows")
    _same(ix.search(Q, q_cnt, 25, filter=flt), late_search_ref.expected(exp, np.tile(masks[0], (33, 1)), 25), f"{dtype} row 0 for every query")
    for q in (0, 17, 32):  # a query's row is the same alone as inside the batch of 33
        alone = ix.search(Q[q: q + 1], q_cnt[q: q + 1], 25, filter=flt, q_filter=q_filter[q: q + 1])
        _same(alone, [t[q: q + 1] for t in got], f"{dtype} query {q} alone")


@pytest.mark.parametrize("storage", TYPES)
def test_service(golden_dir, storage):
    import sparse_rx
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    rng = np.random.default_rng(71)
    svc = sparse_rx.RetrievalService(device=DEV, tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    ids = svc.doc_ids
    assert len(ids) <= 1024  # rerank_late can take every doc as one list
    tok = {d: rng.integers(-3, 4, (0 if i % 11 == 0 else int(rng.integers(1, 40)), 40)).astype(F) for i, d in enumerate(ids)}
    q_tok = {q: rng.integers(-3, 4, (int(rng.integers(1, 34)), 40)).astype(F) for q in j["queries"]}
    with pytest.raises(ValueError, match="No token index"):
        svc.search_late(q_tok)
    svc.set_token_embeddings(tok, storage=storage)
    everything = {q: {d: 0.0 for d in ids} for q in q_tok}
    assert svc.search_late(q_tok, top_k=10) == svc.rerank_late(everything, q_tok, top_k=10)
    some = ids[::3]
    assert svc.search_late(q_tok, top_k=10, allowed_docs=some) == svc.rerank_late({q: {d: 0.0 for d in some} for q in q_tok}, q_tok, top_k=10)
    having = [d for d in ids if "w3" in j["corpus"][d].get("text", "").split()]  # the index reads the text, never the title
    got = svc.search_late(q_tok, top_k=10, must_terms=["w3"])
    assert got == svc.rerank_late({q: {d: 0.0 for d in having} for q in q_tok}, q_tok, top_k=10) and all(got.values())
    svc.close()
