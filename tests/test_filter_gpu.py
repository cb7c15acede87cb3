"""Filtered search on the GPU (include/sparse_rx_filter.h): sparse, dense f32 / uint8 and the API mirrors restricted to a
doc set.  Expected rows are never the engine's own: the oracle's UNFILTERED ranking at k = n_docs, filtered and cut by the
NumPy restatement (tests/filter_ref.py); the dense side derives its rows the way tests/test_dense_kernels.py does, with the
disallowed columns removed.  Every comparison is exact: ids, score bits, counts, padding.  The geometry and the corpus
recipes are those of tests/test_search_plans.py, built once per module."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import filter_ref  # noqa: E402
import hybrid_ref  # noqa: E402
import oracle  # noqa: E402  (checker only)
import parity  # noqa: E402
from test_gpu_parity import _assert_exact  # noqa: E402
from test_search_plans import CORPORA, TILE_LOG2, UNIT_TILES, _Env  # noqa: E402

pytestmark = pytest.mark.gpu

EDGE_DOCS = 20_011  # last filter word partial (20 011 = 625 * 32 + 11), last tile partial (19 * 1024 + 555)


class _FilterEnv(_Env):
    """The corpora and indexes of test_search_plans.py plus the edge corpus, and each batch's full unfiltered ranking."""

    def __init__(self):
        super().__init__()
        self.full = {}

    def full_ranking(self, name, nq, kind, seed):
        """(queries, the oracle's ranking of ALL docs with score > 0): computed once per batch, never modified."""
        key = (name, nq, kind, seed)
        if key not in self.full:
            q = self.queries(name, nq, kind, seed)
            rows = self.oracle(name, q, CORPORA[name][0])
            for a in rows:
                a.setflags(write=False)
            self.full[key] = (q, rows)
        return self.full[key]


CORPORA.setdefault("edge", (EDGE_DOCS, "uniform", 3_000, 30, 75, {}))


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()
    e = _FilterEnv()
    yield e
    for ix in e.indexes.values():
        ix.close()


def _masks(n_docs, densities, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.ones(n_docs, bool) if d >= 1 else np.zeros(n_docs, bool) if d <= 0 else rng.random(n_docs) < d for d in densities])


def _dev(ix, q):
    import torch
    return [torch.as_tensor(np.ascontiguousarray(x), device=ix.device) for x in q]


def _search_both(ix, q, k, flt, q_filter=None, after=None):
    """The same filtered batch through search_device and search_packed_device; host triples."""
    import torch
    dq = _dev(ix, q)
    qf = None if q_filter is None else torch.as_tensor(np.asarray(q_filter, np.int32), device=ix.device)
    d, s, c = ix.search_device(*dq, k, filter=flt, q_filter=qf, after=after)
    packed = ix.search_packed_device(*dq, k, filter=flt, q_filter=qf, after=after)
    torch.cuda.synchronize()
    rows = packed.cpu().numpy()
    return ((d.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy()),
            (rows[:, :k].copy(), rows[:, k:2 * k].copy().view(np.float32), rows[:, 2 * k].copy()))


def _check_filtered(env, name, nq, kind, seed, k, masks, q_filter, label, target=16, debug=0):
    """One filtered batch against the restatement; returns the expected rows."""
    import sparse_rx
    ix = env.index(name)
    base = CORPORA[name][5].get("doc_base", 0)
    q, full = env.full_ranking(name, nq, kind, seed)
    flt = sparse_rx.DocFilter.from_masks(masks, device=ix.device, doc_base=base)
    per_query = [masks[0]] * nq if q_filter is None else [None if r < 0 else masks[r] for r in q_filter]
    exp = filter_ref.filtered_rows(*full, per_query, base, k)
    ix.set_opts(target_blocks=target, debug=debug)
    try:
        rows, packed = _search_both(ix, q, k, flt, q_filter)
    finally:
        ix.set_opts()
    _assert_exact(rows, exp, f"{label} search_device")
    _assert_exact(packed, exp, f"{label} search_packed_device")
    return q, exp


# ---- 1. a mixed plan: 32 whole queries + a split tail, four rows of different density --------------------------------------
def test_mixed_plan_four_rows(env):
    name, nq, k = "uniform", 37, 100
    n = CORPORA[name][0]
    masks = _masks(n, [1.0, 0.0, 0.5, 0.01], seed=11)
    q_filter = np.array([(-1, 0, 1, 2, 3)[i % 5] for i in range(nq)], np.int32)
    q, exp = _check_filtered(env, name, nq, "u8", 2001, k, masks, q_filter, "mixed q_filter")
    sparse = exp[2][q_filter == 3]
    assert ((sparse > 0) & (sparse < k)).any(), "no density-0.01 query with a short list: the case does not test one"
    assert (exp[2][q_filter == 1] == 0).all()
    # q_filter = None: every query uses row 0 (all ones) -- the plain search's rows, and the oracle's at k
    ix = env.index(name)
    ix.set_opts(target_blocks=16)
    try:
        import torch
        _, exp0 = _check_filtered(env, name, nq, "u8", 2001, k, masks, None, "row 0 for all")
        plain = ix.search_device(*_dev(ix, q), k)
        torch.cuda.synchronize()
        plain = tuple(t.cpu().numpy() for t in plain)
    finally:
        ix.set_opts()
    _assert_exact(plain, exp0, "all-ones row vs the plain search")
    _assert_exact(exp0, env.oracle(name, q, k), "all-ones row vs the oracle at k")
    ones = np.flatnonzero((q_filter == 0) | (q_filter == -1))
    _assert_exact(tuple(a[ones] for a in exp), tuple(a[ones] for a in plain), "all-ones / unfiltered queries vs the plain rows")


# ---- 2. every candidate site: hash units, flat tiles, the wave-dense append scan, its masked and its general form -----------
@pytest.mark.parametrize("debug", [0, 128, 2048, 4096, 8192])
def test_every_candidate_site(env, debug):
    masks = _masks(CORPORA["zipf"][0], [0.5], seed=12)
    _check_filtered(env, "zipf", 37, "zipf8", 2002, 50, masks, None, f"zipf debug={debug}", debug=debug)


# ---- 3. more than 64 terms: the term-pass path ---------------------------------------------------------------------------------
def test_more_than_64_terms(env):
    masks = _masks(CORPORA["uniform"][0], [0.5, 0.05], seed=13)
    q_filter = np.arange(37) % 2
    _check_filtered(env, "uniform", 37, "long100", 2003, 100, masks, q_filter, "long100")


# ---- 4. layouts, with a doc_base: a filter indexed by global rows fails here ---------------------------------------------------
@pytest.mark.parametrize("name,nq,k,kind,target", [("dot16", 37, 100, "learned20", 16), ("dot16", 16, 1000, "learned20", 64),
                                                   ("compact", 36, 113, "u8", 16)])
def test_layouts_with_doc_base(env, name, nq, k, kind, target):
    assert CORPORA[name][5]["doc_base"] > 0
    masks = _masks(CORPORA[name][0], [0.5, 0.1], seed=14)
    q_filter = np.array([(0, 1, -1)[i % 3] for i in range(nq)], np.int32)
    _check_filtered(env, name, nq, kind, 2004 + k, k, masks, q_filter, f"{name} k={k}", target=target)


# ---- 5. bit and boundary edges ------------------------------------------------------------------------------------------------
def test_bit_and_boundary_edges(env):
    allowed = np.array([0, 31, 32, 1023, 1024, 4095, 4096, EDGE_DOCS - 1])
    only = np.zeros(EDGE_DOCS, bool)
    only[allowed] = True
    masks = np.stack([only, ~only])
    for kind, seed in (("u8", 2005), ("long100", 2006)):
        nq = 24
        q_filter = np.arange(nq) % 2
        _, exp = _check_filtered(env, "edge", nq, kind, seed, 100, masks, q_filter, f"edge {kind}", target=0)
        if kind == "long100":  # 100 of 3 000 terms: most docs match, so the eight allowed ones are really returned
            got = set(exp[0][q_filter == 0].ravel().tolist()) - {-1}
            assert got == set(allowed.tolist()), f"the oracle returns {sorted(got)} of the eight allowed docs"


# ---- 6. paging: k > 1024 under a filter -----------------------------------------------------------------------------------------
def test_paging_under_a_filter(env):
    import sparse_rx
    name, nq, k = "uniform", 37, 1500
    ix = env.index(name)
    q, full = env.full_ranking(name, nq, "u8", 2001)
    mask = _masks(CORPORA[name][0], [0.5], seed=16)[0]
    exp = filter_ref.filtered_rows(*full, mask, 0, k)
    assert (exp[2] > 1024).all(), f"every query needs more than one page of allowed rows, the oracle gives {exp[2].min()}"
    flt = sparse_rx.DocFilter.from_masks(mask, device=ix.device)
    ix.set_opts(target_blocks=16)
    try:
        got = ix.search(*q, k, filter=flt)
        two_rows = sparse_rx.DocFilter.from_masks(np.stack([~mask, mask]), device=ix.device)
        got2 = ix.search(*q, k, filter=two_rows, q_filter=np.ones(nq, np.int64))
    finally:
        ix.set_opts()
    _assert_exact(got, exp, "paged filtered search")
    _assert_exact(got2, exp, "paged filtered search, q_filter = row 1")
    with pytest.raises(ValueError):
        ix.search(*q, k, filter=two_rows, q_filter=np.full(nq, 2))
    with pytest.raises(ValueError):
        ix.search(*q, k, filter=sparse_rx.DocFilter.from_masks(mask[:-1], device=ix.device))


# ---- 7. the builders ------------------------------------------------------------------------------------------------------------
def test_builders():
    import torch
    import sparse_rx
    from sparse_rx import _capi
    n, base = 20_011, 5_000
    words = filter_ref.words(n)
    f1 = sparse_rx.DocFilter.filled(3, n, True, doc_base=base)
    bits = f1.bits.cpu().numpy().view(np.uint32)
    assert bits.shape == (3, words)
    exp = filter_ref.pack(np.ones(n, bool))
    assert (exp[n // 32] == (1 << (n % 32)) - 1) and not exp[n // 32 + 1:].any()  # the tail bits and the padding words are 0
    assert all(np.array_equal(bits[r], exp) for r in range(3))
    assert np.array_equal(f1.count(), [n, n, n])
    f0 = sparse_rx.DocFilter.filled(2, n, False, doc_base=base)
    assert not f0.bits.cpu().numpy().any() and np.array_equal(f0.count(), [0, 0])

    # set: duplicates, -1, ids of other shards (below doc_base, at and above doc_base + n); row 0 stays empty
    ids = np.array([base, base, base + 31, base + 32, -1, base - 1, 0, base + n, base + n - 1, base + 777, base + 777, 2 ** 31 - 1], np.int64)
    f0.set_docs(1, ids, True)
    mask = np.zeros(n, bool)
    mask[[0, 31, 32, n - 1, 777]] = True
    got = f0.bits.cpu().numpy().view(np.uint32)
    assert not got[0].any() and np.array_equal(got[1], filter_ref.pack(mask))
    assert np.array_equal(f0.count(), [0, 5])
    # ... a device block as a search returns it (padded with -1), then clear some of it again
    block = torch.tensor([[base + 100, base + 101, -1], [base + 31, -1, -1]], dtype=torch.int32, device=f0.device)
    f0.set_docs(1, block, True)
    f0.set_docs(1, [base + 31, base + 31, base + 5, base + n - 1], False)
    mask[[100, 101]] = True
    mask[[31, n - 1]] = False
    assert np.array_equal(f0.bits.cpu().numpy().view(np.uint32)[1], filter_ref.pack(mask))

    # allow / deny and the count against the restatement's popcount
    lists = [[base + 3, base + 64, base + n - 1], [], [base + 1]]
    fa = sparse_rx.DocFilter.allow(lists, n, doc_base=base)
    fd = sparse_rx.DocFilter.deny(lists, n, doc_base=base)
    for r, ids_r in enumerate(lists):
        m = np.zeros(n, bool)
        m[[i - base for i in ids_r]] = True
        assert np.array_equal(fa.bits.cpu().numpy().view(np.uint32)[r], filter_ref.pack(m))
        assert np.array_equal(fd.bits.cpu().numpy().view(np.uint32)[r], filter_ref.pack(~m))
    assert np.array_equal(fa.count(), [3, 0, 1]) and np.array_equal(fd.count(), [n - 3, n, n - 1])
    rnd = _masks(n, [0.3, 0.7], seed=17)
    fr = sparse_rx.DocFilter.from_masks(rnd, doc_base=base)
    assert np.array_equal(fr.count(), [filter_ref.popcount(filter_ref.pack(m), n) for m in rnd])
    # the count masks tail bits that are not docs, whatever they hold
    fr.bits.view(torch.int32)[0, n // 32] |= -(1 << (n % 32))
    assert fr.count()[0] == rnd[0].sum()
    assert _capi.lib().srx_version() == 301


# ---- 8. dense f32 and uint8 ---------------------------------------------------------------------------------------------------
DENSE_N, DENSE_DIM, DENSE_BASE = 32_801, 64, 1_000
DENSE_QF = np.array([1, -1, 0, 2, 1], np.int32)  # 5 queries: one more than a pass of 4, so q_filter is read at q0 + q


@pytest.fixture(scope="module")
def dense_data():
    rng = np.random.default_rng(21)
    emb = rng.standard_normal((DENSE_N, DENSE_DIM)).astype(np.float32)
    u8 = rng.integers(0, 256, (DENSE_N, DENSE_DIM), dtype=np.uint8)
    scale_min = np.stack([rng.uniform(0.001, 0.01, DENSE_N), rng.uniform(-1.0, -0.2, DENSE_N)], axis=1).astype(np.float32).reshape(-1)
    queries = rng.standard_normal((len(DENSE_QF), DENSE_DIM)).astype(np.float32)
    masks = _masks(DENSE_N, [0.5, 0.02, 0.9], seed=22)
    assert parity.dense_splits(DENSE_N, 4, 100) == 2, "the rank kernel should run 2 splits"
    return emb, u8, scale_min, queries, masks


def _dense_expected(sims, masks, k):
    s = sims.copy()
    for i, r in enumerate(DENSE_QF):
        if r >= 0:
            s[i, ~masks[r]] = 0.0  # a disallowed column is never a result: only scores > 0 are
    d, sc, c = parity.dense_topk_rows(s, k)
    return np.where(d >= 0, d + DENSE_BASE, d).astype(np.int32), sc, c


@pytest.mark.parametrize("k", [10, 100])
def test_dense_f32_filtered(dense_data, k):
    import sparse_rx
    emb, _, _, queries, masks = dense_data
    ix = sparse_rx.DenseF32Index(emb, doc_base=DENSE_BASE)
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=DENSE_BASE)
    for off in ((0.0, 2.5) if k == 10 else (0.0,)):
        exp = _dense_expected(parity.dense_rows_scores(emb, queries, score_offset=off), masks, k)
        _assert_exact(ix.search(queries, k, score_offset=off, filter=flt, q_filter=DENSE_QF), exp, f"dense f32 k={k} offset={off}")
    # q_filter = None: row 0 for every query
    sims = parity.dense_rows_scores(emb, queries)
    sims[:, ~masks[0]] = 0.0
    d, s, c = parity.dense_topk_rows(sims, k)
    _assert_exact(ix.search(queries, k, filter=flt), (np.where(d >= 0, d + DENSE_BASE, d).astype(np.int32), s, c), "dense f32 row 0")


@pytest.mark.parametrize("k", [10, 100])
def test_dense_u8_filtered(dense_data, k):
    import torch
    import sparse_rx
    _, u8, scale_min, queries, masks = dense_data
    ix = sparse_rx.DenseUint8Index(u8, scale_min, doc_base=DENSE_BASE)
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=DENSE_BASE)
    exp = _dense_expected(parity.dense_rows_scores(u8, queries, scale_min=scale_min), masks, k)
    qf = torch.as_tensor(DENSE_QF, device=ix.device)
    got = ix.search_device(torch.as_tensor(queries, device=ix.device), k, filter=flt, q_filter=qf)
    torch.cuda.synchronize()
    _assert_exact(tuple(t.cpu().numpy() for t in got), exp, f"dense u8 k={k}")


def test_dense_int8_refuses_a_filter(dense_data):
    import torch
    import sparse_rx
    emb, _, _, queries, masks = dense_data
    ix = sparse_rx.DenseInt8Index.from_embeddings(torch.as_tensor(emb[:2048], device="cuda:0"))
    flt = sparse_rx.DocFilter.from_masks(masks[:, :2048])
    q, qs, _ = sparse_rx.quantize_queries_symmetric_device(torch.as_tensor(queries, device="cuda:0"))
    with pytest.raises(ValueError, match="INT8"):
        ix.search_device(q, qs, 10, filter=flt)
    ix.search_device(q, qs, 10)  # the unfiltered call still runs
    torch.cuda.synchronize()


# ---- 9. the API mirrors on tests/golden/text_small.json ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "text_small.npz"))
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    qids = list(z["score_qids"])
    return j, {q: z["full_scores"][i] for i, q in enumerate(qids)}


def _assert_reference_ranking(got, exp, row, k, full, label):
    """A returned dict against the reference's dict: the golden floats to the bit, the docs equal up to the order inside a
    tie run (the reference's argsort does not order ties by doc id), as tests/test_gpu_parity.py compares them."""
    parity.assert_ranked_equal([row[d] for d in got], np.array(list(got.values()), np.float32), [row[d] for d in exp],
                               np.array(list(exp.values()), np.float32), k=k, full_scores=full, label=label)


def test_api_excluded_and_allowed_docs(golden):
    import sparse_rx
    j, full_scores = golden
    queries, ref = j["queries"], j["results"]["1000"]  # the reference's ranking of every doc with score > 0
    svc = sparse_rx.RetrievalService(device="cuda:0", tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    row = {d: i for i, d in enumerate(svc.doc_ids)}
    k = 10
    shown = {q: list(j["results"]["3"][q])[:3] for q in queries}  # "not the ones I already showed"
    assert any(len(v) == 3 for v in shown.values())
    got = svc.search_bm25(queries, top_k=k, excluded_docs=shown)
    assert list(got) == list(queries) and len(svc.query_cache) == 0
    for q in queries:
        exp = dict([(d, s) for d, s in ref[q].items() if d not in shown[q]][:k])
        full = None
        if q in full_scores:
            full = full_scores[q].copy()
            full[[row[d] for d in shown[q]]] = np.nan  # an excluded doc may not fill a boundary tie
        _assert_reference_ranking(got[q], exp, row, k, full, f"excluded {q}")
        assert not set(got[q]) & set(shown[q])
    # allowed_docs as a per-qid dict: every third doc for q0, the docs of q1's own top 3 for q1; the other qids unfiltered
    third = [d for i, d in enumerate(svc.doc_ids) if i % 3 == 0]
    allowed = {"q0": third, "q1": shown["q1"]}
    got = svc.search_bm25(queries, top_k=k, allowed_docs=allowed)
    for q in queries:
        keep = set(allowed[q]) if q in allowed else None
        exp = dict([(d, s) for d, s in ref[q].items() if keep is None or d in keep][:k])
        full = None
        if q in full_scores:
            full = full_scores[q].copy()
            if keep is not None:
                full[[i for d, i in row.items() if d not in keep]] = np.nan
        _assert_reference_ranking(got[q], exp, row, k, full, f"allowed {q}")
    assert list(got["q1"]) == shown["q1"]
    # one sequence for every query of the call; the registry mirror takes the same keywords
    got = svc.search_bm25(queries, top_k=k, excluded_docs=third)
    assert all(not set(got[q]) & set(third) for q in queries)
    r = sparse_rx.OptimizedBM25Retriever(device="cuda:0", tile_log2=6)
    r.build_index_from_corpus(j["corpus"])
    assert r.search(queries, top_k=k, excluded_docs=third) == got
    assert len(r.query_cache) == 0
    r.close()
    # nothing was cached by the filtered calls, and the next unfiltered call returns the golden result
    assert len(svc.query_cache) == 0
    plain = svc.search_bm25(queries, top_k=3)
    for q in queries:
        _assert_reference_ranking(plain[q], j["results"]["3"][q], row, 3, full_scores.get(q), f"golden after filtered calls {q}")
    n_cached = len(svc.query_cache)
    assert n_cached > 0
    svc.search_bm25(queries, top_k=3, excluded_docs=shown)
    assert len(svc.query_cache) == n_cached and svc.search_bm25(queries, top_k=3) == plain
    with pytest.raises(ValueError, match="not both"):
        svc.search_bm25(queries, allowed_docs=third, excluded_docs=third)
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.search_bm25(queries, excluded_docs=["doc0", "no-such-doc"])
    svc.close()


def test_api_hybrid_and_vector_with_a_filter(golden):
    import sparse_rx
    from test_hybrid_gpu import _assert_dicts, _rows_from_dicts
    j, _ = golden
    queries = dict(j["queries"])
    live = [q for q in queries if queries[q].strip()]  # a blank query is answered {} unsearched
    dim, n_docs = 96, len(j["corpus"])
    rng = np.random.default_rng(31)
    svc = sparse_rx.RetrievalService(device="cuda:0", tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    emb = rng.standard_normal((n_docs, dim)).astype(np.float32)
    svc.set_embeddings(emb)
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    row_of = {d: i for i, d in enumerate(svc.doc_ids)}
    half = [d for i, d in enumerate(svc.doc_ids) if i % 2 == 1]
    mask = np.zeros(n_docs, bool)
    mask[[row_of[d] for d in half]] = True
    flt = sparse_rx.DocFilter.from_masks(mask)
    for rescore in (False, True):
        k, c = 10, 20
        got = svc.search_hybrid(queries, vecs, top_k=k, candidates=c, allowed_docs=half, rescore=rescore)
        assert all(got[q] == {} for q in queries if q not in live)
        sparse = _rows_from_dicts(svc.search_bm25(queries, top_k=c, allowed_docs=half), live, row_of, c)
        dense = svc._dense.search(np.stack([vecs[q] for q in live]), c, filter=flt)
        assert all(set(got[q]) <= set(half) for q in live) and any(got[q] for q in live)
        if not rescore:
            _assert_dicts(got, live, hybrid_ref.fuse(sparse, dense, k, "weighted", (0.3, 0.7)), svc.doc_ids)
        else:
            import rescore_ref
            qa = sparse_rx.encode_queries([queries[q] for q in live], svc.host.vocabulary)
            a_other = svc._dense.score_docs(np.stack([vecs[q] for q in live]), sparse[0], sparse[2])
            b_other = svc.dev.score_docs(*qa, dense[0], dense[2])
            _assert_dicts(got, live, rescore_ref.fuse_scored(sparse, a_other, dense, b_other, k, (0.3, 0.7)), svc.doc_ids)
    # search_by_vector: the reference's np.dot ranking of the allowed rows
    q = vecs["q0"]
    got = svc.search_by_vector(q, k=5, excluded_docs=half)
    sims = parity.dense_rows_scores(np.pad(emb, ((0, 0), (0, 128 - dim))), np.pad(q, (0, 128 - dim))[None, :])[0]
    sims[mask] = 0.0
    d, s, c = parity.dense_topk_rows(sims[None, :], 5)
    assert [r["doc_id"] for r in got] == [svc.doc_ids[i] for i in d[0, : c[0]]]
    assert np.array_equal(np.array([r["score"] for r in got], np.float32).view(np.uint32), s[0, : c[0]].view(np.uint32))
    h = sparse_rx.HybridRetriever(embedding_dim=64, device="cuda:0", tile_log2=6)
    with pytest.raises(ValueError, match="INT8"):
        h.search(queries, allowed_docs=half)
    svc.close()
