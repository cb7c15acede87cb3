"""Late-interaction reranking on the GPU (include/sparse_rx_maxsim.h), both half types.  Two yardsticks: small-integer token and
query values (exact in f16 and bf16, every product and partial sum below 2^24) give expected scores from integer NumPy that
use no engine code at all and are compared bit for bit; on random floats the similarities come from the existing scorer of
given docs (``TokenIndex.tokens.score_docs_device``, pinned by its own tests), tests/late_ref.py's max / ordered sum is
applied to them and the bits must match -- and lie within the derived fp64 bound, so that test is not only a comparison
of two engine paths.  All comparisons are exact unless stated; no case is excluded from any comparison."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import half_ref  # noqa: E402
import late_ref  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
TYPES = ["f16", "bf16"]
N_DOCS = 3001
SPECIAL_COUNTS = [0, 1, 31, 32, 33, 64, 65, 200]
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _same(got, exp, label):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (label, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(_bits(got) != _bits(exp))
    assert len(bad) == 0, f"{label}: {len(bad)} words differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r} exp {exp[tuple(bad[0])]!r}"


# ---- the integer stores: built once per (dim, sign), shared, never modified -------------------------------------------------------
def _counts():
    """Token counts of N_DOCS docs: every special count several times, small random counts between them (so docs start at every
    row offset mod 32), and the last doc ends inside the last tile."""
    rng = np.random.default_rng(5)
    c = rng.integers(1, 10, N_DOCS)
    for i, j in enumerate(range(0, N_DOCS - 8, 37)):
        c[j] = SPECIAL_COUNTS[i % len(SPECIAL_COUNTS)]
    for j in range(10, N_DOCS - 8, 50):  # a twin: doc j + 1 gets the token rows of doc j
        c[j + 1] = c[j]
    if int(c.sum()) % 32 == 0:
        c[-1] += 1
    return c.astype(np.int64)


_STORES = {}


def _int_store(dim, negative=False):
    """(token rows int8[n_tok, dim], tok_ptr int64[N_DOCS + 1]): values in [-3, 3] (negative: in [1, 3], for queries in [-3, -1])"""
    key = (dim, negative)
    if key not in _STORES:
        counts = _counts()
        ptr = np.concatenate([[0], np.cumsum(counts)])
        rng = np.random.default_rng(1000 + dim)
        T = rng.integers(1, 4, (int(ptr[-1]), dim), dtype=np.int8) if negative else rng.integers(-3, 4, (int(ptr[-1]), dim), dtype=np.int8)
        for j in range(10, N_DOCS - 8, 50):
            T[ptr[j + 1]: ptr[j + 2]] = T[ptr[j]: ptr[j + 1]]
        offs = set((ptr[:-1] % 32).tolist())
        assert offs == set(range(32)) and ptr[-1] % 32 != 0 and set(SPECIAL_COUNTS) <= set(counts.tolist())
        _STORES[key] = (T, ptr)
    return _STORES[key]


_INDEXES = {}


def _index(dtype, dim, negative=False, doc_base=0):
    import sparse_rx
    key = (dtype, dim, negative)
    if key not in _INDEXES:
        if len(_INDEXES) >= 4:  # keep the resident stores few
            _INDEXES.pop(next(iter(_INDEXES))).close()
        T, ptr = _int_store(dim, negative)
        _INDEXES[key] = sparse_rx.TokenIndex.from_token_embeddings(T.astype(F), np.diff(ptr), dtype=dtype, device=DEV)
    ix = _INDEXES[key]
    return ix if doc_base == 0 else sparse_rx.TokenIndex(ix.tokens, ix.tok_ptr.cpu().numpy(), doc_base=doc_base)


def _special_docs():
    c = _counts()
    return list(dict.fromkeys([int(np.flatnonzero(c == s)[0]) for s in SPECIAL_COUNTS] + [N_DOCS - 1, 0, 10, 11]))  # each doc once


class _Exact:
    """Expected scores from integer NumPy, one (query, doc) pair at a time, remembered"""

    def __init__(self, T, ptr, Q, q_cnt):
        self.T, self.ptr, self.Q, self.memo = T, ptr, Q, {}
        self.live = [late_ref.live_tokens(None if q_cnt is None else q_cnt[q], Q.shape[1]) for q in range(len(Q))]

    def pair(self, q, d):
        if (q, d) not in self.memo:
            rows = self.T[self.ptr[d]: self.ptr[d + 1]].astype(np.int64)
            s = 0
            if len(rows) and self.live[q] > 0:
                s = int((self.Q[q, : self.live[q]] @ rows.T).max(axis=1).sum())
                assert abs(s) < 2 ** 24
            self.memo[(q, d)] = F(s)
        return self.memo[(q, d)]

    def scores(self, cand, cand_count, doc_base=0):
        out = np.zeros(cand.shape, F)
        for q in range(cand.shape[0]):
            live = late_ref.live_positions(cand[q], None if cand_count is None else cand_count[q], doc_base, N_DOCS)
            for c in np.flatnonzero(live):
                out[q, c] = self.pair(q, int(cand[q, c]) - doc_base)
        return out

    def ranked(self, cand, cand_count, k, doc_base=0):
        s = self.scores(cand, cand_count, doc_base)
        d, sc, n = np.full((len(cand), k), -1, np.int32), np.zeros((len(cand), k), F), np.zeros(len(cand), np.int32)
        for q in range(len(cand)):
            live = late_ref.live_positions(cand[q], None if cand_count is None else cand_count[q], doc_base, N_DOCS)
            d[q], sc[q], n[q] = late_ref.rank(cand[q], s[q], live, k)
        return d, sc, n


def _queries(nq, tq, dim, seed, negative=False):
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 0, (nq, tq, dim)) if negative else rng.integers(-3, 4, (nq, tq, dim))


def _cands(nq, m, seed, distinct=False):
    rng = np.random.default_rng(seed)
    sp = _special_docs()
    out = np.zeros((nq, m), np.int32)
    for q in range(nq):
        if distinct:
            rest = rng.permutation(np.setdiff1d(np.arange(N_DOCS), sp))[: max(0, m - len(sp))]
            row = rng.permutation(np.concatenate([sp, rest]).astype(np.int64))[:m] if m >= len(sp) else np.asarray(sp[:m])
        else:
            row = rng.integers(0, N_DOCS, m)
            row[: min(m, len(sp))] = sp[: min(m, len(sp))]
        out[q] = row
    return out


# ---- 1. exact integers, independent of any engine code ---------------------------------------------------------------------------
SHAPES = [(48, 1), (48, 31), (48, 32), (48, 33), (128, 1), (128, 31), (128, 32), (128, 33), (1024, 1), (1024, 31), (1024, 32),
          (500, 64), (256, 128)]


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("dim,tq", SHAPES)
def test_exact_integers(dtype, dim, tq):
    ix = _index(dtype, dim)
    assert ix.n_docs == N_DOCS and ix.dim_pad == (dim + 63) // 64 * 64 and late_ref.shape_ok(tq, ix.dim_pad)
    T, ptr = _int_store(dim)
    assert ix.n_tokens == int(ptr[-1]) and ix.device_bytes() >= ix.n_tokens * ix.dim_pad * 2
    nq, m = 3, 40
    Q = _queries(nq, tq, dim, 7 * dim + tq)
    q_cnt = np.array([tq, max(tq - 1, 0), min(tq, 5)], np.int32)
    cand = _cands(nq, m, dim + tq)
    ex = _Exact(T, ptr, Q, q_cnt)
    _same(ix.score_docs(Q.astype(F), q_cnt, cand), ex.scores(cand, None), f"scores {dtype} dim {dim} tq {tq}")
    ex_all = _Exact(T, ptr, Q, None)
    _same(ix.score_docs(Q.astype(F), None, cand), ex_all.scores(cand, None), f"scores, NULL token counts, {dtype} dim {dim} tq {tq}")


@pytest.mark.parametrize("dtype", TYPES)
def test_every_similarity_negative(dtype):
    dim, tq, nq, m = 128, 33, 3, 48
    ix = _index(dtype, dim, negative=True)
    T, ptr = _int_store(dim, negative=True)
    Q = _queries(nq, tq, dim, 3, negative=True)
    assert (Q[:, :, None, :] * T[None, None, :50, :].astype(np.int64)).sum(-1).max() < 0
    cand = _cands(nq, m, 11)
    ex = _Exact(T, ptr, Q, None)
    exp = ex.scores(cand, None)
    got = ix.score_docs(Q.astype(F), None, cand)
    _same(got, exp, "all-negative scores")
    counts = np.diff(ptr)[cand]
    assert (got[counts > 0] < 0).all() and (_bits(got[counts == 0]) == 0).all() and (counts == 0).any()
    # the rerank keeps negative scores, and zero-token docs (+0) rank in front of them
    cand = _cands(nq, m, 12, distinct=True)
    k = m
    got = ix.rerank(Q.astype(F), None, cand, None, k)
    exp = ex.ranked(cand, None, k)
    for g, e, what in zip(got, exp, ("doc", "score", "count")):
        _same(g, e, f"all-negative rerank {what}")
    assert (np.diff(ptr)[got[0][:, 0]] == 0).all() and (got[1][:, -1] < 0).all() and (got[2] == m).all()


# ---- 2. bit-equality with the existing scorer on random floats -------------------------------------------------------------------
_FLOAT = {}


def _float_index(dtype):
    import sparse_rx
    if dtype not in _FLOAT:
        rng = np.random.default_rng(21)
        n_docs, dim = 300, 96
        counts = rng.integers(0, 45, n_docs)
        counts[:8] = SPECIAL_COUNTS
        tok = rng.standard_normal((int(counts.sum()), dim)).astype(F)
        ix = sparse_rx.TokenIndex.from_token_embeddings(tok, counts, dtype=dtype, device=DEV)
        _FLOAT[dtype] = (ix, np.concatenate([[0], np.cumsum(counts)]), ix.tokens.corpus_to_host())
    return _FLOAT[dtype]


def _sim_from_scorer(ix, q_tok_q, rows):
    """sim f32[tq, len(rows)] of one query's tokens against token rows, from the EXISTING scorer of given docs"""
    import torch
    tq = len(q_tok_q)
    cd = torch.as_tensor(np.tile(np.asarray(rows, np.int32), (tq, 1)), device=DEV)
    return ix.tokens.score_docs_device(torch.as_tensor(q_tok_q, device=DEV), cd).cpu().numpy()


def _expected_float(ix, ptr, q_tok, q_cnt, cand):
    nq, m = cand.shape
    exp = np.zeros((nq, m), F)
    for q in range(nq):
        docs = sorted({int(d) for d in cand[q] if 0 <= d < ix.n_docs})
        rows = np.concatenate([np.arange(ptr[d], ptr[d + 1]) for d in docs] + [np.zeros(0, np.int64)])
        sim = _sim_from_scorer(ix, q_tok[q], rows) if len(rows) else np.zeros((q_tok.shape[1], 0), F)
        at, o = {}, 0
        for d in docs:
            at[d] = (o, o + int(ptr[d + 1] - ptr[d]))
            o = at[d][1]
        n_live = late_ref.live_tokens(None if q_cnt is None else q_cnt[q], q_tok.shape[1])
        for c in range(m):
            if int(cand[q, c]) in at:
                lo, hi = at[int(cand[q, c])]
                exp[q, c] = late_ref.score_from_sim(sim[:, lo:hi], n_live)
    return exp


@pytest.mark.parametrize("dtype", TYPES)
def test_bits_of_the_existing_scorer_and_fp64_bound(dtype):
    ix, ptr, codes = _float_index(dtype)
    rng = np.random.default_rng(22)
    nq, tq, m = 3, 33, 24
    q_tok = rng.standard_normal((nq, tq, ix.dim)).astype(F)
    q_cnt = np.array([33, 32, 7], np.int32)
    cand = rng.integers(0, ix.n_docs, (nq, m)).astype(np.int32)
    cand[:, :8] = np.arange(8)
    got = ix.score_docs(q_tok, q_cnt, cand)
    _same(got, _expected_float(ix, ptr, q_tok, q_cnt, cand), f"scores against the scorer of given docs, {dtype}")
    pad = np.zeros((codes.shape[0], ix.dim_pad), np.uint16)
    pad[:, : ix.dim] = codes
    worst = 0.0
    for q in range(nq):
        qc = np.zeros((tq, ix.dim_pad), np.uint16)
        qc[:, : ix.dim] = half_ref.round_codes(q_tok[q], dtype)
        for c in range(m):
            d = int(cand[q, c])
            dc = pad[ptr[d]: ptr[d + 1]]
            ref, bound = late_ref.score_f64(qc, dc, dtype, int(q_cnt[q])), late_ref.tol(qc, dc, dtype, int(q_cnt[q]))
            err = abs(float(got[q, c]) - ref)
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
            assert err <= bound, (dtype, q, c, d, float(got[q, c]), ref, bound)
    print(f"{dtype}: worst |score - fp64| / bound = {worst:.4f}")


# ---- 3. candidate-list edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("m", [1, 64, 65, 1024])
def test_candidate_list_edges(dtype, m):
    dim, tq, nq, base = 48, 9, 4, 7
    ix = _index(dtype, dim, doc_base=base)
    assert ix.doc_base == base
    T, ptr = _int_store(dim)
    Q = _queries(nq, tq, dim, 31 + m)
    ex = _Exact(T, ptr, Q, None)
    cand = _cands(nq, m, 32 + m) + base
    if m >= 64:
        cand[0, 3], cand[0, 5], cand[1, 9] = -1, base - 1, base + N_DOCS        # padding, just below the base, just past the end
        cand[1, 11], cand[2, 1] = base + N_DOCS - 1, cand[2, 0]                 # the last doc; a duplicate
        cand[3, 20:30] = cand[3, 19]                                              # a run of duplicates
        cand[0, 40], cand[0, 41] = 2 ** 31 - 1, -(2 ** 31)
    else:
        cand[1, 0], cand[2, 0], cand[3, 0] = -1, base - 1, base + N_DOCS
    for counts in (None, np.array([m, 0, m // 2, m + 5], np.int32), np.array([-3, 1, m, m - 1], np.int32)):
        _same(ix.score_docs(Q.astype(F), None, cand, counts), ex.scores(cand, counts, base), f"edges {dtype} m {m} counts {counts}")


# ---- 4. invariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
def test_bits_do_not_depend_on_the_batch(dtype):
    ix, ptr, _ = _float_index(dtype)
    rng = np.random.default_rng(41)
    tq, m = 20, 16
    q0 = rng.standard_normal((tq, ix.dim)).astype(F)
    docs = rng.permutation(ix.n_docs)[:m].astype(np.int32)
    base = ix.score_docs(q0[None], np.array([17], np.int32), docs[None])[0]                  # nq 1, the list as it is
    assert len(set(_bits(base).tolist())) > m // 2
    for nq, at, m2 in ((5, 3, 40), (70, 69, 65)):
        q_tok = rng.standard_normal((nq, tq, ix.dim)).astype(F)
        q_tok[at] = q0
        q_cnt = rng.integers(0, tq + 1, nq).astype(np.int32)
        q_cnt[at] = 17
        cand = rng.integers(0, ix.n_docs, (nq, m2)).astype(np.int32)
        where = rng.permutation(m2)[:m]
        cand[at, where] = docs                                                                   # other positions, a longer list
        got = ix.score_docs(q_tok, q_cnt, cand)
        _same(got[at, where], base, f"{dtype}: nq {nq}, m {m2}")
        r_doc, r_score, r_count = ix.rerank(q_tok, q_cnt, cand, None, m2)                        # the rerank form scores the same bits
        lookup = {int(d): s for d, s in zip(docs, _bits(base))}
        hit = [j for j in range(int(r_count[at])) if int(r_doc[at, j]) in lookup]
        assert len(hit) >= m and all(lookup[int(r_doc[at, j])] == _bits(r_score[at])[j] for j in hit)


# ---- 5. rerank ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("m,k", [(1, 1), (64, 1), (65, 10), (65, 65), (1024, 100), (1024, 1024)])
def test_rerank(dtype, m, k):
    dim, tq, nq, base = 48, 6, 4, 7
    ix = _index(dtype, dim, doc_base=base)
    T, ptr = _int_store(dim)
    Q = _queries(nq, tq, dim, 51 + m)
    Q[3] = 0                                       # every doc scores +0 for query 3: the ranking is by ascending doc id
    ex = _Exact(T, ptr, Q, None)
    cand = _cands(nq, m, 52 + m, distinct=True) + base
    if m >= 64:
        cand[0, 3], cand[0, 5], cand[1, 9] = -1, base - 1, base + N_DOCS          # dead positions are never listed
        assert {10 + base, 11 + base} <= set(cand[2].tolist())                    # twins: equal scores, the lower id first
    counts = np.array([m, m // 2, m, m], np.int32)                               # query 1: k may exceed the live count
    for cc in (None, counts):
        got = ix.rerank(Q.astype(F), None, cand, cc, k)
        exp = ex.ranked(cand, cc, k, base)
        for g, e, what in zip(got, exp, ("doc", "score", "count")):
            _same(g, e, f"rerank {dtype} m {m} k {k} counts {cc is not None}: {what}")
    d, s, n = got
    if m >= 64:
        assert n[1] == min(k, m // 2 - (1 if 9 < m // 2 else 0)) and (k <= n[1] or (d[1, n[1]:] == -1).all() and (_bits(s[1, n[1]:]) == 0).all())
        if k == m:
            j = d[2].tolist().index(10 + base)
            assert d[2, j + 1] == 11 + base and _bits(s[2])[j] == _bits(s[2])[j + 1]
    assert (np.diff(d[3, : n[3]]) > 0).all() and (_bits(s[3]) == 0).all()


@pytest.mark.parametrize("dtype", TYPES)
def test_degenerate_inputs(dtype):
    import torch
    dim, tq, nq, m = 128, 33, 3, 70
    ix = _index(dtype, dim)
    T, ptr = _int_store(dim)
    Q = _queries(nq, tq, dim, 61)
    q_cnt = np.array([tq, 0, -5], np.int32)      # queries 1 and 2 have no live token
    cand = _cands(nq, m, 62, distinct=True)
    ex = _Exact(T, ptr, Q, q_cnt)
    got = ix.score_docs(Q.astype(F), q_cnt, cand)
    _same(got, ex.scores(cand, None), "no live query token: scores")
    assert (_bits(got[1:]) == 0).all() and (got[0] != 0).any()
    d, s, n = ix.rerank(Q.astype(F), q_cnt, cand, None, 20)
    for g, e, what in zip((d, s, n), ex.ranked(cand, None, 20), ("doc", "score", "count")):
        _same(g, e, f"no live query token: rerank {what}")
    assert d[1].tolist() == sorted(cand[1].tolist())[:20] and (_bits(s[1:]) == 0).all() and n.tolist() == [20, 20, 20]
    # nq == 0: nothing is launched, empty outputs of the right shape
    e_q, e_c = torch.zeros((0, tq, dim), device=DEV), torch.zeros((0, m), dtype=torch.int32, device=DEV)
    assert tuple(ix.score_docs_device(e_q, None, e_c).shape) == (0, m)
    d0, s0, n0 = ix.rerank_device(e_q, None, e_c, None, 5)
    assert tuple(d0.shape) == (0, 5) and tuple(s0.shape) == (0, 5) and tuple(n0.shape) == (0,)
    with pytest.raises(ValueError, match="k must be"):
        ix.rerank(Q.astype(F), q_cnt, cand, None, m + 1)
    with pytest.raises(ValueError, match="candidates per query"):
        ix.rerank(Q.astype(F), q_cnt, np.zeros((nq, 1025), np.int32), None, 5)


# ---- 6. the service ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", TYPES)
def test_service(golden_dir, storage):
    import sparse_rx
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    queries = dict(j["queries"])
    dim, n_docs = 40, len(j["corpus"])
    rng = np.random.default_rng(71)
    svc = sparse_rx.RetrievalService(device=DEV, tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    ids = svc.doc_ids
    row_of = {d: i for i, d in enumerate(ids)}
    tok = {d: rng.integers(-3, 4, (0 if i % 11 == 0 else int(rng.integers(1, 40)), dim)).astype(F) for i, d in enumerate(ids)}
    tok[ids[5]] = tok[ids[4]].copy()  # twins: equal scores, the lower row first
    q_tok = {q: rng.integers(-3, 4, (int(rng.integers(1, 34)), dim)).astype(F) for q in queries}
    svc.set_embeddings(rng.standard_normal((n_docs, 32)).astype(F), storage="f32")
    vecs = {q: rng.standard_normal(32).astype(F) for q in queries}
    with pytest.raises(ValueError, match="No token index"):
        svc.rerank_late({"q0": {ids[0]: 1.0}}, q_tok)
    svc.set_token_embeddings(tok, storage=storage)
    assert svc._late.n_docs == n_docs and svc._late.dtype == storage and svc._late.n_tokens == sum(len(t) for t in tok.values())

    def by_hand(lists, k):
        out = {}
        for q, row in lists.items():
            docs = list(row)
            scores = [F(int((q_tok[q].astype(np.int64) @ tok[d].astype(np.int64).T).max(axis=1).sum())) if len(tok[d]) else F(0) for d in docs]
            rd, rs, n = late_ref.rank([row_of[d] for d in docs], np.asarray(scores, F), np.ones(len(docs), bool), k) if docs else ([], [], 0)
            out[q] = {ids[int(rd[i])]: float(rs[i]) for i in range(n)}
        return out

    def check(got, exp, label):
        assert set(got) == set(exp), label
        for q in exp:
            assert list(got[q].items()) == list(exp[q].items()), (label, q)

    bm25 = svc.search_bm25(queries, top_k=60)
    assert any(len(r) > 20 for r in bm25.values()) and any(not r for r in bm25.values())
    check(svc.rerank_late(bm25, q_tok, top_k=10), by_hand(bm25, 10), "rerank_late over search_bm25")
    check(svc.rerank_late(bm25, q_tok, top_k=1000), by_hand(bm25, 1000), "rerank_late, every doc of the lists")
    hyb = svc.search_hybrid(queries, vecs, top_k=50)
    check(svc.rerank_late(hyb, q_tok, top_k=10), by_hand(hyb, 10), "rerank_late over search_hybrid")
    # the second form of set_token_embeddings gives the same index
    svc.set_token_embeddings((np.concatenate([tok[d] for d in ids]), [len(tok[d]) for d in ids]), storage=storage)
    check(svc.rerank_late(hyb, q_tok, top_k=10), by_hand(hyb, 10), "rerank_late, (matrix, counts)")
    # the keyword: the fusion late_pool deep, reranked on the device = the same two steps by hand
    excluded = [d for i, d in enumerate(ids) if i % 5 == 0]
    for kw in (dict(), dict(rescore=True), dict(excluded_docs=excluded), dict(must_terms=["w3"]), dict(must_not_terms=["w0"], rescore=True)):
        for pool, k in ((None, 10), (30, 10), (8, 10)):
            depth = min(max(k, 100), n_docs) if pool is None else pool
            got = svc.search_hybrid(queries, vecs, top_k=k, late_query_tokens=q_tok, late_pool=pool, **kw)
            fused = svc.search_hybrid(queries, vecs, top_k=depth, candidates=max(k, depth), **kw)  # the depth the keyword fetches
            check(got, by_hand(fused, k), f"search_hybrid(late_query_tokens) {kw.keys()} pool {pool}")
            if "excluded_docs" in kw:
                assert not any(d in excluded for r in got.values() for d in r)
    with pytest.raises(ValueError, match="do not combine"):
        svc.search_hybrid(queries, vecs, top_k=10, late_query_tokens=q_tok, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.rerank_late({"q0": {"nope": 1.0}}, q_tok)
    svc.close()
