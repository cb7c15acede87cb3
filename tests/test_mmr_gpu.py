"""The MMR selection on the GPU (include/sparse_rx_mmr.h), f32 and both half types.  The Gram stage is pinned to what existed
before it: G[a][b] must be, to the bit, what ``score_docs_device`` returns for the query that equals row a and the candidate
row b (every (a, b) in its own orientation); the selection is then tests/mmr_ref.py's on that matrix, to the bit.  Small
integer rows give a second yardstick that uses no engine code at all (every order of every sum is exact), and the half Gram
lies within the bound DESIGN.md section 4.13 derives for one MFMA chain.  The service test comes FIRST in this file: it
compares ``search_hybrid`` without the new keyword before and after the process has made its first MMR call."""
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
import hybrid_ref  # noqa: E402
import mmr_ref  # noqa: E402
import parity  # noqa: E402

pytestmark = pytest.mark.gpu
N, BASE = 4099, 7          # the last tile of 32 rows is partial
STORAGES = ["f32", "f16", "bf16"]
TWIN_A, TWIN_B, ZERO = 100, 200, 300   # rows TWIN_A and TWIN_B are identical, row ZERO is all zeros
SPECIAL = (4096, 4097, 4098, TWIN_A, TWIN_B, ZERO)
F = np.float32


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
    assert got.shape == exp.shape and got.dtype == exp.dtype, (label, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(_bits(got) != _bits(exp))
    assert len(bad) == 0, f"{label}: {len(bad)} words differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r} exp {exp[tuple(bad[0])]!r}"


# ---- 6. the service (first: see the module docstring) ---------------------------------------------------------------------------
def _items(res):
    return {q: [(d, F(s).view(np.uint32)) for d, s in row.items()] for q, row in res.items()}


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_service_diversify_and_hybrid(golden_dir, storage):
    import sparse_rx
    from test_hybrid_gpu import _assert_dicts, _rows_from_dicts
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    queries = dict(j["queries"])
    live = [q for q in queries if queries[q].strip()]
    dim, n_docs = 96, len(j["corpus"])
    rng = np.random.default_rng(61)
    emb = rng.standard_normal((n_docs, dim)).astype(F)
    for twin in range(1, n_docs, 3):  # a third of the docs share the embedding of the doc in front of them
        emb[twin] = emb[twin - 1]
    vecs = {q: rng.standard_normal(dim).astype(F) for q in queries}
    svc = sparse_rx.RetrievalService(device="cuda:0", tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    svc.set_embeddings(emb, storage=storage)
    row_of = {d: i for i, d in enumerate(svc.doc_ids)}
    excluded = [x for i, x in enumerate(svc.doc_ids) if i % 5 == 0]
    k, cdepth = 10, 20
    variants = [dict(), dict(rescore=True), dict(excluded_docs=excluded), dict(rescore=True, excluded_docs=excluded)]
    # without the keyword: today's call, made BEFORE this service (for the first storage: this process) has run an MMR launch
    before = [svc.search_hybrid(queries, vecs, top_k=k, candidates=cdepth, **kw) for kw in variants]
    sparse = _rows_from_dicts(svc.search_bm25(queries, top_k=cdepth), live, row_of, cdepth)
    dense = svc._dense.search(np.stack([vecs[q] for q in live]), cdepth)
    _assert_dicts(before[0], live, hybrid_ref.fuse(sparse, dense, k, "weighted", (0.3, 0.7)), svc.doc_ids)  # the parent's code path, restated

    # diversify(search_bm25) = the restatement on the same lists, G from the scorer of given docs
    rows = emb if storage == "f32" else half_ref.to_f32(svc._dense.corpus_to_host(), storage)
    lists = svc.search_bm25(queries, top_k=30)
    for lam, sim in ((0.5, "cosine"), (0.3, "dot"), (1.0, "cosine")):
        got = svc.diversify(lists, top_k=7, mmr_lambda=lam, similarity=sim)
        assert set(got) == set(lists)
        for q in queries:
            docs = [row_of[d] for d in lists[q]]
            if not docs:
                assert got[q] == {}
                continue
            cd = np.asarray(docs, np.int32)
            G = svc._dense.score_docs(rows[cd], np.tile(cd, (len(cd), 1)))
            rel = np.asarray(list(lists[q].values()), F)
            picked, _ = mmr_ref.select(G, rel, np.ones(len(cd), bool), 7, *mmr_ref.weights(lam), mmr_ref.MODES[sim])
            assert list(got[q]) == [svc.doc_ids[cd[c]] for c in picked], (q, lam, sim)
            assert [F(v).view(np.uint32) for v in got[q].values()] == [rel[c].view(np.uint32) for c in picked]  # the ORIGINAL scores
            if lam == 1.0:
                assert list(got[q]) == list(lists[q])[:7]  # BM25 lists are descending: lambda 1 keeps them
    assert any(list(svc.diversify(lists, top_k=7)[q]) != list(lists[q])[:7] for q in live)  # the twins make MMR reorder something

    # search_hybrid(mmr_lambda) = diversify(search_hybrid(top_k = pool, candidates = pool), top_k)
    top = 6
    pool = min(4 * top, 256, n_docs)
    for kw in variants:
        got = svc.search_hybrid(queries, vecs, top_k=top, mmr_lambda=0.5, **kw)
        exp = svc.diversify(svc.search_hybrid(queries, vecs, top_k=pool, candidates=pool, **kw), top)
        assert _items(got) == _items(exp), kw
        assert all(len(got[q]) == top for q in live) and all(got[q] == {} for q in queries if q not in live)
        if "excluded_docs" in kw:
            assert all(not set(got[q]) & set(excluded) for q in live)
    got = svc.search_hybrid(queries, vecs, top_k=top, mmr_lambda=0.25, mmr_pool=9, mmr_similarity="dot", candidates=15)
    exp = svc.diversify(svc.search_hybrid(queries, vecs, top_k=9, candidates=15), top, mmr_lambda=0.25, similarity="dot")
    assert _items(got) == _items(exp)
    with pytest.raises(ValueError, match="mmr_pool"):
        svc.search_hybrid(queries, vecs, top_k=top, mmr_lambda=0.5, mmr_pool=257)
    with pytest.raises(ValueError, match="at most 256"):
        svc.diversify({live[0]: {d: 1.0 for d in svc.doc_ids[:257]}})
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.diversify({live[0]: {"no such doc": 1.0}})

    # ... and after all that, the call without the keyword still returns what it returned
    after = [svc.search_hybrid(queries, vecs, top_k=k, candidates=cdepth, **kw) for kw in variants]
    for b, a, kw in zip(before, after, variants):
        assert _items(b) == _items(a), kw
    svc.close()


# ---- the corpora of the kernel tests ---------------------------------------------------------------------------------------------
_WORLD = {}


def _world(storage, dim, kind="normal"):
    """(index, the rows it holds as f32[N, dim]) -- random normal rows, or small integers; built once per module."""
    import sparse_rx
    key = (storage, dim, kind)
    if key not in _WORLD:
        rng = np.random.default_rng(1000 + dim + (0 if kind == "normal" else 7))
        emb = rng.standard_normal((N, dim)).astype(F) if kind == "normal" else rng.integers(-3, 4, (N, dim)).astype(F)
        emb[TWIN_B] = emb[TWIN_A]
        emb[ZERO] = 0.0
        if storage == "f32":
            ix = sparse_rx.DenseF32Index(emb, device="cuda:0", doc_base=BASE)
            rows = emb
        else:
            ix = sparse_rx.DenseHalfIndex(emb, dtype=storage, device="cuda:0", doc_base=BASE)
            rows = half_ref.to_f32(ix.corpus_to_host(), storage)
        _WORLD[key] = (ix, rows)
    return _WORLD[key]


def _pool(rng, nq, m, grid=False):
    """cand_doc i32[nq, m] (distinct GLOBAL ids per row; the special rows at positions 1 .. 6 when they fit), cand_rel f32[nq, m]"""
    plain = np.setdiff1d(np.arange(N), SPECIAL)
    cd = np.stack([rng.choice(plain, m, replace=False) for _ in range(nq)]).astype(np.int32)
    if m >= 8:
        cd[:, 1:7] = SPECIAL
    cr = rng.standard_normal((nq, m)).astype(F)
    cr[1::2] = np.round(cr[1::2] * 4) / 4  # every other query: many equal relevances
    if grid:
        cr = (rng.integers(-64, 65, (nq, m)) / 64).astype(F)
    return cd + BASE, cr


def _expected_gram(ix, rows, cd):
    """f32[nq, m, m] from the scorer of given docs: the query = the row of position a, the candidates = the whole list; both
    orientations of every pair are computed, nothing is mirrored.  Positions outside the corpus get a zero query."""
    import torch
    nq, m = cd.shape
    local = cd.astype(np.int64) - BASE
    inside = (local >= 0) & (local < N)
    q = np.where(inside[..., None], rows[np.clip(local, 0, N - 1)], F(0.0)).reshape(nq * m, -1)
    cand = np.repeat(cd, m, axis=0)  # row (q, a) -> list q
    out = ix.score_docs_device(torch.as_tensor(q, device=ix.device), torch.as_tensor(cand, device=ix.device))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(nq, m, m)


def _run(ix, cd, cr, cc, k, lam, sim):
    import torch
    t = lambda x: None if x is None else torch.as_tensor(x, device=ix.device)
    out = ix.mmr_device(t(cd), t(cr), t(cc), k, lam, sim, return_sim=True)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def _check(ix, rows, cd, cr, cc, k, lam, sim, label):
    """One batch against the scorer + the restatement, to the bit."""
    G = _expected_gram(ix, rows, cd)
    doc, rel, mmr, count, got_sim = _run(ix, cd, cr, cc, k, lam, sim)
    exp = mmr_ref.select_rows(G, cd, cr, cc, N, BASE, k, lam, mmr_ref.MODES[sim])
    for q in range(len(cd)):
        live = mmr_ref.live_mask(cd[q], cr[q], None if cc is None else cc[q], N, BASE)
        _same(got_sim[q], mmr_ref.mask_gram(G[q], live), f"{label} out_sim q={q}")
    _same(count, exp[3], f"{label} out_count")
    _same(doc, exp[0], f"{label} out_doc")
    _same(rel, exp[1], f"{label} out_rel")
    _same(mmr, exp[2], f"{label} out_mmr")
    return doc, rel, mmr, count, got_sim


def _counts(m):
    return np.array([m, 0, -2, m + 7, max(1, m // 2)], np.int32)


# ---- 1. bit-exact against what existed before ------------------------------------------------------------------------------------
BASE_CASE = dict(m=100, dim=200, k=10, lam=0.5, sim="cosine")
CASES = ([dict(BASE_CASE)] + [dict(BASE_CASE, m=m, k=min(10, m)) for m in (1, 31, 32, 33, 256)] + [dict(BASE_CASE, dim=d) for d in (64, 768, 1024)]
         + [dict(BASE_CASE, k=1), dict(BASE_CASE, k=100)] + [dict(BASE_CASE, lam=x) for x in (0.0, 0.3, 1.0)] + [dict(BASE_CASE, sim="dot")]
         + [dict(m=256, dim=1024, k=256, lam=0.5, sim="cosine")])


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "m{m}-d{dim}-k{k}-l{lam}-{sim}".format(**c))
def test_bits_against_the_scorer_and_the_restatement(storage, case):
    m, dim, k, lam, sim = (case[x] for x in ("m", "dim", "k", "lam", "sim"))
    ix, rows = _world(storage, dim)
    rng = np.random.default_rng(m * 7 + dim + k)
    cd, cr = _pool(rng, 5, m)
    out = _check(ix, rows, cd, cr, _counts(m), k, lam, sim, f"{storage} {case}")
    assert out[3].tolist() == [min(k, m), 0, 0, min(k, m), min(k, max(1, m // 2))]
    if case == BASE_CASE:
        _check(ix, rows, cd, cr, None, k, lam, sim, f"{storage} cand_count=None")


# ---- 2. exact arithmetic, independent of any engine code --------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dim,m", [(200, 100), (1024, 33)])
def test_small_integers_are_exact(storage, dim, m):
    """Rows in {-3 .. 3}: |G| <= 9 * 1024, w_rel * rel is a multiple of 2^-8 and w_div * G a multiple of 1 / 4 for lambda in
    {1/4, 1/2, 3/4} and relevances j / 64: every value is representable, so the fp64 restatement is THE answer."""
    ix, rows = _world(storage, dim, "integers")
    rng = np.random.default_rng(dim + m)
    cd, cr = _pool(rng, 3, m, grid=True)
    for lam in (0.25, 0.5, 0.75):
        doc, rel, mmr, count, sim = _run(ix, cd, cr, None, 10, lam, "dot")
        for q in range(3):
            G = mmr_ref.gram_exact(rows[cd[q] - BASE])
            assert np.array_equal(sim[q].astype(np.float64), G), (storage, q)
            picked, values = mmr_ref.select_naive_f64(G, cr[q], np.ones(m, bool), 10, *mmr_ref.weights(lam), mmr_ref.DOT)
            assert count[q] == 10 and doc[q].tolist() == cd[q, picked].tolist(), (storage, lam, q)
            assert np.array_equal(mmr[q].astype(np.float64), values) and np.array_equal(rel[q], cr[q, picked])


# ---- 3. the half Gram against fp64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("dim", [200, 1024])
def test_half_gram_within_the_chain_bound(dtype, dim):
    ix, rows = _world(dtype, dim)
    rng = np.random.default_rng(dim)
    cd, cr = _pool(rng, 2, 100)
    sim = _run(ix, cd, cr, None, 1, 0.5, "dot")[4]
    for q in range(2):
        codes, flag = half_ref.convert(rows[cd[q] - BASE], dtype, ix.dim_pad)  # the rows are half values already: the rounding is the identity
        assert flag == 0
        err = np.abs(sim[q].astype(np.float64) - mmr_ref.gram_exact(rows[cd[q] - BASE]))
        assert (err <= half_ref.tol(codes, codes, dtype)).all(), (dtype, dim, err.max())  # dim_pad * 2^-22 * sum |a_i b_i|
        assert err.max() > 0  # not a comparison of a thing with itself


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------
def _raw(ix, cd, cr, cc, k, lam, sim, want_mmr=True, want_sim=True):
    """The entry point itself on the current stream, every output pre-filled with junk.  Host arrays back (None where not asked)."""
    import torch
    from sparse_rx import _capi
    from sparse_rx.dense import check_mmr_args
    from sparse_rx.index import _stream_ptr
    nq, m = cd.shape
    dev = ix.device
    t = lambda x: None if x is None else torch.as_tensor(x, device=dev)
    d_cd, d_cr, d_cc = t(cd), t(cr), t(cc)
    doc = torch.full((nq, k), -77, dtype=torch.int32, device=dev)
    rel = torch.full((nq, k), float("nan"), dtype=torch.float32, device=dev)
    mmr = torch.full((nq, k), float("nan"), dtype=torch.float32, device=dev)
    count = torch.full((nq,), -77, dtype=torch.int32, device=dev)
    sim_t = torch.full((nq, m, m), float("nan"), dtype=torch.float32, device=dev)
    L = _capi.lib()
    ws = torch.full((L.srx_mmr_workspace_bytes(nq, m),), 0xAB, dtype=torch.uint8, device=dev)
    mode, w_rel, w_div = check_mmr_args(lam, sim)
    rc = ix._launch_mmr(L, d_cd.data_ptr(), d_cr.data_ptr(), None if d_cc is None else d_cc.data_ptr(), nq, m, k, mode, w_rel, w_div, doc.data_ptr(),
                        rel.data_ptr(), mmr.data_ptr() if want_mmr else None, count.data_ptr(), sim_t.data_ptr() if want_sim else None, ws.data_ptr(),
                        ws.numel(), _stream_ptr(torch, dev))
    _capi.check(rc, ix._mmr_entry)
    torch.cuda.synchronize()
    return (doc.cpu().numpy(), rel.cpu().numpy(), mmr.cpu().numpy() if want_mmr else None, count.cpu().numpy(), sim_t.cpu().numpy() if want_sim else None)


@pytest.mark.parametrize("storage", STORAGES)
def test_edges(storage):
    import torch
    ix, rows = _world(storage, 200)
    rng = np.random.default_rng(9)
    m, k = 40, 12
    cd, cr = _pool(rng, 6, m)
    a, b, z = 4, 5, 6                                # positions of TWIN_A, TWIN_B, ZERO (positions 1 .. 3: rows 4096 .. 4098)
    assert cd[0, 1:4].tolist() == [BASE + 4096, BASE + 4097, BASE + 4098] and cd[0, a] - BASE == TWIN_A and cd[0, z] - BASE == ZERO
    cd[0, 7], cd[0, 8], cd[0, 9] = -1, BASE - 1, BASE + N  # dead ids inside the count
    cr[0, 10] = np.nan                                       # a NaN relevance is dead
    cr[2] = -np.abs(cr[2]) - 1.0                             # query 2: only negative relevances
    cr[:, a] = cr[:, b] = 9.0                                # the twins: equal relevance, the best of the list
    cr[2, a] = cr[2, b] = -0.5
    cc = np.array([m, m, m, 5, m, m], np.int32)             # query 3: fewer live positions than k (and TWIN_B past the count)
    dead0 = [7, 8, 9, 10]
    for sim in ("cosine", "dot"):
        doc, rel, mmr, count, S = _check(ix, rows, cd, cr, cc, k, 0.5, sim, f"{storage} edges {sim}")
        assert count[0] == k and not set(doc[0].tolist()) & {-1, BASE - 1, BASE + N, int(cd[0, 10])}  # the dead ids are never returned
        assert not S[0][dead0, :].any() and not S[0][:, dead0].any() and not np.signbit(S[0][dead0, :]).any() and not np.signbit(S[0][:, dead0]).any()
        assert count.tolist() == [k, k, k, 5, k, k] and (doc[3, 5:] == -1).all() and not _bits(rel[3, 5:]).any() and not _bits(mmr[3, 5:]).any()
        assert count[2] == k and (rel[2, :k] < 0).all()  # negative relevances are selectable
        assert {int(x) for x in cd[0, 1:4]} <= set(cd[0].tolist()) and S[0][1:4, 1:4].any()  # the partial tile's rows were read
        # the twins: the same bits as either's self-similarity, in both orientations; the lowest position goes first
        for q in range(6):
            g = _bits(S[q])
            assert doc[q, 0] == cd[q, a]
            if q != 3:
                assert g[a, a] != 0 and g[a, b] == g[a, a] == g[b, b] == g[b, a], (storage, sim, q)
        assert not S[0][z, :].any() and not S[0][:, z].any()  # the all-zero row
    # cosine: the zero row's similarity to everything is +0, so it is picked with fl(w_rel * rel), whenever it is picked
    doc, rel, mmr, count, S = _raw(ix, cd, cr, cc, m, 0.5, "cosine")
    pos_z = doc[1].tolist().index(int(cd[1, z]))
    assert count[1] == m and mmr[1, pos_z].view(np.uint32) == (F(0.5) * cr[1, z]).view(np.uint32)
    # lambda = 1: the stable sort of the live positions by relevance, descending
    doc1, rel1, _, count1, _ = _raw(ix, cd, cr, cc, m, 1.0, "cosine")
    for q in range(6):
        live = mmr_ref.live_mask(cd[q], cr[q], cc[q], N, BASE)
        idx = np.flatnonzero(live)
        order = idx[np.argsort(-cr[q, idx], kind="stable")]
        assert count1[q] == len(idx) and doc1[q, : len(idx)].tolist() == cd[q, order].tolist() and (doc1[q, len(idx):] == -1).all()
        _same(rel1[q, : len(idx)], cr[q, order], "lambda 1 out_rel")
    # junk-filled buffers are fully overwritten (the helper fills them); out_mmr = NULL and out_sim = NULL change no other output
    full = _raw(ix, cd, cr, cc, k, 0.3, "cosine")
    assert not np.isnan(full[1]).any() and not np.isnan(full[2]).any() and not np.isnan(full[4]).any() and (full[0] != -77).all() and (full[3] != -77).all()
    for want_mmr, want_sim in ((False, True), (True, False), (False, False)):
        part = _raw(ix, cd, cr, cc, k, 0.3, "cosine", want_mmr, want_sim)
        for i, (x, y) in enumerate(zip(part, full)):
            if x is not None:
                _same(x, y, f"{storage} out_mmr={want_mmr} out_sim={want_sim} output {i}")
    # a side stream
    side = torch.cuda.Stream(device=ix.device)
    side.wait_stream(torch.cuda.current_stream(ix.device))
    with torch.cuda.stream(side):
        on_side = _raw(ix, cd, cr, cc, k, 0.3, "cosine")
    for i, (x, y) in enumerate(zip(on_side, full)):
        _same(x, y, f"{storage} side stream output {i}")
    # the Python layer: an empty batch launches nothing; a batch is split so that one call stays within 256 MiB
    empty = ix.mmr(np.zeros((0, 5), np.int32), np.zeros((0, 5), F), None, 3)
    assert [x.shape for x in empty] == [(0, 3), (0, 3), (0, 3), (0,)]


def test_large_batch_is_split(monkeypatch):
    """The Python layer cuts a batch into calls whose Gram matrices fit the per-call budget; the rows do not change."""
    from sparse_rx import dense
    ix, rows = _world("f16", 64)
    rng = np.random.default_rng(3)
    cd, cr = _pool(rng, 7, 33)
    whole = _run(ix, cd, cr, _counts(33)[[0, 1, 2, 3, 4, 0, 4]], 5, 0.5, "cosine")
    monkeypatch.setattr(dense, "MMR_CALL_BYTES", 3 * 33 * 33 * 4)  # three queries per call: 3 + 3 + 1
    split = _run(ix, cd, cr, _counts(33)[[0, 1, 2, 3, 4, 0, 4]], 5, 0.5, "cosine")
    for i, (x, y) in enumerate(zip(split, whole)):
        _same(x, y, f"split output {i}")
    plain = ix.mmr(cd, cr, _counts(33)[[0, 1, 2, 3, 4, 0, 4]], 5, 0.5, "cosine")  # no out_sim: the index's own workspace
    for i, (x, y) in enumerate(zip(plain, whole[:4])):
        _same(x, y, f"workspace output {i}")


# ---- 5. independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_a_row_does_not_depend_on_the_batch(storage):
    ix, rows = _world(storage, 768)
    rng = np.random.default_rng(12)
    cd, cr = _pool(rng, 5, 100)
    cc = np.array([100, 3, 100, 77, 100], np.int32)
    batch = _run(ix, cd, cr, cc, 10, 0.5, "cosine")
    alone = _run(ix, cd[3:4], cr[3:4], cc[3:4], 10, 0.5, "cosine")
    for i, (x, y) in enumerate(zip(alone, batch)):
        _same(x[0], y[3], f"{storage} output {i}")
    other = cd.copy()
    other[[0, 1, 2, 4]] = _pool(np.random.default_rng(13), 4, 100)[0]  # other neighbours, another nq
    again = _run(ix, np.concatenate([other, other[:2]]), np.concatenate([cr, cr[:2]]), np.concatenate([cc, cc[:2]]), 10, 0.5, "cosine")
    for i, (x, y) in enumerate(zip(again, batch)):
        _same(x[3], y[3], f"{storage} other neighbours, output {i}")
