"""Term constraints on the GPU (include/sparse_rx_terms.h): filter rows built from the posting lists, and the searches that take
them.  Expected bits are never the engine's own: the NumPy restatement (tests/terms_ref.py) on the CSR an index was built from,
packed by filter_ref.  Every comparison is exact, and every output buffer is pre-filled with 0xFFFFFFFF so that a word the
builder does not write shows.  Corpora and indexes are those of tests/test_search_plans.py, built once per module."""
import ctypes
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
import terms_ref  # noqa: E402
from test_filter_gpu import _FilterEnv, _masks, _search_both  # noqa: E402
from test_gpu_parity import _assert_exact  # noqa: E402
from test_search_plans import CORPORA  # noqa: E402

pytestmark = pytest.mark.gpu


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


def _csr(lists, device):
    import torch
    ptr = np.zeros(len(lists) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in lists])
    term = np.asarray([t for r in lists for t in r] or [0], np.int32)  # an empty term array still needs an address
    return torch.as_tensor(ptr, device=device), torch.as_tensor(term, device=device)


def _build(ix, all_, any_, none, base=None, q_base=None, canonical=False):
    """Filter rows from the builder as uint32[n_rows, words], the output pre-filled with ones.  canonical: through the C call
    with a descriptor that names the canonical blocks only, so the reader of `post` runs even where a compact copy exists."""
    import torch
    import sparse_rx
    from sparse_rx import _capi
    n_rows = len(next(x for x in (all_, any_, none) if x is not None))
    out = torch.full((n_rows, filter_ref.words(ix.n_docs)), -1, dtype=torch.int32, device=ix.device)
    pairs = [None if x is None else _csr(x, ix.device) for x in (all_, any_, none)]
    qb = None if q_base is None else torch.as_tensor(np.asarray(q_base, np.int32), device=ix.device)
    if not canonical:
        f = ix.term_filter_device(*pairs, base=base, q_base=qb, out=out)
        assert isinstance(f, sparse_rx.DocFilter) and f.bits is out and (f.n_docs, f.doc_base, f.n_filters) == (ix.n_docs, ix.doc_base, n_rows)
    else:
        assert ix.post is not None
        d = _capi.IndexDesc.from_buffer_copy(ix._desc)
        d.post16 = None
        bdesc, keep = (None, None) if base is None else base.launch_args(qb, n_rows)
        ptrs = [p for pair in pairs for p in ((None, None) if pair is None else (pair[0].data_ptr(), pair[1].data_ptr()))]
        rc = _capi.lib().srx_filter_from_terms(ctypes.byref(d), n_rows, *ptrs, bdesc, out.data_ptr(), torch.cuda.current_stream(ix.device).cuda_stream)
        _capi.check(rc, "srx_filter_from_terms")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _assert_rows(got, masks, label):
    exp = np.stack([filter_ref.pack(m) for m in masks])
    assert got.shape == exp.shape, label
    bad = np.argwhere(got != exp)
    assert bad.size == 0, f"{label}: {len(bad)} words differ, first at row {bad[0][0]} word {bad[0][1]}: got {got[tuple(bad[0])]:#x}, expected {exp[tuple(bad[0])]:#x}"


def _row_set(a, b, c, d):
    """The rows of test 1 from four term ids (a, b, c share a doc where the corpus allows it): (all, any, none) per row."""
    return [([a], [], []), ([a, b], [], []), ([a, b, c], [], []),            # all-only with 1, 2 and 3 terms
            ([], [a, d], []), ([], [d], []),                                  # any-only
            ([], [], [a]), ([], [], [a, d]),                                  # none-only
            ([a], [b, d], [c]), ([d], [a, b], [c, c]),                        # all three together
            ([], [], []),                                                     # the empty triple: every doc
            ([-1], [], []), ([a, -1], [], []), ([], [-1], []), ([], [-1, a], []), ([], [], [-1]), ([a], [], [-1, d]),  # -1 in each list
            ([a, a, b, a], [d, d], [c, c]),                                   # duplicates
            ([a, b], [], [b]), ([a], [a], [a])]                               # a term in all and in none


# ---- 1. builder bits equal the restatement, every word, tail and padding included ----------------------------------------------
@pytest.mark.parametrize("name,canonical", [("uniform", True), ("uniform", False), ("compact", False), ("dot16", True), ("dot16", False),
                                            ("zipf", False)])
def test_builder_bits(env, name, canonical):
    import sparse_rx
    ix = env.index(name)
    c = env.corpus(name)[0]
    terms_ref.assert_no_stored_zero(c.data)
    n = CORPORA[name][0]
    assert (ix.post16 is not None) and (ix.post is not None or not canonical)
    df = np.bincount(c.indices, minlength=CORPORA[name][2])
    if name == "zipf":  # the most and the least frequent terms
        order = np.argsort(-df, kind="stable")
        a, b, d = (int(t) for t in order[:3])
        cc = int(order[df[order] > 0][-1])
        assert df[a] > n // 4 and 0 < df[cc] * 1000 < df[a]
    else:  # three terms of one doc, so that their intersection is not empty, and one other
        doc = int(np.flatnonzero(np.diff(c.indptr) >= 3)[7])
        a, b, cc = (int(t) for t in np.unique(c.indices[c.indptr[doc]:c.indptr[doc + 1]])[:3])
        d = int(np.flatnonzero(df > 0)[-1])
    rows = _row_set(a, b, cc, d)
    all_, any_, none = ([list(r[i]) for r in rows] for i in range(3))
    got = _build(ix, all_, any_, none, canonical=canonical)
    masks = terms_ref.term_masks(c.indptr, c.indices, n, all_, any_, none)
    assert masks[1].any() and masks[9].all() and not masks[10].any() and not masks[17].any()
    _assert_rows(got, masks, f"{name} canonical={canonical}")
    # a list that is absent altogether
    _assert_rows(_build(ix, all_, None, None, canonical=canonical), terms_ref.term_masks(c.indptr, c.indices, n, all_, None, None), f"{name} all only")
    _assert_rows(_build(ix, None, None, none, canonical=canonical), terms_ref.term_masks(c.indptr, c.indices, n, None, None, none), f"{name} none only")
    # the same rows over a 3-row base of densities 1 / 0.5 / 0.01, q_base cycling through -1 and the rows
    base_masks = _masks(n, [1.0, 0.5, 0.01], seed=41)
    base = sparse_rx.DocFilter.from_masks(base_masks, device=ix.device, doc_base=ix.doc_base)
    q_base = [(i % 4) - 1 for i in range(len(rows))]
    got = _build(ix, all_, any_, none, base=base, q_base=q_base, canonical=canonical)
    _assert_rows(got, terms_ref.term_masks(c.indptr, c.indices, n, all_, any_, none, base_masks, q_base), f"{name} with a base")
    got = _build(ix, all_, any_, none, base=base, canonical=canonical)  # q_base None: base row 0
    _assert_rows(got, terms_ref.term_masks(c.indptr, c.indices, n, all_, any_, none, base_masks, None), f"{name} base row 0")


def test_host_door_validates(env):
    ix = env.index("uniform")
    c = env.corpus("uniform")[0]
    f = ix.term_filter([[3], []], None, [[-1], [5, 7]])
    import torch
    torch.cuda.synchronize()
    _assert_rows(f.bits.cpu().numpy().view(np.uint32), terms_ref.term_masks(c.indptr, c.indices, ix.n_docs, [[3], []], None, [[-1], [5, 7]]), "term_filter")
    for bad in (dict(all_terms=[[ix.vocab]]), dict(all_terms=[[-2]]), dict(all_terms=[[1]], none_terms=[[1], [2]]), dict(),
                dict(all_terms=[[1]], q_base=[0])):
        with pytest.raises(ValueError):
            ix.term_filter(**bad)
    with pytest.raises(ValueError):
        ix.term_filter([[1]], base=f, q_base=[2])


# ---- 2. geometry edges, each a small index of its own --------------------------------------------------------------------------
GEOMETRY = [  # (n_docs, tile_log2, unit_tiles, keep_canonical)
    (20_011, 10, 4, True),    # the last word, the last tile and the last unit are all partial
    (20_011, 10, 4, False),
    (100, 10, 4, True),       # one partial unit, a row of 4 words
    (64, 6, 1, True),         # one unit of 64 docs: 2 words, and the row's 2 padding words
    (1_000, 6, 1, False),     # units of 64 docs, the smallest: a unit is no multiple of 16 bytes
    (500, 6, 3, True),        # units of 192 docs: 6 words
    (60_000, 14, 3, True),    # the 49 152-doc unit, the LDS bitmaps at full size, and a second unit that is partial
    (60_000, 14, 3, False),
    (70_000, 14, 4, True),    # units of 65 536 docs: no compact copy, the canonical reader cuts the units into 3-tile pieces
]


@pytest.mark.parametrize("n_docs,tile_log2,unit_tiles,keep", GEOMETRY)
def test_geometry_edges(n_docs, tile_log2, unit_tiles, keep):
    import sparse_rx
    rng = np.random.default_rng(n_docs + tile_log2)
    unit = unit_tiles << tile_log2
    piece = unit if unit <= 49_152 else (49_152 >> tile_log2) << tile_log2  # what one workgroup covers
    edges = sorted({0, n_docs - 1} | {d for u in range(0, n_docs, piece) for d in (u, min(u + piece, n_docs) - 1)}
                   | {d for u in range(0, n_docs, unit) for d in (u, min(u + unit, n_docs) - 1)})
    has = np.zeros((n_docs, 5), bool)
    has[edges, 0] = True                       # term 0: the first and the last doc of every unit, docs 0 and n_docs - 1
    has[:, 1] = rng.random(n_docs) < 0.3
    has[:, 1] |= has[:, 0]                     # term 1: 30 % of the docs, the edge docs among them
    has[:, 2] = rng.random(n_docs) < 0.01
    has[:, 3] = True                           # term 3: every doc
    # term 4: no doc
    indptr = np.zeros(n_docs + 1, np.int64)
    indptr[1:] = np.cumsum(has.sum(1))
    indices = np.nonzero(has)[1].astype(np.int32)
    data = rng.uniform(0.5, 2.0, len(indices)).astype(np.float32)
    terms_ref.assert_no_stored_zero(data)
    ix = sparse_rx.DeviceIndex.from_csr(indptr, indices, data, np.ones(5, np.float32), mode="dot", tile_log2=tile_log2, unit_tiles=unit_tiles,
                                        keep_canonical=keep, doc_base=123)
    try:
        assert ix.unit_tiles == unit_tiles and (ix.post16 is None) == (unit > 49_152) and (ix.post is None) == (not keep)
        rows = [([0], [], []), ([0, 1], [], []), ([1], [], [0]), ([], [0, 2], []), ([], [], [0]), ([], [], [1, 2]), ([3], [], []),
                ([3], [], [3]), ([4], [], []), ([], [4], []), ([], [], [4]), ([], [], []), ([1, 3], [2, 0], [4, -1])]
        all_, any_, none = ([list(r[i]) for r in rows] for i in range(3))
        masks = terms_ref.term_masks(indptr, indices, n_docs, all_, any_, none)
        assert np.flatnonzero(masks[0]).tolist() == edges and masks[6].all() and masks[11].all() and not masks[8].any()
        label = f"n_docs={n_docs} tile_log2={tile_log2} unit_tiles={unit_tiles} keep={keep}"
        _assert_rows(_build(ix, all_, any_, none), masks, label)
        if keep and ix.post16 is not None:
            _assert_rows(_build(ix, all_, any_, none, canonical=True), masks, label + " canonical reader")
        base_masks = _masks(n_docs, [0.5, 1.0], seed=7)
        base_masks[0, edges] = True
        base = sparse_rx.DocFilter.from_masks(base_masks, device=ix.device, doc_base=123)
        q_base = [i % 3 - 1 for i in range(len(rows))]
        _assert_rows(_build(ix, all_, any_, none, base=base, q_base=q_base),
                     terms_ref.term_masks(indptr, indices, n_docs, all_, any_, none, base_masks, q_base), label + " with a base")
    finally:
        ix.close()


# ---- 3. constrained sparse search ------------------------------------------------------------------------------------------------
def _query_constraints(q, nq):
    """One (all, any, none) triple per query, from its own terms: must-not its first term, any of its first two, must its last"""
    all_, any_, none = [], [], []
    for i in range(nq):
        t = [int(x) for x in q[1][q[0][i]:q[0][i + 1]]]
        all_.append([t[-1]] if i % 3 == 2 else [])
        any_.append(t[:2] if i % 3 == 1 else [])
        none.append([t[0]] if i % 3 == 0 else [])
    return all_, any_, none


@pytest.mark.parametrize("name", ["uniform", "compact"])
def test_constrained_sparse_search(env, name):
    import torch
    nq, k = 37, 100
    ix = env.index(name)
    c = env.corpus(name)[0]
    base = CORPORA[name][5].get("doc_base", 0)
    q, full = env.full_ranking(name, nq, "u8", 2001)
    all_, any_, none = _query_constraints(q, nq)
    masks = terms_ref.term_masks(c.indptr, c.indices, ix.n_docs, all_, any_, none)
    exp = filter_ref.filtered_rows(*full, list(masks), base, k)
    assert (exp[2] > 0).all() and (exp[2] < full[2]).any()
    out = torch.full((nq, filter_ref.words(ix.n_docs)), -1, dtype=torch.int32, device=ix.device)
    flt = ix.term_filter_device(_csr(all_, ix.device), _csr(any_, ix.device), _csr(none, ix.device), out=out)
    ix.set_opts(target_blocks=16)
    try:
        rows, packed = _search_both(ix, q, k, flt, np.arange(nq))
    finally:
        ix.set_opts()
    _assert_exact(rows, exp, f"{name} constrained search_device")
    _assert_exact(packed, exp, f"{name} constrained search_packed_device")


def test_constrained_search_past_one_page(env):
    """k = 1 500 under one hot must-term: the paging carries the term-built filter.  On the zipf corpus, whose hottest term is in
    enough docs (the uniform corpus has no term in 1 500 docs)."""
    name, k = "zipf", 1500
    ix = env.index(name)
    c = env.corpus(name)[0]
    batch, full = env.full_ranking(name, 16, "zipf8", 2002)
    hot = int(np.argmax(np.bincount(c.indices, minlength=CORPORA[name][2])))
    mask = terms_ref.term_masks(c.indptr, c.indices, ix.n_docs, [[hot]], None, None)[0]
    exp = filter_ref.filtered_rows(*full, mask, 0, k)
    # the queries of the batch for which the restated set holds k scoring docs (a query of rare terms alone scores fewer docs)
    pick = np.flatnonzero(exp[2] == k)[:6]
    assert len(pick) >= 4, f"too few queries with {k} scoring docs under the must-term: the oracle counts {exp[2].tolist()}"
    exp = tuple(a[pick] for a in exp)
    spans = [np.arange(batch[0][i], batch[0][i + 1]) for i in pick]
    q_ptr = np.zeros(len(pick) + 1, np.int32)
    q_ptr[1:] = np.cumsum([len(x) for x in spans])
    q = (q_ptr, batch[1][np.concatenate(spans)], batch[2][np.concatenate(spans)])
    flt = ix.term_filter([[hot]])
    ix.set_opts(target_blocks=16)
    try:
        got = ix.search(*q, k, filter=flt)
    finally:
        ix.set_opts()
    _assert_exact(got, exp, "paged constrained search")


# ---- 4. the dense indexes take a term-built filter -------------------------------------------------------------------------------
def test_dense_indexes_under_term_rows():
    import sparse_rx
    from sparse_rx import synth
    n, dim, base = 32_801, 64, 1_000
    c = synth.uniform_corpus_np(n, 400, 12, seed=51)
    terms_ref.assert_no_stored_zero(c.data)
    _, idf, avgdl = synth.corpus_stats(c)
    ix = sparse_rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, tile_log2=10, unit_tiles=4,
                                        doc_base=base, keep_canonical=False)
    rng = np.random.default_rng(52)
    emb = rng.standard_normal((n, dim)).astype(np.float32)
    queries = rng.standard_normal((5, dim)).astype(np.float32)
    all_, any_, none = [[3], [], [5]], [[], [1, 2, 4], []], [[7], [], [8, 9]]
    q_filter = np.array([1, -1, 0, 2, 1], np.int32)
    masks = terms_ref.term_masks(c.indptr, c.indices, n, all_, any_, none)
    assert all(10 < m.sum() < n for m in masks)
    built = ix.term_filter(all_, any_, none)
    restated = sparse_rx.DocFilter.from_masks(masks, doc_base=base)
    try:
        for dense in (sparse_rx.DenseF32Index(emb, doc_base=base), sparse_rx.DenseHalfIndex(emb, dtype="f16", doc_base=base)):
            for k in (10, 100):
                got = dense.search(queries, k, filter=built, q_filter=q_filter)
                exp = dense.search(queries, k, filter=restated, q_filter=q_filter)
                assert (exp[2] == k).all()
                _assert_exact(got, exp, f"{type(dense).__name__} k={k}")
    finally:
        ix.close()


# ---- 5. the API mirrors on tests/golden/text_small.json --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text(golden_dir):
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    import sparse_rx
    # the text build_host_index indexes: "text", else "content", else "body"; the title never
    tokens = {d: set(sparse_rx.tokenize(doc.get("text", doc.get("content", doc.get("body", ""))) or "")) for d, doc in j["corpus"].items()}
    return j, tokens


def _satisfying(tokens, must=(), any_=(), must_not=()):
    """The doc ids whose tokenised text satisfies the constraint, in corpus order"""
    return [d for d, t in tokens.items() if all(w in t for w in must) and (not any_ or any(w in t for w in any_)) and not any(w in t for w in must_not)]


def _restricted(full, keep, k):
    keep = set(keep)
    return {q: dict([(d, s) for d, s in full[q].items() if d in keep][:k]) for q in full}


def test_api_search_bm25_with_term_constraints(text, tmp_path):
    import sparse_rx
    j, tokens = text
    queries, n_docs, k = j["queries"], len(j["corpus"]), 10
    svc = sparse_rx.RetrievalService(device="cuda:0", tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    full = svc.search_bm25(queries, top_k=n_docs)
    n_cached = len(svc.query_cache)
    assert n_cached > 0
    must, any_, must_not = ["w3"], ["W5", "w7 w9"], ["w1"]
    keep = _satisfying(tokens, ["w3"], ["w5", "w7", "w9"], ["w1"])
    assert 5 < len(keep) < n_docs // 2
    got = svc.search_bm25(queries, top_k=k, must_terms=must, any_terms=any_, must_not_terms=must_not)
    exp = _restricted(full, keep, k)
    assert got == exp and [list(got[q]) for q in queries] == [list(exp[q]) for q in queries]
    assert any(len(got[q]) == k for q in queries) and any(got[q] != dict(list(full[q].items())[:k]) for q in queries)
    # the dict form: only the named qids are constrained
    got = svc.search_bm25(queries, top_k=k, must_terms={"q1": ["w3"]}, must_not_terms={"q2": ["w1", "w0"]})
    for q in queries:
        keep_q = _satisfying(tokens, ["w3"]) if q == "q1" else _satisfying(tokens, must_not=["w1", "w0"]) if q == "q2" else list(tokens)
        assert list(got[q].items()) == list(_restricted(full, keep_q, k)[q].items()), q
    # operators=True gives the dict of the keywords
    ops = {q: f"+w3 -w1 {t}" for q, t in queries.items() if t.strip()}
    plain = {q: f"w3 {t}" for q, t in queries.items() if t.strip()}
    got = svc.search_bm25(ops, top_k=k, operators=True)
    assert got == svc.search_bm25(plain, top_k=k, must_terms=["w3"], must_not_terms=["w1"]) and any(got.values())
    assert got == svc.search_bm25(ops, top_k=k, operators=True, must_terms={"q0": ["w3"]})  # merged with the keywords
    full_plain = svc.search_bm25(plain, top_k=n_docs)
    assert got == _restricted(full_plain, _satisfying(tokens, ["w3"], (), ["w1"]), k)
    n_cached = len(svc.query_cache)
    # with excluded_docs / allowed_docs as the base
    shown = _satisfying(tokens, ["w3"])[::2]
    got = svc.search_bm25(queries, top_k=k, must_terms=["w3"], excluded_docs=shown)
    assert got == _restricted(full, [d for d in _satisfying(tokens, ["w3"]) if d not in set(shown)], k) and any(got.values())
    third = list(tokens)[::3]
    got = svc.search_bm25(queries, top_k=k, must_not_terms={"q0": ["w0"]}, allowed_docs={"q0": third, "q3": third})
    for q in queries:
        keep_q = [d for d in third if "w0" not in tokens[d]] if q == "q0" else third if q == "q3" else list(tokens)
        assert list(got[q].items()) == list(_restricted(full, keep_q, k)[q].items()), q
    # an out-of-vocabulary must-term: no doc; in must_not it changes nothing
    assert svc.search_bm25(queries, top_k=k, must_terms=["nosuchword"]) == {q: {} for q in queries}
    assert svc.search_bm25(queries, top_k=k, must_not_terms=["nosuchword"]) == {q: dict(list(full[q].items())[:k]) for q in queries}
    # the constrained calls left the query cache alone
    assert len(svc.query_cache) == n_cached
    r = sparse_rx.OptimizedBM25Retriever(device="cuda:0", tile_log2=6)
    r.build_index_from_corpus(j["corpus"])
    assert r.search(queries, top_k=k, must_terms=must, any_terms=any_, must_not_terms=must_not) == exp and len(r.query_cache) == 0
    assert r.search(ops, top_k=k, operators=True) == svc.search_bm25(ops, top_k=k, operators=True)
    r.close()
    p = sparse_rx.OptimizedRetriever({"type": "bm25"}, device="cuda:0", tile_log2=6, cache_dir=str(tmp_path))
    p.build_index_from_corpus(j["corpus"])
    pk = p.search(queries, top_k=k, must_terms=must, any_terms=any_, must_not_terms=must_not)
    assert pk == _restricted(p.search(queries, top_k=n_docs), keep, k) and any(pk.values())  # its own accumulation order, its own floats
    p.close()
    svc.close()


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_api_vector_and_hybrid_with_term_constraints(text, storage):
    import sparse_rx
    j, tokens = text
    queries = dict(j["queries"])
    n_docs, dim = len(j["corpus"]), 96
    rng = np.random.default_rng(61)
    svc = sparse_rx.RetrievalService(device="cuda:0", tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    svc.set_embeddings(rng.standard_normal((n_docs, dim)).astype(np.float32), storage=storage)
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    kw = dict(must_terms=["w2"], any_terms=["w4", "w6"], must_not_terms=["w5"])
    keep = _satisfying(tokens, ["w2"], ["w4", "w6"], ["w5"])
    assert 5 < len(keep) < n_docs // 2
    # keyword-constrained vector search = the same call with the satisfying ids as allowed_docs
    for k, min_score in ((5, 0.0), (len(keep) + 3, -100.0)):
        got = svc.search_by_vector(vecs["q0"], k=k, min_score=min_score, **kw)
        assert got == svc.search_by_vector(vecs["q0"], k=k, min_score=min_score, allowed_docs=keep) and len(got) == min(k, len(keep))
        assert {r["doc_id"] for r in got} <= set(keep)
    assert svc.search_by_vector(vecs["q0"], k=5, must_terms=["nosuchword"]) == []
    # hybrid: both sides get the rows
    for extra in (dict(), dict(rescore=True), dict(mmr_lambda=0.5)):
        got = svc.search_hybrid(queries, vecs, top_k=10, candidates=20, **kw, **extra)
        assert got == svc.search_hybrid(queries, vecs, top_k=10, candidates=20, allowed_docs=keep, **extra), extra
        assert any(got.values()) and all(set(v) <= set(keep) for v in got.values())
    # with a doc filter as the base, and through the operators
    out = keep[::2]
    got = svc.search_hybrid(queries, vecs, top_k=10, candidates=20, excluded_docs=out, **kw)
    assert got == svc.search_hybrid(queries, vecs, top_k=10, candidates=20, allowed_docs=[d for d in keep if d not in set(out)])
    ops = {q: f"+w2 -w5 {t}" for q, t in queries.items() if t.strip()}
    plain = {q: f"w2 {t}" for q, t in queries.items() if t.strip()}
    got = svc.search_hybrid(ops, vecs, top_k=10, candidates=20, operators=True)
    assert got == svc.search_hybrid(plain, vecs, top_k=10, candidates=20, allowed_docs=_satisfying(tokens, ["w2"], (), ["w5"]))
    assert len(svc.query_cache) == 0
    svc.close()
