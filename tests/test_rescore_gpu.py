"""Hybrid rescoring on the GPU: the three dense "score these docs" kernels, srx_fuse_topk_scored and the rescore=True
doors against the NumPy restatement (tests/rescore_ref.py).  Every comparison is on doc ids, counts and fp32 score BITS."""
import json
import os

import numpy as np
import pytest

import hybrid_ref
import oracle
import rescore_ref
import sparse_rx
from oracle import np_oracle
from test_hybrid_gpu import SHAPES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _assert_bits(got, exp, tag):
    bad = np.argwhere(_bits(got) != _bits(exp))
    assert got.shape == exp.shape and len(bad) == 0, (tag, "first difference at", bad[:1], got[tuple(bad[0])] if len(bad) else None,
                                                      exp[tuple(bad[0])] if len(bad) else None)


# ---- one small harness per engine: build(rng, n_docs, dim, doc_base) -> (index, queries(rng, nq) -> device args, host restatement) ----
class _F32:
    def __init__(self, rng, n_docs, dim, doc_base=0, **kw):
        self.emb = rng.standard_normal((n_docs, dim)).astype(np.float32)
        self.ix = sparse_rx.DenseF32Index(self.emb, doc_base=doc_base)

    def queries(self, rng, nq):
        q = rng.standard_normal((nq, self.emb.shape[1])).astype(np.float32)
        return (_t(q),), lambda cd, cc: rescore_ref.f32_scores(self.emb, q, cd, cc, self.ix.doc_base)


class _U8:
    def __init__(self, rng, n_docs, dim, doc_base=0, **kw):
        self.c8, self.cs = sparse_rx.quantize_asymmetric(rng.standard_normal((n_docs, dim)).astype(np.float32))
        self.ix = sparse_rx.DenseUint8Index(self.c8, self.cs, doc_base=doc_base)

    def queries(self, rng, nq):
        qq = [sparse_rx.quantize_query_asymmetric(x) for x in rng.standard_normal((nq, self.c8.shape[1])).astype(np.float32)]
        self.host_queries = (np.stack([a for a, _ in qq]), np.stack([b for _, b in qq]))  # what the host door takes
        q = np.stack([sparse_rx.dense.dequantize_query_asymmetric(a, b) for a, b in qq]).astype(np.float32)
        return (_t(q),), lambda cd, cc: rescore_ref.u8_scores(self.c8, self.cs, q, cd, cc, self.ix.doc_base)


class _I8:
    def __init__(self, rng, n_docs, dim, doc_base=0, packed=True):
        self.c8 = rng.integers(-127, 128, (n_docs, dim), dtype=np.int8)
        self.cs = (rng.uniform(0.5, 1.5, n_docs) / 127).astype(np.float32)
        self.ix = sparse_rx.DenseInt8Index(self.c8, self.cs, doc_base=doc_base, packed=packed)

    def queries(self, rng, nq):
        q = rng.integers(-127, 128, (nq, self.c8.shape[1]), dtype=np.int8)
        qs = (rng.uniform(0.5, 1.5, nq) / 127).astype(np.float32)
        return (_t(q), _t(qs)), lambda cd, cc: rescore_ref.i8_scores(self.c8, self.cs, q, qs, cd, cc, self.ix.doc_base)


def _candidates(rng, ix, qargs, nq, m):
    """cand_doc i32[nq, m] / cand_count i32[nq]: rows the index's own search returns, random docs, the first and the last doc,
    repeats, -1, ids below doc_base and at or above doc_base + n_docs; counts shorter than m with live-looking junk behind
    them, a zero, a negative and an oversized count."""
    import torch
    n, base = ix.n_docs, ix.doc_base
    cand = (base + rng.integers(0, n, (nq, m))).astype(np.int64)
    kk = min(10, n, m)
    d, _, _ = ix.search_device(*qargs, kk)
    torch.cuda.synchronize()
    cand[:, :kk] = d.cpu().numpy()  # search rows (padded with -1 where fewer than kk docs score > 0)
    special = np.array([base, base + n - 1, -1, base - 1, base + n, base + n + 31, 2 ** 31 - 1, -2 ** 31, base + n // 2, base + n // 2])
    where = rng.random((nq, m)) < 0.3
    where[:, :kk] = False
    cand[where] = rng.choice(special, int(where.sum()))
    if m >= 65:
        cand[:, 63:65] = [base + n - 1, base]  # across the chunk boundary
    count = rng.integers(0, m + 1, nq).astype(np.int32)
    count[rng.integers(0, nq)] = m
    if nq >= 3:
        count[0], count[1], count[2] = 0, -7, m + 1000
    return cand.astype(np.int32), count


def _check_scores(h, rng, nq, m, tag):
    import torch
    qargs, ref = h.queries(rng, nq)
    cand, count = _candidates(rng, h.ix, qargs, nq, m)
    got = h.ix.score_docs_device(*qargs, _t(cand), _t(count))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (nq, m)
    exp = ref(cand, count)
    _assert_bits(got.cpu().numpy(), exp, (tag, nq, m))
    return exp


CASES = [(1, 1), (63, 3), (64, 5), (65, 257), (1500, 3), (1, 257), (64, 1)]  # (m, nq)


@pytest.mark.parametrize("n_docs", [33, 1000])
@pytest.mark.parametrize("dim", [64, 128, 1024])
@pytest.mark.parametrize("engine", [_F32, _U8])
def test_dense_score_rows_kernels(engine, dim, n_docs):
    rng = np.random.default_rng(dim + n_docs)
    h = engine(rng, n_docs, dim)
    live = 0
    for m, nq in CASES:
        live += int(np.count_nonzero(_check_scores(h, rng, nq, m, (engine.__name__, dim, n_docs))))
    assert live > 1000  # the comparison is not one of zeros


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("n_docs", [33, 1000])
@pytest.mark.parametrize("dim", [32, 96, 768, 1024])
def test_dense_score_i8_kernel(dim, n_docs, packed):
    rng = np.random.default_rng(dim + n_docs)
    h = _I8(rng, n_docs, dim, packed=packed)
    assert h.ix.packed is packed
    live = 0
    for m, nq in CASES:
        live += int(np.count_nonzero(_check_scores(h, rng, nq, m, ("i8", dim, n_docs, packed))))
    assert live > 1000


@pytest.mark.parametrize("engine,dim,kw", [(_F32, 192, {}), (_U8, 64, {}), (_I8, 192, {"packed": True}), (_I8, 64, {"packed": False})])
def test_dense_score_doc_base_null_count_and_out_reuse(engine, dim, kw):
    import torch
    rng = np.random.default_rng(dim)
    h = engine(rng, 1000, dim, doc_base=5000, **kw)
    assert h.ix.doc_base == 5000
    _check_scores(h, rng, 5, 130, "doc_base")
    qargs, ref = h.queries(rng, 4)
    cand, count = _candidates(rng, h.ix, qargs, 4, 70)
    got = h.ix.score_docs_device(*qargs, _t(cand))  # cand_count = NULL: every column counts
    torch.cuda.synchronize()
    _assert_bits(got.cpu().numpy(), ref(cand, None), "no cand_count")
    # out= reused on a non-default stream: every word is rewritten by each call
    out = torch.full((4, 70), float("nan"), device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        r1 = h.ix.score_docs_device(*qargs, _t(cand), _t(count), out=out)
        first = r1.clone()
        cand2 = np.ascontiguousarray(cand[:, ::-1])
        r2 = h.ix.score_docs_device(*qargs, _t(cand2), None, out=out)
    side.synchronize()
    assert r1 is out and r2 is out
    _assert_bits(first.cpu().numpy(), ref(cand, count), "out, first call")
    _assert_bits(out.cpu().numpy(), ref(cand2, None), "out, second call")
    # the host door validates and gives the same array
    host_queries = h.host_queries if engine is _U8 else [x.cpu().numpy() for x in qargs]  # u8: quantized queries + (scale, min)
    _assert_bits(h.ix.score_docs(*host_queries, cand, count), ref(cand, count), "host door")
    with pytest.raises(ValueError):
        h.ix.score_docs_device(*qargs, _t(cand).long())
    with pytest.raises(ValueError):
        h.ix.score_docs_device(*qargs, _t(cand[:3]))


def test_packed_corpus_is_the_restated_fragment_order():
    """what srx_dense_pack_i8 writes against rescore_ref.pack_i8, byte for byte: the layout the i8 restatement documents"""
    rng = np.random.default_rng(4)
    for n, dim in ((33, 32), (70, 96), (1000, 192), (40, 1024)):
        rows = rng.integers(-127, 128, (n, dim), dtype=np.int8)
        ix = sparse_rx.DenseInt8Index(rows, np.ones(n, np.float32), packed=True)
        assert np.array_equal(ix.corpus.cpu().numpy(), rescore_ref.pack_i8(rows)), (n, dim)


@pytest.mark.parametrize("kw", [{"quantization_method": "asymmetric"}, {"quantization_method": "symmetric"}, {"use_quantization": False}])
def test_quantized_embedding_retriever_score(kw):
    """the thin door on each of the mirror's three storage schemes: caller's order, restated bits"""
    r = sparse_rx.QuantizedEmbeddingRetriever("dpr", "m", embedding_dim=64, **kw)
    r.build_index_from_corpus({f"d{i}": {"text": "x"} for i in range(120)})
    qemb = {f"q{i}": r.query_embedding_from_seed(50 + i) for i in range(3)}
    cands = {"q0": ["d7", "d0", "d119"], "q1": ["d3"], "q2": []}
    got = r.score(qemb, cands)
    assert got["q2"] == {} and list(got["q0"]) == cands["q0"] and list(got["q1"]) == ["d3"]
    rows = np.array([[7, 0, 119], [3, -1, -1]], np.int32)
    e = [qemb["q0"], qemb["q1"]]
    if kw.get("use_quantization") is False:
        exp = rescore_ref.f32_scores(r.corpus_embeddings_fp32, np.stack(e), rows)
    elif kw["quantization_method"] == "symmetric":
        qq = [sparse_rx.quantize_query_symmetric(x) for x in e]
        exp = rescore_ref.i8_scores(r.corpus_embeddings_int8, r.corpus_scales, np.stack([a for a, _ in qq]), np.array([b for _, b in qq], np.float32), rows)
    else:
        qf = np.stack([sparse_rx.dense.dequantize_query_asymmetric(*sparse_rx.quantize_query_asymmetric(x)) for x in e])
        exp = rescore_ref.u8_scores(r.corpus_embeddings_int8, r.corpus_scales, qf, rows)
    for i, q in enumerate(("q0", "q1")):
        assert [np.float32(v).view(np.uint32) for v in got[q].values()] == [x.view(np.uint32) for x in exp[i, : len(cands[q])]], (kw, q)
    assert exp[0].all()
    with pytest.raises(ValueError, match="unknown doc id"):
        r.score(qemb, {"q0": ["nope"]})


@pytest.mark.parametrize("nq", [5, 257])
@pytest.mark.parametrize("engine,dim,kw", [(_F32, 1024, {}), (_F32, 128, {}), (_U8, 128, {}), (_I8, 96, {"packed": True}),
                                           (_I8, 768, {"packed": False})])
def test_a_search_row_scores_to_its_own_bits(engine, dim, kw, nq):
    import torch
    rng = np.random.default_rng(nq + dim)
    h = engine(rng, 1000, dim, **kw)
    qargs, _ = h.queries(rng, nq)
    for k in (10, 100):
        d, s, n = h.ix.search_device(*qargs, k)
        got = h.ix.score_docs_device(*qargs, d, n)
        torch.cuda.synchronize()
        assert int(n.min()) == k  # full rows: about half of 1 000 random docs score > 0
        _assert_bits(got.cpu().numpy(), s.cpu().numpy(), (engine.__name__, dim, nq, k))


# ---- srx_fuse_topk_scored ------------------------------------------------------------------------------------------------
def _others(rng, shape, plain):
    """what the opposite side says: the plain list-derived value, or -- two entries in five -- a positive value, a zero, a
    negative one, a NaN or a denormal"""
    kind = rng.integers(0, 10, shape)
    out = np.array(plain, np.float32)
    out[kind == 0] = rng.uniform(0.01, 40.0, int((kind == 0).sum()))
    out[kind == 1] = 0.0
    out[kind == 2] = -rng.uniform(0.01, 40.0, int((kind == 2).sum()))
    out[kind == 3] = np.nan
    out[kind == 4] = np.float32(1e-40) * rng.integers(1, 1000, int((kind == 4).sum())).astype(np.float32)
    return out


def _run_scored(a, a_other, b, b_other, k, weights=(0.3, 0.7)):
    import torch
    d, s, n = sparse_rx.fuse_scored_device(tuple(_t(x) for x in a), _t(a_other), tuple(_t(x) for x in b), _t(b_other), k, weights)
    torch.cuda.synchronize()
    return d.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()


def _check_scored(a, a_other, b, b_other, k, weights=(0.3, 0.7), tag=None):
    got = _run_scored(a, a_other, b, b_other, k, weights)
    exp = rescore_ref.fuse_scored(a, a_other, b, b_other, k, weights)
    tag = (tag, a[0].shape, b[0].shape, k, weights)
    assert got[0].shape == (len(a[2]), k) and got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert np.array_equal(got[2], exp[2]), (tag, got[2], exp[2])
    bad = np.nonzero((got[0] != exp[0]).any(axis=1) | (_bits(got[1]) != _bits(exp[1])).any(axis=1))[0]
    assert len(bad) == 0, (tag, "first differing query", int(bad[0]), got[0][bad[0]][:8], exp[0][bad[0]][:8], got[1][bad[0]][:8], exp[1][bad[0]][:8])
    return got


@pytest.mark.parametrize("ka,kb,k,form,nq", SHAPES)
def test_fuse_scored_shapes_and_overlaps(ka, kb, k, form, nq):
    assert hybrid_ref.form(ka, kb, k) == form  # the dispatch rule is the plain fusion's
    for overlap in (0.0, 0.5, 1.0):
        rng = np.random.default_rng(1000 * ka + kb + k + int(10 * overlap))
        a, b = hybrid_ref.make_lists(rng, nq, ka, kb, overlap=overlap)
        plain = rescore_ref.others_from_lists(a, b)
        a_other, b_other = _others(rng, a[0].shape, plain[0]), _others(rng, b[0].shape, plain[1])
        got = _check_scored(a, a_other, b, b_other, k, tag=("overlap", overlap))
        if overlap == 0.0:
            assert np.array_equal(got[2], np.minimum(k, a[2] + b[2]))  # every used entry has an own contribution > 0
        # the equivalence with the plain weighted fusion, on the device
        import torch
        same = _run_scored(a, plain[0], b, plain[1], k)
        d, s, n = sparse_rx.fuse_topk_device(tuple(_t(x) for x in a), tuple(_t(x) for x in b), k, mode="weighted", weights=(0.3, 0.7))
        torch.cuda.synchronize()
        assert np.array_equal(same[0], d.cpu().numpy()) and np.array_equal(same[2], n.cpu().numpy())
        assert np.array_equal(_bits(same[1]), _bits(s.cpu().numpy()))


@pytest.mark.parametrize("nq", [1, 5, 1000])
def test_fuse_scored_partly_filled_last_workgroup(nq):
    assert hybrid_ref.form(24, 16, 10) == "wave"  # four queries per workgroup in this form
    rng = np.random.default_rng(nq)
    a, b = hybrid_ref.make_lists(rng, nq, 24, 16, overlap=0.5)
    plain = rescore_ref.others_from_lists(a, b)
    _check_scored(a, _others(rng, a[0].shape, plain[0]), b, _others(rng, b[0].shape, plain[1]), 10)


@pytest.mark.parametrize("ka,kb,k", [(60, 70, 40), (600, 700, 400)])
def test_fuse_scored_empty_sides_zero_weights_and_wide_ranges(ka, kb, k):
    assert hybrid_ref.form(ka, kb, k) == ("wave" if ka == 60 else "block")
    rng = np.random.default_rng(ka)
    a, b = hybrid_ref.make_lists(rng, 6, ka, kb, overlap=0.5)
    a_other, b_other = (rng.uniform(0.0, 30.0, x[0].shape).astype(np.float32) for x in (a, b))  # every doc scores on both sides
    zero = lambda t: (t[0], t[1], np.zeros_like(t[2]))
    neg = lambda t: (t[0], t[1], np.full_like(t[2], -3))
    mixed = lambda t, m: (t[0], t[1], np.where(np.arange(len(t[2])) % m == 0, 0, t[2]).astype(np.int32))
    headless = lambda t: (np.where(np.arange(t[0].shape[1])[None, :] == 0, -1, t[0]).astype(np.int32), t[1], t[2])  # head doc = padding
    for aa, bb in ((zero(a), b), (a, zero(b)), (zero(a), zero(b)), (neg(a), b), (mixed(a, 2), mixed(b, 3)), (headless(a), b), (a, headless(b))):
        got = _check_scored(aa, a_other, bb, b_other, k, tag="empty side")
        if aa[2].max() <= 0 and bb[2].max() <= 0:
            assert not got[2].any() and np.all(got[0] == -1) and np.all(got[1] == 0)
    for w in ((0.0, 1.0), (2.5, 0.0), (1e-6, 1e5), (1.0, 1e-7)):
        _check_scored(a, a_other, b, b_other, k, weights=w, tag="weights")
    over = lambda t: (t[0], t[1], np.full_like(t[2], 5000))  # counts above the row width clamp to it
    a2, b2 = hybrid_ref.make_lists(rng, 4, ka, kb, overlap=0.3, fill=(1.0, 1.0), garbage=False)
    _check_scored(over(a2), a_other[:4], over(b2), b_other[:4], k, tag="count > width")
    # scores, weights and quotients into the denormals, which the contract keeps
    a, b = hybrid_ref.make_lists(rng, 6, ka, kb, overlap=0.5, score_range=(1e-20, 1e18))
    a_other, b_other = (np.exp(rng.uniform(np.log(1e-20), np.log(1e18), x[0].shape)).astype(np.float32) for x in (a, b))
    for w in ((1.0, 1.0), (1e-3, 1e-37), (1e-36, 1e-37)):
        _check_scored(a, a_other, b, b_other, k, weights=w, tag="denormal range")


@pytest.mark.parametrize("wide", [False, True])
def test_fuse_scored_duplicate_is_taken_from_list_a(wide):
    """doc 9 is in both lists and the two copies disagree about both scores: list A's copy decides, whatever it fuses to"""
    f = np.float32
    ka, kb, k = (2, 5, 10) if not wide else (700, 600, 200)
    assert hybrid_ref.form(ka, kb, k) == ("block" if wide else "wave")
    a_doc, b_doc = np.full((2, ka), -1, np.int32), np.full((2, kb), -1, np.int32)
    a_score, b_score, a_other, b_other = (np.zeros(s, f) for s in ((2, ka), (2, kb), (2, ka), (2, kb)))
    a_doc[:, :2], a_score[:, :2] = [5, 9], [2.0, 1.0]
    b_doc[:, :5], b_score[:, :5] = [9, 6, 4, 3, 8], [4.0, 2.0, 1.0, 0.5, 0.25]
    a_other[0, :2], b_other[:, :5] = [np.nan, 1.0], [2.0, -3.0, 0.0, 1e-45, np.nan]
    a_other[1, :2] = [0.5, -1.0]  # query 1: A's copy of doc 9 has no B contribution ...
    a = (a_doc, a_score, np.array([2, 2], np.int32))
    b = (b_doc, b_score, np.array([5, 5], np.int32))
    got = _check_scored(a, a_other, b, b_other, k, weights=(1.0, 1.0))
    assert got[0][0, :6].tolist() == [5, 9, 6, 4, 3, 8] and got[1][0, 1] == f(0.75) and got[2][0] == 6
    assert got[1][1, :3].tolist() == [1.125, 0.5, 0.5] and got[0][1, :3].tolist() == [5, 6, 9]
    got = _check_scored(a, a_other, b, b_other, k, weights=(0.0, 1.0))  # ... and with weight_a = 0 it fuses to +0: B's copy
    assert 9 not in got[0][1].tolist() and got[2][1] == 5               # (4 / 4) is dropped all the same


# ---- end to end through both doors ---------------------------------------------------------------------------------------
def _oracle_sparse(host, texts, k, k1=1.2, b=0.75):
    q_ptr, q_term, q_w = sparse_rx.encode_queries(texts, host.vocabulary)
    return oracle.search_batch(host.indptr, host.indices, host.data, host.doc_lengths, host.idf, q_ptr, q_term, q_w, k, k1, b, host.avgdl)


def _expected_rescored(sparse_all, dense_all, n_docs, cand, k, weights):
    """The rescore pipeline restated: both sides' scores of EVERY doc are given (sparse_all: the oracle's full-depth rows;
    dense_all f32[nq, n_docs]: the restated dense scores); the lists are their top `cand`, completed from the same tables."""
    nq = len(dense_all)
    bm25 = np.zeros((nq, n_docs), np.float32)
    for q in range(nq):
        bm25[q, sparse_all[0][q, : sparse_all[2][q]]] = sparse_all[1][q, : sparse_all[2][q]]
    a = np_oracle.dense_topk(bm25, cand)  # the engine's list contract: score > 0, (score desc, doc asc)
    b = np_oracle.dense_topk(dense_all, cand)
    other = lambda table, lst: np.where(lst[0] >= 0, np.take_along_axis(table, np.maximum(lst[0], 0).astype(np.int64), axis=1), 0).astype(np.float32)
    return rescore_ref.fuse_scored(a, other(dense_all, a), b, other(bm25, b), k, weights)


def _dicts_equal(got, qids, exp, doc_ids):
    ed, es, en = exp
    for i, qid in enumerate(qids):
        assert list(got[qid]) == [doc_ids[j] for j in ed[i, : en[i]]], qid  # dict order = rank order
        assert [np.float32(v).view(np.uint32) for v in got[qid].values()] == [x.view(np.uint32) for x in es[i, : en[i]]], qid


def _depth_independence(search, live, n_docs, expected):
    """(a), (b), (c) of the issue for one door: search(top_k, candidates, rescore) -> {qid: {doc: fused}}"""
    full_plain, full = search(n_docs, n_docs, False), search(n_docs, n_docs, True)
    for qid in live:  # (a) both lists complete: nothing to add, the same rows to the bit
        assert list(full[qid].items()) == list(full_plain[qid].items()), qid
    shallow = search(5, 5, True)
    expected(shallow, 5, 5)       # (b)
    expected(full, n_docs, n_docs)
    for qid in live:              # (c) the fused score of a returned doc does not depend on the depth
        assert len(shallow[qid]) == 5
        for doc, v in shallow[qid].items():
            assert np.float32(v).view(np.uint32) == np.float32(full[qid][doc]).view(np.uint32), (qid, doc)
    plain_shallow = search(5, 5, False)  # ... which the plain fusion does not give on this corpus
    moved = sum(np.float32(v).view(np.uint32) != np.float32(full_plain[qid][doc]).view(np.uint32)
                for qid in live for doc, v in plain_shallow[qid].items())
    assert moved > 0


def test_service_search_hybrid_rescore_end_to_end(golden_dir):
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    queries = dict(j["queries"])
    queries["blank"] = "   "
    queries["oov"] = "zzzunknown qqqmissing"
    dim, w = 96, (0.3, 0.7)
    rng = np.random.default_rng(11)
    svc = sparse_rx.RetrievalService()
    svc.build_bm25_index(j["corpus"])
    n_docs = len(j["corpus"])
    emb = rng.standard_normal((n_docs, dim)).astype(np.float32)
    svc.set_embeddings(emb)
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    live = [q for q in queries if queries[q].strip()]
    pad = lambda x: np.concatenate([x, np.zeros((x.shape[0], 128 - dim), np.float32)], axis=1)
    dense_all = rescore_ref.f32_scores(pad(emb), pad(np.stack([vecs[q] for q in live])), np.tile(np.arange(n_docs, dtype=np.int32), (len(live), 1)))
    sparse_all = _oracle_sparse(svc.host, [queries[q] for q in live], n_docs, svc.k1, svc.b)

    def search(top_k, cand, rescore):
        got = svc.search_hybrid(queries, vecs, top_k=top_k, sparse_weight=w[0], dense_weight=w[1], candidates=cand, rescore=rescore)
        assert list(got) == list(queries) and got["blank"] == {}
        return got

    _depth_independence(search, live, n_docs, lambda got, k, cand: _dicts_equal(got, live, _expected_rescored(sparse_all, dense_all, n_docs, cand, k, w), svc.doc_ids))
    assert len(search(5, 5, True)["oov"]) == 5  # no sparse side: the dense list alone
    # the thin door: the dense score of named docs, in the caller's order, to the bits of the restatement
    docs = [svc.doc_ids[i] for i in (7, 0, n_docs - 1, 7)]
    got = svc.score_by_vector({live[0]: vecs[live[0]], live[1]: vecs[live[1]], "none": vecs[live[2]]}, {live[0]: docs, live[1]: docs[:2], "none": []})
    assert got["none"] == {} and list(got[live[0]]) == [docs[0], docs[1], docs[2]] and list(got[live[1]]) == docs[:2]
    for qi in (0, 1):
        for d, v in got[live[qi]].items():
            assert np.float32(v).view(np.uint32) == dense_all[qi, svc.doc_ids.index(d)].view(np.uint32)
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.score_by_vector({live[0]: vecs[live[0]]}, {live[0]: ["no such doc"]})
    with pytest.raises(ValueError, match="rescore"):
        svc.search_hybrid(queries, vecs, fusion="rrf", rescore=True)
    svc.close()


def test_hybrid_retriever_rescore_end_to_end(golden_dir):
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    corpus, queries = j["corpus"], dict(j["queries"])
    queries["oov"] = "zzzunknown qqqmissing"
    queries["blank"] = ""
    dim, w, n_docs = 48, (0.3, 0.7), len(j["corpus"])
    r = sparse_rx.RetrieverRegistry.create({"type": "hybrid", "model": {"sparse": "bm25_custom", "dense": "dpr"},
                                            "params": {"sparse_weight": w[0], "dense_weight": w[1], "embedding_dim": dim, "rescore": True}})
    r.build_index_from_corpus(corpus, embeddings=np.random.default_rng(3).standard_normal((n_docs, dim)).astype(np.float32))
    assert r.rescore is True and r.dense._index.packed and r.dense._index.dim_pad == 64
    live = [q for q in queries if queries[q]]
    qemb = {qid: r.dense.query_embedding_from_seed(1000 + i) for i, qid in enumerate(live)}
    qq = [sparse_rx.quantize_query_symmetric(qemb[q]) for q in live]
    q8, qs = np.stack([a for a, _ in qq]), np.array([s for _, s in qq], np.float32)
    every = np.tile(np.arange(n_docs, dtype=np.int32), (len(live), 1))
    dense_all = rescore_ref.i8_scores(r.dense.corpus_embeddings_int8, r.dense.corpus_scales, q8, qs, every)
    sparse_all = _oracle_sparse(r.sparse.host, [queries[q] for q in live], n_docs)

    def search(top_k, cand, rescore):
        r.candidates, r.rescore = cand, rescore
        got = r.search(queries, top_k=top_k, query_embeddings=qemb)
        assert list(got) == list(queries) and got["blank"] == {}
        return got

    _depth_independence(search, live, n_docs, lambda got, k, cand: _dicts_equal(got, live, _expected_rescored(sparse_all, dense_all, n_docs, cand, k, w), r.doc_ids))
    # the thin door of the dense mirror
    docs = [r.doc_ids[i] for i in (3, n_docs - 1, 3)]
    got = r.dense.score({live[0]: qemb[live[0]], "none": qemb[live[1]]}, {live[0]: docs})
    assert got["none"] == {} and list(got[live[0]]) == docs[:2]
    for d, v in got[live[0]].items():
        assert np.float32(v).view(np.uint32) == dense_all[0, r.doc_ids.index(d)].view(np.uint32)
    with pytest.raises(ValueError, match="unknown doc id"):
        r.dense.score({live[0]: qemb[live[0]]}, {live[0]: ["no such doc"]})
    r.close()
