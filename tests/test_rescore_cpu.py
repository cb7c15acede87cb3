"""Hybrid rescoring without a GPU: the second header and its symbol table, every refusal of the four entry points (none
reaches a device), the NumPy restatement (tests/rescore_ref.py) against the oracle's similarities on the golden dense
fixtures and against the plain fusion's restatement, and the Python doors' argument checks."""
import os
import re

import numpy as np
import pytest

import hybrid_ref
import rescore_ref
import sparse_rx
from oracle import np_oracle
from sparse_rx import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 29, 1 << 30]  # never dereferenced


def test_second_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "sparse_rx_rescore.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_capi.RESCORE_SYMBOLS) and len(declared) == 4, declared ^ set(_capi.RESCORE_SYMBOLS)
    assert '#include "sparse_rx.h"' in hdr
    assert not set(_capi.RESCORE_SYMBOLS) & set(_capi.SYMBOLS)
    assert "dense_score.hip" in _capi.SOURCES
    L = _capi.lib()
    for name, (res, args) in _capi.RESCORE_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name


def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg, (rc, msg)


def test_dense_score_f32_refusals():
    f = _capi.lib().srx_dense_score_docs_f32
    ok = dict(device=0, emb=P[0], n_docs=100, dim=64, queries=P[1], nq=2, doc_base=0, cand_doc=P[2], cand_count=None, m=5, out=P[3], stream=None)
    call = lambda **kw: f(*{**ok, **kw}.values())
    _refused(call(nq=-1), "nq < 0")
    _refused(call(m=0), "m must be")
    _refused(call(nq=1 << 20, m=1 << 20), "int32")
    for dim in (0, 48, 1088, -64):
        _refused(call(dim=dim), "multiple of 64")
    for n_docs in (0, -5, 2 ** 31 - 1):
        _refused(call(n_docs=n_docs), "n_docs")
    for null in ("emb", "queries", "cand_doc", "out"):
        _refused(call(**{null: None}), "null pointer")
    assert call(nq=0, emb=None, queries=None, cand_doc=None, out=None) == 0  # nothing to do: no launch
    assert b"srx_dense_score_docs_f32" in _capi.lib().srx_last_error()  # the last refusal's text names the entry point


def test_dense_score_u8_refusals():
    f = _capi.lib().srx_dense_score_docs_u8
    ok = dict(device=0, corpus=P[0], scales=P[4], n_docs=100, dim=128, queries=P[1], nq=2, doc_base=0, cand_doc=P[2], cand_count=None, m=5,
              out=P[3], stream=None)
    call = lambda **kw: f(*{**ok, **kw}.values())
    _refused(call(nq=-1), "nq < 0")
    _refused(call(m=-1), "m must be")
    _refused(call(nq=65536, m=65536), "int32")
    for dim in (32, 96, 2048):
        _refused(call(dim=dim), "multiple of 64")
    _refused(call(n_docs=0), "n_docs")
    for null in ("corpus", "scales", "queries", "cand_doc", "out"):
        _refused(call(**{null: None}), "null pointer")
    assert call(nq=0, corpus=None, scales=None) == 0
    assert b"srx_dense_score_docs_u8" in _capi.lib().srx_last_error()


def test_dense_score_i8_refusals():
    f = _capi.lib().srx_dense_score_docs_i8
    ok = dict(device=0, corpus=P[0], packed=1, cscale=P[4], n_docs=100, dim=96, queries=P[1], qscale=P[5], nq=2, doc_base=0, cand_doc=P[2],
              cand_count=None, m=5, out=P[3], stream=None)
    call = lambda **kw: f(*{**ok, **kw}.values())
    _refused(call(nq=-1), "nq < 0")
    _refused(call(m=0), "m must be")
    _refused(call(nq=1 << 16, m=1 << 15), "int32")
    for dim in (0, 48, 160, 640, 2048):  # 160 and 640 are multiples of 32 the INT8 engine has no instance for
        _refused(call(dim=dim), "dim must be")
    _refused(call(n_docs=0), "n_docs")
    for packed in (2, -1):
        _refused(call(packed=packed), "packed")
    for null in ("corpus", "cscale", "queries", "qscale", "cand_doc", "out"):
        _refused(call(**{null: None}), "null pointer")
    _refused(call(corpus=P[0] + 8), "aligned")
    _refused(call(queries=P[1] + 4), "aligned")
    assert call(nq=0, corpus=None) == 0
    assert call(nq=1 << 15, m=1 << 15, n_docs=0) == -1  # nq * m = 2^30 fits; n_docs is what is refused


def test_fuse_scored_refusals():
    f = _capi.lib().srx_fuse_topk_scored
    ok = dict(device=0, a_doc=P[0], a_score=P[1], a_other=P[2], a_count=P[3], ka=10, b_doc=P[4], b_score=P[5], b_other=P[6], b_count=P[7],
              kb=10, nq=3, k=5, wa=0.3, wb=0.7, out_doc=P[8], out_score=P[9], out_count=P[10], stream=None)
    call = lambda **kw: f(*{**ok, **kw}.values())
    _refused(call(nq=-1), "nq < 0")
    for kw in (dict(ka=0), dict(ka=1025), dict(kb=0), dict(kb=1025)):
        _refused(call(**kw), "ka / kb")
    for k in (0, 1025):
        _refused(call(k=k), "k must be")
    for kw in (dict(wa=-1.0), dict(wb=float("nan")), dict(wa=float("inf"))):
        _refused(call(**kw), "finite")
    _refused(call(wa=0.0, wb=0.0), "both weights")
    for null in ("a_doc", "a_score", "a_other", "a_count", "b_doc", "b_score", "b_other", "b_count", "out_doc", "out_score", "out_count"):
        _refused(call(**{null: None}), "null pointer")
    assert call(nq=0, a_doc=None, out_doc=None) == 0


# ---- the dense restatement against the oracle's similarities on the golden fixtures -------------------------------------------
def _pad(x, dim_pad):
    out = np.zeros((x.shape[0], dim_pad), x.dtype)
    out[:, : x.shape[1]] = x
    return out


def _all_docs(nq, n_docs):
    return np.tile(np.arange(n_docs, dtype=np.int32), (nq, 1))


def test_i8_restatement_is_the_oracle_bit_for_bit(golden_dir):
    z = np.load(os.path.join(golden_dir, "dense_int8.npz"))
    sims = np_oracle.int8_similarities(z["query_int8"], z["corpus_int8"], z["query_scales"], z["corpus_scales"])
    nq, n = sims.shape
    rng = np.random.default_rng(5)
    cand = np.concatenate([_all_docs(nq, n), rng.integers(0, n, (nq, 40)).astype(np.int32)], axis=1)  # every doc, then repeats
    got = rescore_ref.i8_scores(_pad(z["corpus_int8"], 64), z["corpus_scales"], _pad(z["query_int8"], 64), z["query_scales"], cand)
    exp = np.take_along_axis(sims, cand.astype(np.int64), axis=1)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(exp[:, :n].view(np.uint32), z["similarities"].view(np.uint32))  # and the reference's own rows
    # padding, ids outside the index and doc_base
    cand2 = np.array([[5, -1, n, 7, 7, 2 ** 31 - 1001, -2 ** 31, 0]] * nq, np.int32)
    cnt = np.array([8, 0, -3, 4, 100] + [8] * (nq - 5), np.int32)
    got = rescore_ref.i8_scores(z["corpus_int8"], z["corpus_scales"], z["query_int8"], z["query_scales"], cand2 + 1000, cnt, doc_base=1000)
    for q in range(nq):
        for c in range(8):
            d = int(cand2[q, c])
            live = c < max(int(cnt[q]), 0) and 0 <= d < n
            assert got[q, c].view(np.uint32) == (sims[q, d].view(np.uint32) if live else 0), (q, c)
    assert got[0, 0] != 0 and not got[1].any() and not got[2].any() and got[3, 4] == 0 and got[4, 7] != 0


def test_packed_layout_restatement_is_a_permutation_of_the_rows():
    rng = np.random.default_rng(2)
    for n, dim in ((33, 32), (70, 96), (5, 1024)):
        rows = rng.integers(-127, 128, (n, dim), dtype=np.int8)
        packed = rescore_ref.pack_i8(rows)
        assert packed.size == _capi.lib().srx_dense_packed_bytes(n, dim)
        offs = np.concatenate([rescore_ref.packed_offsets(d, dim) for d in range(n)])
        assert len(set(offs.tolist())) == len(offs) and offs.max() + 16 <= packed.size and np.all(offs % 16 == 0)
        assert packed.astype(np.int64).sum() == rows.astype(np.int64).sum()


def test_f32_and_u8_restatements_agree_with_the_oracle(golden_dir):
    """The summation order of the reference's BLAS dot is unspecified, so -- as tests/test_dense_int8.py does for these two
    engines -- f32: within 1e-5 * sum |e_i| |q_i| of the float64 value; u8: rtol 1e-5, atol 1e-6 * max |similarity|."""
    z = np.load(os.path.join(golden_dir, "dense_int8.npz"))
    emb, qemb = z["emb"], z["qemb"]
    nq, n = len(qemb), len(emb)
    got = rescore_ref.f32_scores(_pad(emb, 64), _pad(qemb, 64), _all_docs(nq, n))
    exact = qemb.astype(np.float64) @ emb.astype(np.float64).T
    tol = 1e-5 * (np.abs(qemb.astype(np.float64)) @ np.abs(emb.astype(np.float64)).T)
    assert np.all(np.abs(got - exact) <= tol + 1e-12)
    assert np.all(np.abs(got - np_oracle.f32_similarities(emb, qemb)) <= tol + 1e-12)
    a = np.load(os.path.join(golden_dir, "dense_uint8_asym.npz"))
    qf = np.stack([sparse_rx.dense.dequantize_query_asymmetric(q, s) for q, s in zip(a["query_uint8"], a["query_scales"])])
    got = rescore_ref.u8_scores(_pad(a["corpus_uint8"], 64), a["corpus_scales"], _pad(qf, 64), _all_docs(nq, n))
    sims = np_oracle.uint8_asymmetric_similarities(a["query_uint8"], a["query_scales"], a["corpus_uint8"], a["corpus_scales"])
    assert np.allclose(got, sims, rtol=1e-5, atol=1e-6 * float(np.max(np.abs(sims))))
    assert np.allclose(got, a["similarities"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(a["similarities"]))))


def test_lane_dot_is_order_sensitive_and_never_minus_zero():
    """the restatement really is the lane order (a plain fp32 sum differs somewhere), and a sum that starts at +0 is never -0"""
    rng = np.random.default_rng(0)
    e, q = rng.standard_normal((500, 256)).astype(np.float32), rng.standard_normal(256).astype(np.float32)
    got = rescore_ref.lane_dot(e, q)
    naive = np.array([np.float32(sum(np.float32(x * y) for x, y in zip(r, q))) for r in e[:50]], np.float32)
    assert np.any(got[:50].view(np.uint32) != naive.view(np.uint32))
    assert np.allclose(got, e.astype(np.float64) @ q.astype(np.float64), rtol=1e-4, atol=1e-4)
    z = rescore_ref.lane_dot(-np.abs(e) * 0, np.abs(q))  # every product is -0
    assert np.all(z.view(np.uint32) == 0)


# ---- the fusion restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ka,kb,k,overlap", [(10, 10, 10, 0.5), (60, 70, 40, 0.0), (60, 70, 200, 1.0), (300, 200, 128, 0.5)])
def test_fuse_scored_with_list_scores_is_the_plain_weighted_fusion(ka, kb, k, overlap):
    rng = np.random.default_rng(ka + kb)
    a, b = hybrid_ref.make_lists(rng, 6, ka, kb, overlap=overlap)
    a_other, b_other = rescore_ref.others_from_lists(a, b)
    for w in ((0.3, 0.7), (0.0, 1.0), (2.5, 0.0), (1e-3, 1e4)):
        got = rescore_ref.fuse_scored(a, a_other, b, b_other, k, w)
        exp = hybrid_ref.fuse(a, b, k, "weighted", w)
        assert np.array_equal(got[2], exp[2]) and np.array_equal(got[0], exp[0]), w
        assert np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32)), w
    if overlap == 0.5:
        assert (a_other > 0).any() and (a_other == 0).any()


def test_fuse_scored_side_without_a_used_head_contributes_nothing():
    f = np.float32
    a = (np.array([[1, 2, 3]], np.int32), np.array([[4.0, 2.0, 1.0]], f), np.array([3], np.int32))
    b = (np.array([[7, 2, 8]], np.int32), np.array([[8.0, 4.0, 2.0]], f), np.array([3], np.int32))
    a_other, b_other = np.array([[1.0, 4.0, 0.0]], f), np.array([[0.5, 2.0, 1.0]], f)

    def run(aa, bb, w=(1.0, 1.0)):
        d, s, n = rescore_ref.fuse_scored(aa, a_other, bb, b_other, 10, w)
        assert np.all(d[0, n[0]:] == -1) and np.all(s[0, n[0]:] == 0)
        return dict(zip(d[0, : n[0]].tolist(), s[0, : n[0]].tolist()))

    assert run(a, b) == {1: 1.0 + 1.0 / 8.0, 2: 0.5 + 0.5, 3: 0.25, 7: 0.5 / 4.0 + 1.0, 8: 0.25 + 0.25}
    # side B without a normaliser: neither its own entries' scores nor a_other count.  An entry of B that is still used (own
    # score > 0) carries what side A gives it through b_other, and one whose doc list A holds is still dropped
    only_a = {1: 1.0, 2: 0.5, 3: 0.25}
    assert run(a, (np.array([[-1, 2, 8]], np.int32), b[1], b[2])) == {**only_a, 8: 0.25}   # the head's doc is padding
    assert run(a, (b[0], np.array([[0.0, 4.0, 2.0]], f), b[2])) == {**only_a, 8: 0.25}     # the head's own score is not > 0
    assert run(a, (b[0], b[1], np.array([0], np.int32))) == only_a                         # an empty list
    # side A without one: A's used entries still rank, with what side B gives them through a_other
    assert run((np.array([[-1, 2, 3]], np.int32), a[1], a[2]), b) == {2: 0.5, 7: 1.0, 8: 0.25}
    assert run((a[0], a[1], np.array([0], np.int32)), (b[0], b[1], np.array([0], np.int32))) == {}
    # a zero weight is a contribution of +0, not a missing side
    assert run(a, b, (0.0, 2.0)) == {1: 0.25, 2: 1.0, 7: 2.0, 8: 0.5}


def test_fuse_scored_takes_a_doc_in_both_lists_from_a_and_ignores_bad_others():
    f = np.float32
    a = (np.array([[5, 9]], np.int32), np.array([[2.0, 1.0]], f), np.array([2], np.int32))
    b = (np.array([[9, 6, 4, 3, 8]], np.int32), np.array([[4.0, 2.0, 1.0, 0.5, 0.25]], f), np.array([5], np.int32))
    a_other = np.array([[np.nan, 1.0]], f)                      # A says doc 9 scores 1.0 on side B; B's own entry says 4.0
    b_other = np.array([[2.0, -3.0, 0.0, 1e-45, np.nan]], f)    # negative, zero, a denormal, NaN
    got = rescore_ref.fuse_scored(a, a_other, b, b_other, 10, (1.0, 1.0))
    n = got[2][0]
    res = dict(zip(got[0][0, :n].tolist(), got[1][0, :n]))
    assert res[9] == f(0.5) + f(0.25)                           # list A's copy: 1/2 + 1/4, not B's 2/2 + 4/4
    assert res[5] == f(1.0)                                     # a NaN other score does not contribute
    assert res[6] == f(0.5) and res[4] == f(0.25)               # negative and zero do not contribute
    assert res[3] == f(f(1e-45) / f(2.0)) + f(0.125) and res[8] == f(0.0625)  # the denormal does (its quotient underflows to +0)
    assert got[0][0, :n].tolist() == [5, 9, 6, 4, 3, 8]


# ---- the Python doors ----------------------------------------------------------------------------------------------------
def test_rescore_with_rrf_is_refused_before_the_index_checks():
    svc = sparse_rx.RetrievalService()
    q, v = {"a": "hello"}, {"a": np.ones(64, np.float32)}
    with pytest.raises(ValueError, match="rescore"):
        svc.search_hybrid(q, v, fusion="rrf", rescore=True)
    with pytest.raises(ValueError, match="BM25 index not built"):  # the weighted mode gets as far as the index check
        svc.search_hybrid(q, v, rescore=True)
    with pytest.raises(ValueError, match="rescore"):
        sparse_rx.RetrieverRegistry.create({"type": "hybrid", "params": {"fusion": "rrf", "rescore": True}})
    r = sparse_rx.RetrieverRegistry.create({"type": "hybrid", "params": {"rescore": True, "candidates": 50}})
    assert r.rescore is True and r.fusion == "weighted"
    assert sparse_rx.RetrieverRegistry.create({"type": "hybrid"}).rescore is False
    r.fusion = "rrf"  # plain attributes: the combination is checked again where it is used
    with pytest.raises(ValueError, match="rescore"):
        r.search({"q": "hello"})
    r.fusion = "weighted"
    with pytest.raises(ValueError, match="Index not built"):
        r.search({"q": "hello"})
    from sparse_rx.index import hybrid_search
    with pytest.raises(ValueError, match="rescore"):
        hybrid_search(None, None, None, None, None, 5, 5, 5, "rrf", (0.3, 0.7), 60.0, rescore=True)
    with pytest.raises(ValueError, match="Index not built"):
        sparse_rx.QuantizedEmbeddingRetriever("dpr", "m").score({"q": np.ones(8, np.float32)}, {"q": ["d"]})
    with pytest.raises(ValueError, match="No embedding index"):
        svc.score_by_vector(v, {"a": ["d"]})
