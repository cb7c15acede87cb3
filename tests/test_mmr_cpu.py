"""The MMR selection without a GPU: the sixth header and its symbol table, the frozen counts of the other five, every refusal
of the three entry points (none reaches a device), the Python layer's ValueErrors, the NumPy restatement (tests/mmr_ref.py)
pinned by a second, naive fp64 restatement on inputs where both are exact, and the plumbing of the service keywords with the
launches replaced by recorders."""
import os
import re

import numpy as np
import pytest

import mmr_ref
import sparse_rx
from sparse_rx import _capi
from sparse_rx.dense import DenseF32Index, DenseHalfIndex, DenseInt8Index, DenseUint8Index, check_mmr_args, check_mmr_shape
from sparse_rx.index import mmr_pool_depth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(12)]  # 16-byte aligned addresses, never dereferenced


def test_sixth_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "sparse_rx_mmr.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_capi.MMR_SYMBOLS) and len(declared) == 3, declared ^ set(_capi.MMR_SYMBOLS)
    assert '#include "sparse_rx.h"' in hdr and "has no diversification" in hdr
    others = (_capi.SYMBOLS, _capi.RESCORE_SYMBOLS, _capi.QUANT_SYMBOLS, _capi.FILTER_SYMBOLS, _capi.HALF_SYMBOLS)
    for other in others:
        assert not set(_capi.MMR_SYMBOLS) & set(other)
    assert tuple(len(t) for t in others) == (35, 4, 4, 8, 5)  # the new entry points are a table of their own: 59 in six headers
    assert "mmr.hip" in _capi.SOURCES
    deps = [os.path.basename(p) for p in _capi._deps()]
    assert "sparse_rx_mmr.h" in deps and "mmr_common.h" in deps and "mmr.hip" in deps
    L = _capi.lib()
    assert L.srx_version() == 301
    for name, (res, args) in _capi.MMR_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    assert len(_capi.MMR_SYMBOLS["srx_mmr_select_f32"][1]) == 22 and len(_capi.MMR_SYMBOLS["srx_mmr_select_half"][1]) == 23
    assert (_capi.SRX_MMR_DOT, _capi.SRX_MMR_COSINE) == (0, 1) == (mmr_ref.DOT, mmr_ref.COSINE)
    assert re.search(r"SRX_MMR_DOT = 0, SRX_MMR_COSINE = 1", hdr)
    assert int(re.search(r"#define SRX_MMR_MAX_M (\d+)", hdr).group(1)) == _capi.SRX_MMR_MAX_M == mmr_ref.MAX_M == 256
    for name in ("check_mmr_args", "mmr_pool_depth"):
        assert name in sparse_rx.__all__ and callable(getattr(sparse_rx, name))


def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg, (rc, word, msg)


def test_workspace_bytes():
    L = _capi.lib()
    for args in ((-1, 10), (1, 0), (1, 257), (1, -3)):
        _refused(L.srx_mmr_workspace_bytes(*args), "srx_mmr_workspace_bytes")
    for nq, m in ((0, 1), (1, 1), (5, 33), (1024, 128), (1024, 256)):
        got = L.srx_mmr_workspace_bytes(nq, m)
        assert nq * m * m * 4 <= got <= nq * m * m * 4 + 256
    assert L.srx_mmr_workspace_bytes(1024, 256) == 256 * (1 << 20) + 256  # the most one call of the Python layer asks for


def _calls(L):
    ok = dict(device=0, corpus=P[0], n_docs=1000, dim=64, doc_base=0, cand_doc=P[1], cand_rel=P[2], cand_count=P[3], nq=2, m=8, k=4, sim=1,
              w_rel=0.5, w_div=0.5, out_doc=P[4], out_rel=P[5], out_mmr=P[6], out_count=P[7], out_sim=None, ws=P[8], ws_bytes=1 << 30, stream=None)
    f32 = lambda **kw: L.srx_mmr_select_f32(*{**ok, **kw}.values())

    def half(type_):
        def call(**kw):
            a = {**ok, **kw}
            return L.srx_mmr_select_half(a.pop("device"), a.pop("type", type_), *a.values())
        return call
    return [("srx_mmr_select_f32", f32), ("srx_mmr_select_half", half(0)), ("srx_mmr_select_half", half(1))]


def test_select_refusals():
    L = _capi.lib()
    for who, call in _calls(L):
        for m in (0, -1, 257):
            _refused(call(m=m, k=1), "m must be")
        for k in (0, -1, 9):
            _refused(call(k=k), "k must be")
        for s in (-1, 2, 7):
            _refused(call(sim=s), "sim_mode")
        for w in (-0.5, float("nan"), float("inf"), -float("inf")):
            _refused(call(w_rel=w), "weights must be finite")
            _refused(call(w_div=w), "weights must be finite")
        _refused(call(w_rel=0.0, w_div=0.0), "both 0")
        for d in (0, 32, 96, 1088, -64):
            _refused(call(dim=d), "multiple of 64")
        for n in (0, -1, 2 ** 31 - 1):
            _refused(call(n_docs=n), "n_docs")
        _refused(call(doc_base=-1), "doc_base")
        _refused(call(nq=-1), "nq < 0")
        _refused(call(nq=2 ** 24, m=256, k=1), "nq * m")
        for null in ("corpus", "cand_doc", "cand_rel", "out_doc", "out_rel", "out_count"):
            _refused(call(**{null: None}), "null pointer")
        assert who.encode() in L.srx_last_error()
        assert call(ws=None) == -3 and call(ws_bytes=2 * 8 * 8 * 4) == -3  # SRX_ERR_NOMEM: the alignment slack is part of the size
        assert b"workspace" in L.srx_last_error()
        assert call(out_sim=P[9], ws=P[9], ws_bytes=2 * 8 * 8 * 4 - 1) == -3  # out_sim as the workspace: exactly the Gram bytes are enough
        # nothing to do: no launch, whatever the pointers; a single zero weight, a NULL count, out_mmr and out_sim are legal
        assert call(nq=0, corpus=None, cand_doc=None, cand_rel=None, out_doc=None, out_rel=None, out_count=None, ws=None, ws_bytes=0) == 0
        assert call(nq=0, w_rel=0.0, w_div=1.0, cand_count=None, out_mmr=None) == 0 and call(nq=0, w_rel=1.0, w_div=0.0, m=256, k=256, dim=1024) == 0
    half = _calls(L)[1][1]
    for t in (-1, 2, 7):
        _refused(half(type=t), "type must be")
    _refused(half(corpus=P[0] + 8), "16-byte aligned")
    assert _calls(L)[0][1](corpus=P[0] + 4, ws=None) == -3  # the f32 rows need no 16-byte alignment: the call gets as far as the workspace


def test_python_value_errors():
    assert check_mmr_args(0.5, "cosine") == (1, 0.5, 0.5) and check_mmr_args(1, "DOT") == (0, 1.0, 0.0) and check_mmr_args(0.0, "dot") == (0, 0.0, 1.0)
    sim, w_rel, w_div = check_mmr_args(0.3, "cosine")
    assert (np.float32(w_rel), np.float32(w_div)) == (np.float32(0.3), np.float32(1.0 - 0.3)) == mmr_ref.weights(0.3)
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="lambda"):
            check_mmr_args(bad, "cosine")
    for bad in ("l2", "", None, "cos"):
        with pytest.raises(ValueError, match="similarity must be"):
            check_mmr_args(0.5, bad)
    assert check_mmr_shape(256, 256) == 256 and check_mmr_shape(1, 1) == 1
    for m, k in ((257, 1), (0, 1)):
        with pytest.raises(ValueError, match="candidates per query"):
            check_mmr_shape(m, k)
    for m, k in ((10, 0), (10, 11), (10, -1)):
        with pytest.raises(ValueError, match="k must be"):
            check_mmr_shape(m, k)
    assert mmr_pool_depth(10, None, 10 ** 6) == 40 and mmr_pool_depth(100, None, 10 ** 6) == 256 and mmr_pool_depth(10, None, 25) == 25
    assert mmr_pool_depth(10, 256, 10 ** 6) == 256 and mmr_pool_depth(10, 5, 10 ** 6) == 5 and mmr_pool_depth(300, None, 10 ** 6) == 256
    for bad in (257, 0, -1, 1000):
        with pytest.raises(ValueError, match="mmr_pool"):
            mmr_pool_depth(10, bad, 10 ** 6)
    # the methods exist on the two indexes that keep rows, and only there
    for cls in (DenseF32Index, DenseHalfIndex):
        assert callable(cls.mmr_device) and callable(cls.mmr)
    for cls in (DenseInt8Index, DenseUint8Index, sparse_rx.QuantizedEmbeddingIndex, sparse_rx.HybridRetriever, sparse_rx.ShardedSearcher,
                sparse_rx.HostBatchPipeline):
        assert not hasattr(cls, "mmr_device") and not hasattr(cls, "mmr") and not hasattr(cls, "diversify")


def test_index_methods_check_before_any_launch():
    import torch
    for cls in (DenseF32Index, DenseHalfIndex):
        ix = cls.__new__(cls)  # no device behind it: every check below comes before the library is touched
        ix.device = torch.device("cpu")
        d = torch.zeros((2, 300), dtype=torch.int32)
        with pytest.raises(ValueError, match="candidates per query"):
            ix.mmr_device(d, d.float(), None, 10)
        with pytest.raises(ValueError, match="candidates per query"):
            ix.mmr(np.zeros((2, 257), np.int32), np.zeros((2, 257), np.float32), None, 10)
        d = torch.zeros((2, 8), dtype=torch.int32)
        with pytest.raises(ValueError, match="k must be"):
            ix.mmr_device(d, d.float(), None, 9)
        with pytest.raises(ValueError, match="lambda"):
            ix.mmr_device(d, d.float(), None, 4, lambda_=1.5)
        with pytest.raises(ValueError, match="similarity must be"):
            ix.mmr_device(d, d.float(), None, 4, similarity="l2")
        with pytest.raises(ValueError, match="cand_doc must be an int32"):
            ix.mmr_device(d.long(), d.float(), None, 4)
        with pytest.raises(ValueError, match="cand_rel"):
            ix.mmr_device(d, d.double(), None, 4)
        with pytest.raises(ValueError, match="cand_rel"):
            ix.mmr_device(d, d.float()[:, :4], None, 4)
        with pytest.raises(ValueError, match="cand_count"):
            ix.mmr_device(d, d.float(), torch.zeros(3, dtype=torch.int32), 4)
        with pytest.raises(ValueError, match="cand_rel must have"):
            ix.mmr(np.zeros((2, 8), np.int32), np.zeros((2, 7), np.float32), None, 4)
        with pytest.raises(ValueError, match="2-D integer"):
            ix.mmr(np.zeros((2, 8), np.float32), np.zeros((2, 8), np.float32), None, 4)


# ---- the restatement, pinned by a second one ---------------------------------------------------------------------------------
def _dyadic_case(seed, m, dim, lam):
    """Rows in {-3 .. 3}, relevances j / 64: every product, sum and difference of a dot-mode selection is representable."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-3, 4, (m, dim)).astype(np.float64)
    rows[m // 2] = rows[0]  # a copy of another row
    rel = rng.integers(-64, 65, m).astype(np.float64) / 64
    rel[m // 3] = rel[0]    # equal relevances: the tie rule decides
    live = rng.random(m) > 0.15
    live[0] = True
    return mmr_ref.gram_exact(rows), rel, live, mmr_ref.weights(lam)


@pytest.mark.parametrize("lam", [0.25, 0.5, 0.75, 0.0, 1.0])
@pytest.mark.parametrize("m,dim,k", [(1, 8, 1), (7, 16, 7), (40, 64, 12), (130, 32, 130)])
def test_restatement_against_naive_fp64_dot(lam, m, dim, k):
    G, rel, live, (w_rel, w_div) = _dyadic_case(m * 1000 + dim, m, dim, lam)
    assert np.array_equal(G.astype(np.float32).astype(np.float64), G)
    got, got_v = mmr_ref.select(G, rel, live, k, w_rel, w_div, mmr_ref.DOT)
    exp, exp_v = mmr_ref.select_naive_f64(G, rel, live, k, w_rel, w_div, mmr_ref.DOT)
    assert got == exp and len(got) == min(k, int(live.sum())) and all(live[c] for c in got) and len(set(got)) == len(got)
    assert got_v.dtype == np.float32 and np.array_equal(got_v.astype(np.float64), exp_v)


@pytest.mark.parametrize("lam", [0.25, 0.5, 1.0])
def test_restatement_against_naive_fp64_cosine(lam):
    """Cosine mode is exact when every norm is a power of two: rows with exactly four entries of +-2^e (norm 2^(e + 1))."""
    rng = np.random.default_rng(77)
    m, dim = 24, 16
    rows = np.zeros((m, dim))
    for a in range(m):
        rows[a, rng.choice(dim, 4, replace=False)] = rng.choice([-1.0, 1.0], 4) * 2.0 ** rng.integers(-2, 3)
    rows[5] = rows[2]
    rows[9] = 0.0  # an all-zero row: its similarity to everything is +0
    rel = rng.integers(0, 65, m).astype(np.float64) / 64
    live = np.ones(m, bool)
    live[3] = False
    G = mmr_ref.gram_exact(rows)
    w_rel, w_div = mmr_ref.weights(lam)
    got, got_v = mmr_ref.select(G, rel, live, m, w_rel, w_div, mmr_ref.COSINE)
    exp, exp_v = mmr_ref.select_naive_f64(G, rel, live, m, w_rel, w_div, mmr_ref.COSINE)
    assert got == exp and len(got) == m - 1 and 3 not in got
    assert np.array_equal(got_v.astype(np.float64), exp_v)


def test_restatement_by_hand():
    # three docs: 0 and 1 identical, 2 orthogonal; relevances descending.  lambda 0.5, dot: after 0, doc 1 is penalised by 1
    G = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1]], np.float32)
    rel = np.array([1.0, 0.875, 0.5], np.float32)
    live = np.ones(3, bool)
    picked, v = mmr_ref.select(G, rel, live, 3, 0.5, 0.5, mmr_ref.DOT)
    assert picked == [0, 2, 1] and v.tolist() == [0.5, 0.25, -0.0625]
    assert mmr_ref.select(G, rel, live, 3, 1.0, 0.0, mmr_ref.DOT)[0] == [0, 1, 2]             # lambda 1: the relevance order
    assert mmr_ref.select(G, [1.0, 1.0, 1.0], live, 2, 1.0, 0.0, mmr_ref.DOT)[0] == [0, 1]    # ties: the lowest position
    assert mmr_ref.select(G, rel, np.array([False, True, True]), 3, 0.5, 0.5, mmr_ref.DOT)[0] == [1, 2]
    assert mmr_ref.select(G, [-1.0, -2.0, -3.0], live, 1, 0.5, 0.5, mmr_ref.DOT)[0] == [0]    # negative relevances are selectable
    assert mmr_ref.live_mask([7, 6, 8, 9, 10, -1], [1, 1, np.nan, 1, 1, 1], 5, 3, 7).tolist() == [True, False, False, True, False, False]
    assert mmr_ref.live_mask([7, 8], [1, 1], -2, 3, 7).tolist() == [False, False] and mmr_ref.live_mask([7, 8], [1, 1], None, 3, 7).all()
    out = mmr_ref.mask_gram(G, np.array([True, False, True]))
    assert out.tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 1]] and not np.signbit(out).any()


# ---- the service: errors, and the plumbing of the keywords with the launches replaced --------------------------------------------
class _FakeDense:
    """Stands where the dense index stands; records what the service asks of it."""
    dim, n_docs, doc_base, device = 4, 1000, 0, "cpu"

    def __init__(self):
        self.calls = []

    def mmr(self, cand_doc, cand_rel, cand_count, k, lambda_, similarity):
        self.calls.append(("mmr", cand_doc.copy(), cand_rel.copy(), cand_count.copy(), k, lambda_, similarity))
        nq = len(cand_doc)
        # "selection": the list reversed, cut to k
        doc = np.full((nq, k), -1, np.int32)
        rel = np.zeros((nq, k), np.float32)
        count = np.minimum(cand_count, k).astype(np.int32)
        for i in range(nq):
            n = int(cand_count[i])
            doc[i, : count[i]], rel[i, : count[i]] = cand_doc[i, :n][::-1][:k], cand_rel[i, :n][::-1][:k]
        return doc, rel, rel.copy(), count

    def mmr_device(self, doc, rel, count, k, lambda_, similarity):
        self.calls.append(("mmr_device", k, lambda_, similarity))
        return doc, rel, rel, count


def test_diversify_errors_and_plumbing():
    svc = sparse_rx.RetrievalService()
    assert svc.diversify({}) == {}
    with pytest.raises(ValueError, match="lambda"):
        svc.diversify({"q": {"1": 1.0}}, mmr_lambda=2.0)
    with pytest.raises(ValueError, match="similarity must be"):
        svc.diversify({"q": {"1": 1.0}}, similarity="jaccard")
    with pytest.raises(ValueError, match="No embedding index"):
        svc.diversify({"q": {"1": 1.0}})
    svc._dense = fake = _FakeDense()  # embeddings without a BM25 index: docs are named by their row number
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.diversify({"q": {"1": 1.0, "nope": 0.5}})
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.diversify({"q": {"1000": 1.0}})
    with pytest.raises(ValueError, match="at most 256"):
        svc.diversify({"q": {str(i): 1.0 for i in range(257)}}, top_k=10)
    assert not fake.calls
    res = {"a": {"5": 0.75, "9": 0.5, "2": 0.25}, "b": {}, "c": {"7": -1.5}}
    out = svc.diversify(res, top_k=2, mmr_lambda=0.25, similarity="dot")
    assert out == {"a": {"2": 0.25, "9": 0.5}, "b": {}, "c": {"7": -1.5}} and list(out["a"]) == ["2", "9"]  # selection order, original scores
    (_, cd, cr, cc, k, lam, sim), = fake.calls
    assert cd.tolist() == [[5, 9, 2], [7, -1, -1]] and cr.tolist() == [[0.75, 0.5, 0.25], [-1.5, 0, 0]] and cc.tolist() == [3, 1]
    assert (k, lam, sim) == (2, 0.25, "dot") and cr.dtype == np.float32
    assert svc.diversify(res, top_k=0) == {"a": {}, "b": {}, "c": {}} and svc.diversify(res, top_k=99)["a"] == {"2": 0.25, "9": 0.5, "5": 0.75}
    assert "NOT descending" in sparse_rx.RetrievalService.diversify.__doc__
    svc._be.sharded = lambda: True
    with pytest.raises(ValueError, match="whole index on one GPU"):
        svc.diversify(res)


def test_search_hybrid_keywords_plumbing(monkeypatch):
    from sparse_rx import service
    svc = sparse_rx.RetrievalService()
    corpus = {f"d{i}": {"text": f"alpha beta w{i} w{i % 7}"} for i in range(300)}
    svc._be.build(corpus, idf_kind="bm25")  # the host index only: nothing is uploaded
    svc._built_k1b = (svc.k1, svc.b)
    svc._dense = fake = _FakeDense()
    seen = []

    def recorder(index, q_ptr, q_term, q_weight, dense_search, ka, kb, k, mode, weights, rrf_c, rescore=False, dense_score=None, **kw):
        seen.append(dict(ka=ka, kb=kb, k=k, rescore=rescore, **kw))
        nq = len(q_ptr) - 1
        return np.tile(np.arange(k, dtype=np.int32), (nq, 1)), np.ones((nq, k), np.float32), np.full(nq, k, np.int32)

    monkeypatch.setattr(service, "hybrid_search", recorder)
    q, v = {"a": "alpha w3"}, {"a": np.ones(4, np.float32)}
    out = svc.search_hybrid(q, v, top_k=10)
    assert seen[-1] == dict(ka=10, kb=10, k=10, rescore=False) and len(out["a"]) == 10 and not fake.calls  # no pool, no post step: today's call
    svc.search_hybrid(q, v, top_k=10, mmr_lambda=0.5)
    assert (seen[-1]["k"], seen[-1]["ka"], seen[-1]["kb"]) == (40, 40, 40) and callable(seen[-1]["post"])
    d, r, n = seen[-1]["post"]("doc", "score", "count")
    assert (d, r, n) == ("doc", "score", "count") and fake.calls == [("mmr_device", 10, 0.5, "cosine")]
    svc.search_hybrid(q, v, top_k=100, mmr_lambda=0.0, mmr_similarity="dot", rescore=True)
    assert (seen[-1]["k"], seen[-1]["ka"], seen[-1]["rescore"]) == (256, 256, True)  # min(max(400, 100), 256, 300)
    svc.search_hybrid(q, v, top_k=10, mmr_lambda=1.0, mmr_pool=20, candidates=15)
    assert (seen[-1]["k"], seen[-1]["ka"]) == (20, 15)  # a given depth is kept
    svc.search_hybrid(q, v, top_k=10, mmr_lambda=1.0, mmr_pool=4)
    seen[-1]["post"]("doc", "score", "count")
    assert seen[-1]["k"] == 4 and fake.calls[-1] == ("mmr_device", 4, 1.0, "cosine")  # a pool below top_k: all of it, reordered
    n_before = len(seen)
    with pytest.raises(ValueError, match="mmr_pool"):
        svc.search_hybrid(q, v, top_k=10, mmr_lambda=0.5, mmr_pool=257)
    with pytest.raises(ValueError, match="lambda"):
        svc.search_hybrid(q, v, top_k=10, mmr_lambda=1.5)
    with pytest.raises(ValueError, match="similarity must be"):
        svc.search_hybrid(q, v, top_k=10, mmr_lambda=0.5, mmr_similarity="l2")
    assert len(seen) == n_before
    svc.search_hybrid(q, v, top_k=10, mmr_pool=300, mmr_similarity="l2")  # without mmr_lambda the other two keywords are not looked at
    assert seen[-1] == dict(ka=10, kb=10, k=10, rescore=False)
    assert "not descending" in sparse_rx.RetrievalService.search_hybrid.__doc__
