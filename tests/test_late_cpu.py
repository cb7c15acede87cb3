"""Late-interaction reranking without a GPU: the eighth header and its symbol table, the frozen counts of the other seven,
every refusal of the three entry points (none reaches a device), the Python layer's ValueErrors, the NumPy restatement
(tests/late_ref.py) on an example small enough to do by hand, and the plumbing of the service doors with the token index
replaced by a recorder."""
import os
import re

import numpy as np
import pytest

import late_ref
import sparse_rx
from sparse_rx import _capi
from sparse_rx.late import TokenIndex, check_late_shape, doc_token_ptr, late_pool_depth, stack_query_tokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(12)]  # 16-byte aligned addresses, never dereferenced


def test_eighth_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "sparse_rx_maxsim.h")).read()
    declared = set(re.findall(r"\b(srx_maxsim_[a-z_0-9]+)\s*\(", hdr.split("#ifndef SPARSE_RX_MAXSIM_H")[1]))
    assert declared == set(_capi.MAXSIM_SYMBOLS) and len(declared) == 3, declared ^ set(_capi.MAXSIM_SYMBOLS)
    assert '#include "sparse_rx.h"' in hdr and '#include "sparse_rx_half.h"' in hdr and "has no reranker" in hdr
    others = (_capi.SYMBOLS, _capi.RESCORE_SYMBOLS, _capi.QUANT_SYMBOLS, _capi.FILTER_SYMBOLS, _capi.HALF_SYMBOLS, _capi.MMR_SYMBOLS,
              _capi.TERMS_SYMBOLS)
    for other in others:
        assert not set(_capi.MAXSIM_SYMBOLS) & set(other)
    assert [len(t) for t in others] == [35, 4, 4, 8, 5, 3, 2]  # the new entry points are a table of their own: 64 in eight headers
    assert "maxsim.hip" in _capi.SOURCES
    deps = [os.path.basename(p) for p in _capi._deps()]
    assert "sparse_rx_maxsim.h" in deps and "maxsim.hip" in deps and "half_common.h" in deps
    assert "sparse_rx_maxsim.h" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    L = _capi.lib()
    assert L.srx_version() == 301
    for name, (res, args) in _capi.MAXSIM_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    assert len(_capi.MAXSIM_SYMBOLS["srx_maxsim_score_docs_half"][1]) == 19 and len(_capi.MAXSIM_SYMBOLS["srx_maxsim_rerank_half"][1]) == 22
    assert int(re.search(r"#define SRX_MAXSIM_MAX_QT (\d+)", hdr).group(1)) == _capi.SRX_MAXSIM_MAX_QT == late_ref.MAX_QT == 128
    assert late_ref.MAX_M == _capi.SRX_MAX_K == 1024
    for name in ("TokenIndex", "check_late_shape", "late_pool_depth"):
        assert name in sparse_rx.__all__ and getattr(sparse_rx, name) is not None


def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg, (rc, word, msg)


LIMITS_OK = [(1, 64), (32, 1024), (33, 512), (64, 512), (65, 256), (128, 256), (128, 64), (96, 320)]
LIMITS_BAD = [(0, 64), (-1, 64), (129, 64), (33, 1024), (65, 512), (97, 320), (128, 320), (1, 0), (1, 32), (1, 96), (1, 1088)]


def test_workspace_bytes():
    L = _capi.lib()
    ws = L.srx_maxsim_workspace_bytes
    for tq, dim_pad in LIMITS_OK:
        assert late_ref.shape_ok(tq, dim_pad) and ws(3, tq, dim_pad, 7) > 0, (tq, dim_pad)
    for tq, dim_pad in LIMITS_BAD:
        _refused(ws(3, tq, dim_pad, 7), "srx_maxsim_workspace_bytes")
    for args in ((-1, 8, 64, 4), (1, 8, 64, -1), (1, 8, 64, 1025), (2 ** 22, 8, 64, 1024)):
        _refused(ws(*args), "srx_maxsim_workspace_bytes")
    # the packed query tokens, the score matrix of the rerank form (m >= 1), slack
    for nq, tq, dim_pad, m in ((0, 1, 64, 0), (1, 1, 64, 1), (5, 33, 128, 65), (1024, 32, 128, 128), (70, 128, 256, 1024)):
        q = nq * ((tq + 31) // 32 * 32) * dim_pad * 2
        assert q <= ws(nq, tq, dim_pad, 0) <= q + 512
        assert q + nq * m * 4 <= ws(nq, tq, dim_pad, m) <= q + nq * m * 4 + 768
    # monotone in every argument
    base = (8, 31, 128, 100)
    for i, hi in enumerate((9, 33, 192, 101)):
        more = list(base)
        more[i] = hi
        assert ws(*more) >= ws(*base), (i, hi)
    assert ws(8, 33, 128, 100) > ws(8, 32, 128, 100) == ws(8, 1, 128, 100) and ws(8, 31, 128, 1) > ws(8, 31, 128, 0)


def _calls(L):
    ok = dict(device=0, type=0, tok=P[0], n_tok=5000, dim_pad=128, tok_ptr=P[1], n_docs=1000, doc_base=0, q_tok=P[2], q_cnt=P[3], nq=2, tq=32,
              cand_doc=P[4], cand_count=P[5], m=8)
    tail_s = dict(out_score=P[6], ws=P[7], ws_bytes=1 << 30, stream=None)
    tail_r = dict(k=4, out_doc=P[8], out_score=P[6], out_count=P[9], ws=P[7], ws_bytes=1 << 30, stream=None)
    score = lambda **kw: L.srx_maxsim_score_docs_half(*{**ok, **tail_s, **kw}.values())
    rerank = lambda **kw: L.srx_maxsim_rerank_half(*{**ok, **tail_r, **kw}.values())
    return [("srx_maxsim_score_docs_half", score), ("srx_maxsim_rerank_half", rerank)]


def test_refusals():
    L = _capi.lib()
    for who, call in _calls(L):
        rerank = who.endswith("rerank_half")
        for t in (-1, 2, 7):
            _refused(call(type=t), "type must be")
        for d in (0, 32, 96, 1088, -64):
            _refused(call(dim_pad=d), "multiple of 64")
        for tq, dim_pad in LIMITS_BAD[:7]:
            _refused(call(tq=tq, dim_pad=dim_pad), "tq must be")
        for m in (0, -1):
            _refused(call(m=m, k=1), "m must be")
        for n in (0, -1, 2 ** 31 - 1):
            _refused(call(n_docs=n), "n_docs")
        for n in (-1, 2 ** 31 - 1):
            _refused(call(n_tok=n), "n_tok")
        _refused(call(doc_base=-1), "doc_base")
        _refused(call(nq=-1), "nq < 0")
        _refused(call(nq=2 ** 22, m=1024, k=1), "nq * m")
        for null in ("tok", "tok_ptr", "q_tok", "cand_doc", "out_score") + (("out_doc", "out_count") if rerank else ()):
            _refused(call(**{null: None}), "null pointer")
        assert who.encode() in L.srx_last_error()
        _refused(call(tok=P[0] + 8), "16-byte aligned")
        _refused(call(q_tok=P[2] + 4), "16-byte aligned")
        need = L.srx_maxsim_workspace_bytes(2, 32, 128, 8 if rerank else 0)
        assert call(ws=None) == -3 and call(ws_bytes=need - 1) == -3  # SRX_ERR_NOMEM
        assert b"workspace" in L.srx_last_error()
        # nothing to do: no launch, whatever the pointers; NULL counts and an empty token store are legal arguments
        nulls = dict(tok=None, tok_ptr=None, q_tok=None, cand_doc=None, out_score=None, ws=None, ws_bytes=0)
        if rerank:
            nulls.update(out_doc=None, out_count=None)
        assert call(nq=0, **nulls) == 0
        assert call(nq=0, q_cnt=None, cand_count=None, n_tok=0, tq=128, dim_pad=256) == 0 and call(nq=0, tq=32, dim_pad=1024) == 0
    score, rerank = _calls(L)[0][1], _calls(L)[1][1]
    for m in (1025, 4096):
        _refused(rerank(m=m, k=1), "m must be")  # the rerank form ranks at most SRX_MAX_K candidates ...
    assert score(nq=0, m=2 ** 31 - 1) == 0      # ... the scorer form is limited by nq * m only
    for k in (0, -1, 9):
        _refused(rerank(k=k), "k must be")


def test_python_value_errors():
    assert check_late_shape(32, 1024) is None and check_late_shape(128, 256, 1024, 1024) == 1024 and check_late_shape(1, 64, 1, 1) == 1
    for tq, dim_pad in LIMITS_OK:
        check_late_shape(tq, dim_pad)
    for tq in (0, 129, -1):
        with pytest.raises(ValueError, match="query tokens"):
            check_late_shape(tq, 64)
    for tq, dim_pad in ((33, 1024), (65, 512), (97, 320)):
        with pytest.raises(ValueError, match="ceil32"):
            check_late_shape(tq, dim_pad)
    for m in (0, 1025):
        with pytest.raises(ValueError, match="candidates per query"):
            check_late_shape(8, 64, m, 1)
    for k in (0, 11, -1):
        with pytest.raises(ValueError, match="k must be"):
            check_late_shape(8, 64, 10, k)
    assert late_pool_depth(10, None, 10 ** 6) == 100 and late_pool_depth(300, None, 10 ** 6) == 300 and late_pool_depth(2000, None, 10 ** 6) == 1024
    assert late_pool_depth(10, None, 25) == 25 and late_pool_depth(10, 1024, 10 ** 6) == 1024 and late_pool_depth(10, 5, 10 ** 6) == 5
    for bad in (1025, 0, -1):
        with pytest.raises(ValueError, match="late_pool"):
            late_pool_depth(10, bad, 10 ** 6)
    assert doc_token_ptr([2, 0, 3], 5).tolist() == [0, 2, 2, 5] and doc_token_ptr([0], 0).dtype == np.int32
    for counts, n in (([2, 3], 6), ([-1, 3], 2), ([], 0), ([[1]], 1), ([1.0], 1)):
        with pytest.raises(ValueError, match="doc_token_counts"):
            doc_token_ptr(counts, n)
    block, counts = stack_query_tokens({"a": np.ones((2, 4)), "b": np.zeros((0, 4)), "c": np.ones((3, 4))}, ["a", "b", "c"], 4)
    assert block.shape == (3, 3, 4) and block.dtype == np.float32 and counts.tolist() == [2, 0, 3] and block[0, 2].tolist() == [0, 0, 0, 0]
    assert stack_query_tokens({}, [], 4)[0].shape == (0, 1, 4)
    with pytest.raises(ValueError, match="no query tokens"):
        stack_query_tokens({"a": np.ones((2, 4))}, ["b"], 4)
    with pytest.raises(ValueError, match="expected"):
        stack_query_tokens({"a": np.ones((2, 5))}, ["a"], 4)
    with pytest.raises(ValueError, match="at most 128"):
        stack_query_tokens({"a": np.ones((129, 4))}, ["a"], 4)
    # refused, not approximated: the sharded searcher, the host pipeline and the registry's hybrid mirror have no such door
    for cls in (sparse_rx.ShardedSearcher, sparse_rx.HostBatchPipeline, sparse_rx.HybridRetriever, sparse_rx.DenseHalfIndex):
        assert not hasattr(cls, "rerank_late") and not hasattr(cls, "rerank_device") and not hasattr(cls, "set_token_embeddings")
    for name in ("score_docs_device", "score_docs", "rerank_device", "rerank", "device_bytes", "close", "from_token_embeddings"):
        assert callable(getattr(TokenIndex, name))


def test_token_index_checks_before_any_launch():
    import torch
    ix = TokenIndex.__new__(TokenIndex)  # no device behind it: every check below comes before the library is touched
    ix.device, ix.dim, ix.dim_pad, ix.dtype = torch.device("cpu"), 48, 64, "f16"
    d = torch.zeros((2, 8), dtype=torch.int32)
    q = torch.zeros((2, 4, 48))
    with pytest.raises(ValueError, match="float32 tensor"):
        ix.score_docs_device(q.double(), None, d)
    with pytest.raises(ValueError, match="float32 tensor"):
        ix.rerank_device(q[0], None, d, None, 4)
    with pytest.raises(ValueError, match="dim 32"):
        ix.score_docs_device(q[:, :, :32], None, d)
    with pytest.raises(ValueError, match="query tokens"):
        ix.score_docs_device(torch.zeros((2, 129, 48)), None, d)
    with pytest.raises(ValueError, match="q_tok_count"):
        ix.score_docs_device(q, torch.zeros(3, dtype=torch.int32), d)
    with pytest.raises(ValueError, match="q_tok_count"):
        ix.score_docs_device(q, torch.zeros(2, dtype=torch.int64), d)
    with pytest.raises(ValueError, match="\\[nq, tq, dim\\]"):
        ix.score_docs(np.zeros((2, 48), np.float32), None, np.zeros((2, 8), np.int32))
    with pytest.raises(ValueError, match="2-D integer"):
        ix.score_docs(np.zeros((2, 4, 48), np.float32), None, np.zeros((2, 8), np.float32))
    with pytest.raises(ValueError, match="q_tok_count"):
        ix.rerank(np.zeros((2, 4, 48), np.float32), [1, 2, 3], np.zeros((2, 8), np.int32), None, 4)
    for bad in ("f32", "int8", None):
        with pytest.raises(ValueError, match="dtype must be"):
            TokenIndex.from_token_embeddings(np.zeros((4, 8), np.float32), [4], dtype=bad)
    with pytest.raises(ValueError, match="float32"):
        TokenIndex.from_token_embeddings(np.zeros((4, 8), np.float64), [4])
    with pytest.raises(ValueError, match="doc_token_counts"):
        TokenIndex.from_token_embeddings(np.zeros((4, 8), np.float32), [3])
    with pytest.raises(ValueError, match="at least one token row"):
        TokenIndex.from_token_embeddings(np.zeros((0, 8), np.float32), [0, 0])


# ---- the restatement, by hand ------------------------------------------------------------------------------------------------
def test_restatement_by_hand():
    # two query tokens (and a third, dead one); doc A has two tokens, doc B none, doc C only negative similarities
    sim_a = np.array([[1.0, 3.0], [2.0, -1.0], [100.0, 100.0]], np.float32)
    sim_c = np.array([[-4.0, -2.0, -3.0], [-1.5, -8.0, -0.5], [50.0, 50.0, 50.0]], np.float32)
    assert late_ref.score_from_sim(sim_a, 2) == np.float32(5.0)            # 3 + 2: the dead token's 100 is skipped
    assert late_ref.score_from_sim(sim_a, 3) == np.float32(105.0)
    assert late_ref.score_from_sim(sim_c, 2) == np.float32(-2.5)           # the least negative ones: -2 + -0.5, not 0
    b = late_ref.score_from_sim(np.zeros((3, 0), np.float32), 2)            # no tokens: +0
    z = late_ref.score_from_sim(sim_a, 0)                                   # no live query token: +0
    assert b == 0 and z == 0 and not np.signbit(b) and not np.signbit(z) and b.dtype == np.float32
    # the adds are float32 and ordered: (2^24 + 1) + 1 differs from 2^24 + (1 + 1)
    big = np.array([[2.0 ** 24], [1.0], [1.0]], np.float32)
    assert late_ref.score_from_sim(big, 3) == np.float32(2.0 ** 24) and late_ref.score_from_sim(big[::-1], 3) == np.float32(2.0 ** 24 + 2)
    assert late_ref.live_tokens(None, 5) == 5 and late_ref.live_tokens(-3, 5) == 0 and late_ref.live_tokens(9, 5) == 5 and late_ref.live_tokens(2, 5) == 2
    # positions: the count, padding, ids below doc_base and at doc_base + n_docs
    assert late_ref.live_positions([7, 6, 9, 10, 8, -1], 5, 7, 3).tolist() == [True, False, True, False, True, False]
    assert late_ref.live_positions([7, 8], -2, 7, 3).tolist() == [False, False] and late_ref.live_positions([7, 8], None, 7, 3).all()
    assert late_ref.live_positions([7, 8, 9], 2, 7, 3).tolist() == [True, True, False]
    # ranking: score descending, ties by ascending doc id, negative scores kept, dead positions never listed
    docs, scores = [40, 10, 30, 20, 50], np.array([5.0, -2.5, 5.0, 0.0, 9.0], np.float32)
    live = np.array([True, True, True, True, False])
    d, s, n = late_ref.rank(docs, scores, live, 5)
    assert d.tolist() == [30, 40, 20, 10, -1] and s.tolist() == [5.0, 5.0, 0.0, -2.5, 0.0] and n == 4
    d, s, n = late_ref.rank(docs, scores, live, 2)
    assert d.tolist() == [30, 40] and n == 2
    assert late_ref.rank(docs, scores, np.zeros(5, bool), 3)[0].tolist() == [-1, -1, -1]
    # the fp64 form and its bound on integers: exact, with a positive bound
    import half_ref
    q = half_ref.round_codes(np.array([[1, 2, 0, 0], [0, -1, 1, 0]], np.float32), "f16")
    t = half_ref.round_codes(np.array([[1, 1, 1, 1], [-2, 0, 3, 0]], np.float32), "f16")
    assert late_ref.score_f64(q, t, "f16", 2) == 3.0 + 3.0 and late_ref.score_f64(q, t, "f16", 1) == 3.0
    assert late_ref.score_f64(q, t[:0], "f16", 2) == 0.0 and late_ref.tol(q, t[:0], "f16", 2) == 0.0
    assert 0 < late_ref.tol(q, t, "f16", 2) < 1e-4


# ---- the service: errors, and the plumbing of the keywords with the launches replaced ------------------------------------------
class _FakeTokens:
    """Stands where the token index stands; records what the service asks of it."""
    dim, dim_pad, n_docs, doc_base, device = 4, 64, 300, 0, "cpu"

    def __init__(self):
        self.calls = []

    def rerank(self, q_tok, q_cnt, cand_doc, cand_count, k):
        self.calls.append(("rerank", q_tok.copy(), q_cnt.copy(), cand_doc.copy(), cand_count.copy(), k))
        nq = len(cand_doc)
        doc, score = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.float32)
        count = np.minimum(cand_count, k).astype(np.int32)
        for i in range(nq):  # "rerank": the list reversed, cut to k, scored -(row number)
            n = int(cand_count[i])
            doc[i, : count[i]] = cand_doc[i, :n][::-1][:k]
            score[i, : count[i]] = -doc[i, : count[i]].astype(np.float32)
        return doc, score, count

    def rerank_device(self, q_tok, q_cnt, doc, count, k):
        self.calls.append(("rerank_device", tuple(q_tok.shape), q_cnt.tolist(), k))
        return doc, "late score", count

    def close(self):
        self.calls.append(("close",))


def _service():
    svc = sparse_rx.RetrievalService()
    corpus = {f"d{i}": {"text": f"alpha beta w{i} w{i % 7}"} for i in range(300)}
    svc._be.build(corpus, idf_kind="bm25")  # the host index only: nothing is uploaded
    svc._built_k1b = (svc.k1, svc.b)
    return svc


def test_rerank_late_errors_and_plumbing():
    svc = _service()
    toks = {"a": np.ones((3, 4), np.float32), "c": np.ones((1, 4), np.float32)}
    assert svc.rerank_late({}, toks) == {}
    with pytest.raises(ValueError, match="No token index"):
        svc.rerank_late({"a": {"d1": 1.0}}, toks)
    svc._late = fake = _FakeTokens()
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.rerank_late({"a": {"d1": 1.0, "nope": 0.5}}, toks)
    with pytest.raises(ValueError, match="at most 1024"):
        _too_long(toks)
    with pytest.raises(ValueError, match="at most 128"):
        svc.rerank_late({"a": {"d1": 1.0}}, {"a": np.ones((129, 4), np.float32)})
    with pytest.raises(ValueError, match="no query tokens"):
        svc.rerank_late({"b": {"d1": 1.0}}, toks)
    with pytest.raises(ValueError, match="expected"):
        svc.rerank_late({"a": {"d1": 1.0}}, {"a": np.ones((2, 5), np.float32)})
    assert not fake.calls
    res = {"a": {"d5": 0.75, "d9": 0.5, "d2": 0.25}, "b": {}, "c": {"d7": -1.5}}
    out = svc.rerank_late(res, toks, top_k=2)
    assert out == {"a": {"d2": -2.0, "d9": -9.0}, "b": {}, "c": {"d7": -7.0}} and list(out["a"]) == ["d2", "d9"]  # the new order, the new scores
    (_, qt, qc, cd, cc, k), = fake.calls
    assert qt.shape == (2, 3, 4) and qt.dtype == np.float32 and qc.tolist() == [3, 1] and qt[1, 1:].sum() == 0
    assert cd.tolist() == [[5, 9, 2], [7, -1, -1]] and cc.tolist() == [3, 1] and k == 2
    assert svc.rerank_late(res, toks, top_k=0) == {"a": {}, "b": {}, "c": {}}
    assert list(svc.rerank_late(res, toks, top_k=99)["a"]) == ["d2", "d9", "d5"] and fake.calls[-1][-1] == 3  # k is cut to the longest list
    svc._be.sharded = lambda: True
    with pytest.raises(ValueError, match="whole index on one GPU"):
        svc.rerank_late(res, toks)
    with pytest.raises(ValueError, match="whole index on one GPU"):
        svc.set_token_embeddings((np.zeros((300, 4), np.float32), [1] * 300))
    svc._be.sharded = lambda: False
    svc.close()
    assert fake.calls[-1] == ("close",) and svc._late is None


def _too_long(toks):
    """A list of 1025 known docs: the length is refused after the ids have been resolved, before the token index is asked"""
    big = sparse_rx.RetrievalService()
    big._be.build({f"d{i}": {"text": f"alpha w{i}"} for i in range(1025)}, idf_kind="bm25")
    big._late = _FakeTokens()
    return big.rerank_late({"a": {f"d{i}": 1.0 for i in range(1025)}}, toks)


def test_set_token_embeddings_errors():
    svc = sparse_rx.RetrievalService()
    with pytest.raises(ValueError, match="BM25 index not built"):
        svc.set_token_embeddings({})
    svc = _service()
    with pytest.raises(ValueError, match="dtype must be"):
        svc.set_token_embeddings({}, storage="f32")
    full = {f"d{i}": np.zeros((i % 3, 4), np.float32) for i in range(300)}
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.set_token_embeddings({**full, "zzz": np.zeros((1, 4), np.float32)})
    with pytest.raises(ValueError, match="no token embeddings for doc 'd299'"):
        svc.set_token_embeddings({d: t for d, t in full.items() if d != "d299"})
    with pytest.raises(ValueError, match="one dim"):
        svc.set_token_embeddings({**full, "d4": np.zeros((2, 5), np.float32)})
    with pytest.raises(ValueError, match="one token count per document"):
        svc.set_token_embeddings((np.zeros((10, 4), np.float32), [1] * 10))
    with pytest.raises(ValueError, match="doc_token_counts"):
        svc.set_token_embeddings((np.zeros((10, 4), np.float32), [1] * 300))


def test_search_hybrid_keywords_plumbing(monkeypatch):
    from sparse_rx import service
    svc = _service()
    svc._dense = type("D", (), {"dim": 4, "n_docs": 300, "doc_base": 0, "device": "cpu"})()
    seen = []

    def recorder(index, q_ptr, q_term, q_weight, dense_search, ka, kb, k, mode, weights, rrf_c, rescore=False, dense_score=None, **kw):
        seen.append(dict(ka=ka, kb=kb, k=k, rescore=rescore, **kw))
        nq = len(q_ptr) - 1
        return np.tile(np.arange(k, dtype=np.int32), (nq, 1)), np.ones((nq, k), np.float32), np.full(nq, k, np.int32)

    monkeypatch.setattr(service, "hybrid_search", recorder)
    q, v = {"a": "alpha w3"}, {"a": np.ones(4, np.float32)}
    toks = {"a": np.ones((3, 4), np.float32)}
    out = svc.search_hybrid(q, v, top_k=10)
    assert seen[-1] == dict(ka=10, kb=10, k=10, rescore=False) and len(out["a"]) == 10  # no keyword: the call made today
    with pytest.raises(ValueError, match="No token index"):
        svc.search_hybrid(q, v, top_k=10, late_query_tokens=toks)
    svc._late = fake = _FakeTokens()
    svc.search_hybrid(q, v, top_k=10, late_query_tokens=toks)
    assert (seen[-1]["k"], seen[-1]["ka"], seen[-1]["kb"]) == (100, 100, 100) and callable(seen[-1]["post"])  # the fusion is asked for late_pool
    assert seen[-1]["post"]("doc", "score", "count") == ("doc", "late score", "count") and fake.calls == [("rerank_device", (1, 3, 4), [3], 10)]
    svc.search_hybrid(q, v, top_k=200, late_query_tokens=toks, rescore=True)
    assert (seen[-1]["k"], seen[-1]["ka"], seen[-1]["rescore"]) == (200, 200, True)
    svc.search_hybrid(q, v, top_k=10, late_query_tokens=toks, late_pool=20, candidates=15)
    assert (seen[-1]["k"], seen[-1]["ka"]) == (20, 15)  # a given depth is kept
    svc.search_hybrid(q, v, top_k=10, late_query_tokens=toks, late_pool=4)
    seen[-1]["post"]("doc", "score", "count")
    assert seen[-1]["k"] == 4 and fake.calls[-1] == ("rerank_device", (1, 3, 4), [3], 4)  # a pool below top_k: all of it, reordered
    n_before = len(seen)
    with pytest.raises(ValueError, match="late_pool"):
        svc.search_hybrid(q, v, top_k=10, late_query_tokens=toks, late_pool=1025)
    with pytest.raises(ValueError, match="do not combine"):
        svc.search_hybrid(q, v, top_k=10, late_query_tokens=toks, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="no query tokens"):
        svc.search_hybrid(q, v, top_k=10, late_query_tokens={})
    with pytest.raises(ValueError, match="at most 128"):
        svc.search_hybrid(q, v, top_k=10, late_query_tokens={"a": np.ones((129, 4), np.float32)})
    assert len(seen) == n_before
    svc.search_hybrid(q, v, top_k=10, late_pool=5000)  # without late_query_tokens the pool keyword is not looked at
    assert seen[-1] == dict(ka=10, kb=10, k=10, rescore=False)
    svc._be.sharded = lambda: True
    with pytest.raises(ValueError, match="whole index on one GPU"):
        svc.search_hybrid(q, v, top_k=10, late_query_tokens=toks)
    assert "late_query_tokens" in sparse_rx.RetrievalService.search_hybrid.__doc__
