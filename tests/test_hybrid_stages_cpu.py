"""What ``RetrievalService.search_hybrid`` composes after the fusion, without a GPU: for every legal subset of {late rerank,
boost, collapse, MMR} the depths the fusion is asked for and the (stage, width handed in, rows asked to keep) chain that runs on
the fused triple, with the four device entry points and ``hybrid_search`` replaced by recorders; which refusal wins when a call
has two faults; the pool messages; and the doors ``RetrievalService`` and the registry mirrors share.

The expected values are literals recorded from the hand-written branches this composition replaced -- they are not computed from
a restatement of its rule."""
import inspect
import itertools

import numpy as np
import pytest
import torch

import sparse_rx
from sparse_rx import service
from sparse_rx.backend import collapse_pool_depth
from sparse_rx.index import mmr_pool_depth
from sparse_rx.late import late_pool_depth

N_DOCS, TOP_K = 300, 5
Q, V = {"a": "alpha w3"}, {"a": np.ones(4, np.float32)}
STAGE_KEYWORDS = {"late": dict(late_query_tokens={"a": np.ones((3, 4), np.float32)}),
                  "boost": dict(boost={"functions": [{"field_value": {"field": "price", "lo": 0.0, "hi": 50.0}}]}),
                  "collapse": dict(collapse_by="parent", per_group=2, collapse_nulls="drop"),
                  "mmr": dict(mmr_lambda=0.25, mmr_similarity="dot")}
COMBOS = [c for n in range(5) for c in itertools.combinations(STAGE_KEYWORDS, n) if not ("late" in c and "mmr" in c)]
SETTINGS = {1: dict(),
            2: dict(late_pool=30, boost_pool=40, collapse_pool=50, mmr_pool=12),
            3: dict(late_pool=30, boost_pool=8, collapse_pool=9, mmr_pool=20),
            4: dict(candidates=7)}

# (combination, setting) -> ((ka, kb, k) the fusion was asked for, [(stage, width handed in, rows asked to keep), ...])
EXPECTED = {
    ((), 1): ((5, 5, 5), []),
    ((), 2): ((5, 5, 5), []),
    ((), 3): ((5, 5, 5), []),
    ((), 4): ((7, 7, 5), []),
    (('late',), 1): ((100, 100, 100), [('late', 100, 5)]),
    (('late',), 2): ((30, 30, 30), [('late', 30, 5)]),
    (('late',), 3): ((30, 30, 30), [('late', 30, 5)]),
    (('late',), 4): ((7, 7, 100), [('late', 100, 5)]),
    (('boost',), 1): ((100, 100, 100), [('boost', 100, 5)]),
    (('boost',), 2): ((40, 40, 40), [('boost', 40, 5)]),
    (('boost',), 3): ((8, 8, 8), [('boost', 8, 5)]),
    (('boost',), 4): ((7, 7, 100), [('boost', 100, 5)]),
    (('collapse',), 1): ((100, 100, 100), [('collapse', 100, 5)]),
    (('collapse',), 2): ((50, 50, 50), [('collapse', 50, 5)]),
    (('collapse',), 3): ((9, 9, 9), [('collapse', 9, 5)]),
    (('collapse',), 4): ((7, 7, 100), [('collapse', 100, 5)]),
    (('mmr',), 1): ((20, 20, 20), [('mmr', 20, 5)]),
    (('mmr',), 2): ((12, 12, 12), [('mmr', 12, 5)]),
    (('mmr',), 3): ((20, 20, 20), [('mmr', 20, 5)]),
    (('mmr',), 4): ((7, 7, 20), [('mmr', 20, 5)]),
    (('late', 'boost'), 1): ((100, 100, 100), [('late', 100, 100), ('boost', 100, 5)]),
    (('late', 'boost'), 2): ((30, 30, 30), [('late', 30, 30), ('boost', 30, 5)]),
    (('late', 'boost'), 3): ((30, 30, 30), [('late', 30, 30), ('boost', 30, 5)]),
    (('late', 'boost'), 4): ((7, 7, 100), [('late', 100, 100), ('boost', 100, 5)]),
    (('late', 'collapse'), 1): ((100, 100, 100), [('late', 100, 100), ('collapse', 100, 5)]),
    (('late', 'collapse'), 2): ((30, 30, 30), [('late', 30, 30), ('collapse', 30, 5)]),
    (('late', 'collapse'), 3): ((30, 30, 30), [('late', 30, 30), ('collapse', 30, 5)]),
    (('late', 'collapse'), 4): ((7, 7, 100), [('late', 100, 100), ('collapse', 100, 5)]),
    (('boost', 'collapse'), 1): ((100, 100, 100), [('boost', 100, 100), ('collapse', 100, 5)]),
    (('boost', 'collapse'), 2): ((40, 40, 40), [('boost', 40, 40), ('collapse', 40, 5)]),
    (('boost', 'collapse'), 3): ((8, 8, 8), [('boost', 8, 8), ('collapse', 8, 5)]),
    (('boost', 'collapse'), 4): ((7, 7, 100), [('boost', 100, 100), ('collapse', 100, 5)]),
    (('boost', 'mmr'), 1): ((100, 100, 100), [('boost', 100, 20), ('mmr', 20, 5)]),
    (('boost', 'mmr'), 2): ((40, 40, 40), [('boost', 40, 12), ('mmr', 12, 5)]),
    (('boost', 'mmr'), 3): ((8, 8, 8), [('boost', 8, 8), ('mmr', 8, 5)]),
    (('boost', 'mmr'), 4): ((7, 7, 100), [('boost', 100, 20), ('mmr', 20, 5)]),
    (('collapse', 'mmr'), 1): ((100, 100, 100), [('collapse', 100, 20), ('mmr', 20, 5)]),
    (('collapse', 'mmr'), 2): ((50, 50, 50), [('collapse', 50, 12), ('mmr', 12, 5)]),
    (('collapse', 'mmr'), 3): ((20, 20, 9), [('collapse', 9, 9), ('mmr', 9, 5)]),
    (('collapse', 'mmr'), 4): ((7, 7, 100), [('collapse', 100, 20), ('mmr', 20, 5)]),
    (('late', 'boost', 'collapse'), 1): ((100, 100, 100), [('late', 100, 100), ('boost', 100, 100), ('collapse', 100, 5)]),
    (('late', 'boost', 'collapse'), 2): ((30, 30, 30), [('late', 30, 30), ('boost', 30, 30), ('collapse', 30, 5)]),
    (('late', 'boost', 'collapse'), 3): ((30, 30, 30), [('late', 30, 30), ('boost', 30, 30), ('collapse', 30, 5)]),
    (('late', 'boost', 'collapse'), 4): ((7, 7, 100), [('late', 100, 100), ('boost', 100, 100), ('collapse', 100, 5)]),
    (('boost', 'collapse', 'mmr'), 1): ((100, 100, 100), [('boost', 100, 100), ('collapse', 100, 20), ('mmr', 20, 5)]),
    (('boost', 'collapse', 'mmr'), 2): ((40, 40, 40), [('boost', 40, 40), ('collapse', 40, 12), ('mmr', 12, 5)]),
    (('boost', 'collapse', 'mmr'), 3): ((8, 8, 8), [('boost', 8, 8), ('collapse', 8, 8), ('mmr', 8, 5)]),
    (('boost', 'collapse', 'mmr'), 4): ((7, 7, 100), [('boost', 100, 100), ('collapse', 100, 20), ('mmr', 20, 5)]),
}


class _Recorder:
    """A service over a 300-doc host index (nothing is uploaded) whose dense index, token index, field table, BoostFn and
    hybrid_search are fakes that note what they are asked and slice CPU tensors."""

    def __init__(self, monkeypatch):
        self.fused, self.stages, self.args = [], [], {}
        svc = self.svc = sparse_rx.RetrievalService()
        svc._be.build({f"d{i}": {"text": f"alpha beta w{i} w{i % 7}"} for i in range(N_DOCS)}, idf_kind="bm25")
        svc._built_k1b = (svc.k1, svc.b)
        svc.set_doc_fields({"parent": [i // 4 for i in range(N_DOCS)], "price": np.linspace(0.0, 50.0, N_DOCS, dtype=np.float32)})
        rec = self

        def cut(name, doc, score, count, keep, *args):
            rec.stages.append((name, int(doc.shape[1]), keep))
            rec.args[name] = args
            assert 1 <= keep <= doc.shape[1]  # what every device entry point requires of its k
            return doc[:, :keep], score[:, :keep], count.clamp(max=keep)

        class Dense:
            dim, n_docs, doc_base, device = 4, N_DOCS, 0, "cpu"

            def mmr_device(self, doc, score, count, keep, mmr_lambda, similarity):
                d, s, n = cut("mmr", doc, score, count, keep, mmr_lambda, similarity)
                return d, s, "mmr value", n

        class Tokens:
            dim, device = 4, "cpu"

            def rerank_device(self, q_tok, q_cnt, doc, count, keep):
                return cut("late", doc, torch.zeros(doc.shape), count, keep, tuple(q_tok.shape), q_cnt.tolist())

            def close(self):
                pass

        class Table:
            def collapse_device(self, by, doc, score, count, keep, per_group, nulls):
                return cut("collapse", doc, score, count, keep, by, per_group, nulls)

        class Boost:
            def __init__(self, table, resolved):
                assert table is rec.table and isinstance(resolved, sparse_rx.BoostResolver)

            def __call__(self, doc, score, count, keep):
                return cut("boost", doc, score, count, keep)

        def hybrid_search(index, q_ptr, q_term, q_weight, dense_search, ka, kb, k, mode, weights, rrf_c, rescore=False, dense_score=None, post=None, **kw):
            rec.fused.append((ka, kb, k))
            nq = len(q_ptr) - 1
            out = torch.arange(k, dtype=torch.int32).repeat(nq, 1), torch.ones((nq, k)), torch.full((nq,), k, dtype=torch.int32)
            rec.post = post
            if post is not None:
                out = post(*out)
                assert len(out) == 3
            return tuple(t.numpy() for t in out)

        svc._dense, self.tokens, self.table = Dense(), Tokens(), Table()
        svc._be.field_table = lambda: self.table
        monkeypatch.setattr(sparse_rx.boost, "BoostFn", Boost)
        monkeypatch.setattr(service, "hybrid_search", hybrid_search)

    def trace(self, combo, **keywords):
        """One call with the stages of ``combo`` -> ((ka, kb, k), the stage chain, the result)"""
        self.fused, self.stages, self.args = [], [], {}
        keywords = {**{key: value for name in combo for key, value in STAGE_KEYWORDS[name].items()}, **keywords}
        out = self.svc.search_hybrid(Q, V, top_k=TOP_K, **keywords)
        assert len(self.fused) == 1  # the fusion runs once, whatever follows it
        return self.fused[0], self.stages, out


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder(monkeypatch)
    r.svc._late = r.tokens
    return r


def test_the_recorded_table_is_complete():
    assert len(COMBOS) == 12 and set(EXPECTED) == {(c, s) for c in COMBOS for s in SETTINGS}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_depths_and_stage_chain_of_every_combination(rec, setting):
    for combo in COMBOS:
        fused, stages, out = rec.trace(combo, **SETTINGS[setting])
        assert (fused, stages) == EXPECTED[combo, setting], (combo, setting)
        assert (rec.post is None) == (not combo)  # no stage: nothing is added to the pipeline
        assert len(out["a"]) == (stages[-1][2] if stages else TOP_K)
        # every stage got its own keywords, whatever ran before it
        if "late" in combo:
            assert rec.args["late"] == ((1, 3, 4), [3])
        if "collapse" in combo:
            assert rec.args["collapse"] == ("parent", 2, "drop")
        if "mmr" in combo:
            assert rec.args["mmr"] == (0.25, "dot")


def test_anchor_rows(rec):
    """The rows the composition was specified with, spelled out"""
    assert rec.trace(())[:2] == ((5, 5, 5), [])
    assert rec.trace(("late",))[:2] == ((100, 100, 100), [("late", 100, 5)])
    assert rec.trace(("boost", "mmr"))[:2] == ((100, 100, 100), [("boost", 100, 20), ("mmr", 20, 5)])
    assert rec.trace(("boost", "mmr"), **SETTINGS[3])[:2] == ((8, 8, 8), [("boost", 8, 8), ("mmr", 8, 5)])
    # collapse + MMR alone fetch max(top_k, collapse_pool, mmr_pool) rows per side and fuse collapse_pool deep
    assert rec.trace(("collapse", "mmr"), **SETTINGS[3])[:2] == ((20, 20, 9), [("collapse", 9, 9), ("mmr", 9, 5)])
    assert rec.trace(("late", "boost", "collapse"), **SETTINGS[2])[:2] == ((30, 30, 30), [("late", 30, 30), ("boost", 30, 30), ("collapse", 30, 5)])
    assert rec.trace(("boost", "collapse", "mmr"), **SETTINGS[2])[:2] == ((40, 40, 40), [("boost", 40, 40), ("collapse", 40, 12), ("mmr", 12, 5)])


def test_a_pool_keyword_without_its_stage_is_not_looked_at(rec):
    assert rec.trace((), mmr_pool=300, late_pool=5000, boost_pool=7, collapse_pool=0)[:2] == ((5, 5, 5), [])
    assert rec.post is None
    assert rec.trace(("collapse",), mmr_pool=300, late_pool=5000, boost_pool=7000)[:2] == ((100, 100, 100), [("collapse", 100, 5)])
    # with late_query_tokens the boost and collapse pools are not used; collapse_pool is not even range-checked, boost_pool is
    assert rec.trace(("late", "boost", "collapse"), boost_pool=7, collapse_pool=5000)[:2] == (
        (100, 100, 100), [("late", 100, 100), ("boost", 100, 100), ("collapse", 100, 5)])
    assert _message(rec.trace, ("late", "boost"), boost_pool=5000) == "boost_pool must be in [1, 1024], got 5000"


POOL_MESSAGES = {"mmr_pool": "mmr_pool must be in [1, 256], got 257", "late_pool": "late_pool must be in [1, 1024], got 1025",
                 "collapse_pool": "collapse_pool must be in [1, 1024], got 1025", "boost_pool": "boost_pool must be in [1, 1024], got 1025"}


def _message(fn, *args, **kwargs):
    with pytest.raises(ValueError) as e:
        fn(*args, **kwargs)
    return str(e.value)


def test_pool_messages(rec):
    assert _message(mmr_pool_depth, 10, 257, 10 ** 6) == POOL_MESSAGES["mmr_pool"]
    assert _message(late_pool_depth, 10, 1025, 10 ** 6) == POOL_MESSAGES["late_pool"]
    assert _message(collapse_pool_depth, 10, 1025, 10 ** 6) == POOL_MESSAGES["collapse_pool"]
    assert _message(mmr_pool_depth, 10, 0, 10 ** 6) == "mmr_pool must be in [1, 256], got 0"
    for stage in STAGE_KEYWORDS:
        name = f"{stage}_pool"
        assert _message(rec.trace, (stage,), **{name: 1025 if stage != "mmr" else 257}) == POOL_MESSAGES[name]
    assert _message(rec.trace, ("boost",), boost_pool=0) == "boost_pool must be in [1, 1024], got 0"
    assert not rec.fused and not rec.stages


def test_which_refusal_wins(rec):
    """Two faults in one call: the check that comes first in search_hybrid's order is the one reported"""
    svc, trace = rec.svc, rec.trace
    assert "do not combine" in _message(svc.search_hybrid, Q, V, fusion="nope", mmr_lambda=0.5, **STAGE_KEYWORDS["late"])
    assert "fusion" in _message(trace, (), fusion="nope", rescore=True)
    assert "rescore=True needs fusion='weighted'" in _message(svc.search_hybrid, Q, V, top_k=2000, fusion="rrf", rescore=True)
    assert "at most 1024 rows" in _message(svc.search_hybrid, Q, V, top_k=2000, mmr_lambda=7.0)
    assert "candidates must be >= 1" in _message(trace, ("mmr",), candidates=0, mmr_pool=257)
    assert _message(svc.search_hybrid, Q, V, mmr_lambda=7.0, mmr_pool=257) == "mmr lambda must be in [0, 1], got 7.0"
    assert _message(trace, ("collapse", "mmr"), mmr_pool=257, collapse_pool=1025) == POOL_MESSAGES["mmr_pool"]
    assert _message(trace, ("collapse",), collapse_by="nope", boost_pool=1025, **STAGE_KEYWORDS["boost"]) == "unknown field 'nope'"
    assert _message(trace, ("boost", "collapse"), collapse_pool=1025, boost={"functions": "nope"}) == POOL_MESSAGES["collapse_pool"]
    assert _message(svc.search_hybrid, Q, {}, top_k=TOP_K, boost_pool=1025, **STAGE_KEYWORDS["boost"]) == POOL_MESSAGES["boost_pool"]
    assert _message(svc.search_hybrid, Q, {}, top_k=TOP_K, late_query_tokens={}) == "no query vector for 'a'"
    svc._late = None
    assert _message(svc.search_hybrid, Q, {}, top_k=TOP_K, **STAGE_KEYWORDS["late"]) == "no query vector for 'a'"
    assert "No token index" in _message(trace, ("late",), late_query_tokens={})
    svc._late = rec.tokens
    assert "no query tokens" in _message(trace, ("late",), late_query_tokens={})
    dense, svc._dense = svc._dense, None
    assert _message(trace, ("collapse",), collapse_by="nope") == "No embedding index available"
    host, svc._be.host = svc._be.host, None
    assert _message(trace, ()) == "BM25 index not built. Call build_bm25_index() first."
    svc._be.host, svc._dense = host, dense
    svc._be.sharded = lambda: True
    assert _message(trace, ("late",), late_pool=1025) == POOL_MESSAGES["late_pool"]
    svc._be.host = None
    assert "whole index on one GPU" in _message(trace, ("late",))
    assert not rec.fused and not rec.stages


DOORS = {"set_doc_fields": ({"f": [1]},), "enable_feedback": (), "more_like_this": ({"a": ["d1"]},), "expand_queries": (Q, {"a": {"d1": 1.0}}),
         "facets": (Q, "f"), "facets_of": ({"a": {"d1": 1.0}}, "f"), "search_sorted": (Q, "f"), "sort_results": ({"a": {"d1": 1.0}}, "f"),
         "boost_results": ({"a": {"d1": 1.0}}, {"functions": []})}


def test_the_shared_doors():
    unbuilt = {sparse_rx.RetrievalService: "BM25 index not built. Call build_bm25_index() first.",
               sparse_rx.OptimizedBM25Retriever: "Index not built. Call build_index_from_corpus() first."}
    for cls, message in unbuilt.items():
        obj = cls()
        for door, args in DOORS.items():
            assert _message(getattr(obj, door), *args) == message, (cls, door)
    for door in DOORS:
        a, b = (inspect.signature(getattr(cls, door)) for cls in unbuilt)
        assert a == b, door
        assert getattr(sparse_rx.OptimizedRetriever, door) is getattr(sparse_rx.OptimizedBM25Retriever, door)
