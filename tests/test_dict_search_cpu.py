"""The cached batched dict search of the three API mirrors -- ``RetrievalService.search_bm25``,
``OptimizedBM25Retriever.search``, ``OptimizedRetriever.search`` -- pinned rule by rule: which texts are searched, which
are cached under which key, and what a cache hit returns.  No GPU: every rank of a gloo group of two runs the mirrors
over the CPU oracle (the searcher factory of test_distributed_cpu), wrapped so that every factory call and every search
call (rows, k) is counted.  One pair of workers serves all cases."""
import json
import os
import tempfile
import traceback

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from test_distributed_cpu import _free_port, _oracle_searcher_factory

WORLD = 2
CASES = ("service", "service_k1", "bm25", "bm25_nocache", "pipeline_8gb", "pipeline_2gb")


class _Counted:
    """The oracle searcher factory, counting: ``factory_calls`` and ``calls`` = [(rows, k)] of every search."""

    def __init__(self):
        self.factory_calls = 0
        self.calls = []

    def __call__(self, host, doc_base, mode, k1, b, group):
        self.factory_calls += 1
        s = _oracle_searcher_factory(host, doc_base, mode, k1, b, group)
        inner = s.search

        def search(q_ptr, q_term, q_weight, k, **kw):
            self.calls.append((int(q_ptr.shape[0]) - 1, int(k)))
            return inner(q_ptr, q_term, q_weight, k, **kw)

        s.search = search
        return s

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def _make(case, corpus, tmp):
    """(object, its search method, counted factory, blank text searched?, cache key stripped?, cached?)"""
    import sparse_rx
    f = _Counted()
    if case.startswith("service"):
        o = sparse_rx.RetrievalService(shard_searcher_factory=f)
        o.build_bm25_index(corpus)
        return o, o.search_bm25, f, False, True, True
    if case.startswith("bm25"):
        o = sparse_rx.OptimizedBM25Retriever(shard_searcher_factory=f, cache_queries=case == "bm25")
        o.build_index_from_corpus(corpus)
        return o, o.search, f, True, True, case == "bm25"
    gb = 8 if case == "pipeline_8gb" else 2
    o = sparse_rx.OptimizedRetriever({"type": "bm25"}, hardware_info={"memory_gb": gb}, cache_dir=os.path.join(tmp, case),
                                     shard_searcher_factory=f)
    o.build_index_from_corpus(corpus)
    return o, o.search, f, True, False, gb > 4


def _check_rules(case, corpus, queries, tmp):
    o, search, f, blank_searched, strip, cached = _make(case, corpus, tmp)
    n_docs = len(corpus)
    t = [queries[f"q{i}"] for i in range(8)]
    assert f.factory_calls == 1 and f.take() == []
    if cached:
        assert o.query_cache == {}
    else:
        assert o.query_cache is None
    size = (lambda: len(o.query_cache)) if cached else (lambda: 0)

    def positive(res):
        for d in res.values():
            assert all(isinstance(k, str) for k in d) and all(isinstance(v, float) and v > 0 for v in d.values())  # score > 0 only

    # every qid in the caller's order, blank ones included; "" is never searched; "   " is blank on the service only, and
    # on the registry classes an empty row that is searched but not cached
    r = search({"a": t[0], "b": "", "c": t[1], "d": "   "}, top_k=10)
    assert list(r) == ["a", "b", "c", "d"] and r["b"] == {} and r["d"] == {}
    assert 0 < len(r["a"]) <= 10 and 0 < len(r["c"]) <= 10
    positive(r)
    assert f.take() == [(3 if blank_searched else 2, 10)]
    assert size() == (2 if cached else 0)
    assert search({"x": ""}, top_k=10) == {"x": {}} and f.take() == []
    r_blank = search({"y": "   "}, top_k=10)
    assert r_blank == {"y": {}} and f.take() == ([(1, 10)] if blank_searched else []) and size() == (2 if cached else 0)

    # a second identical call searches nothing new and returns an equal result (fresh dicts, not the first call's)
    r2 = search({"a": t[0], "b": "", "c": t[1], "d": "   "}, top_k=10)
    assert r2 == r and list(r2) == list(r) and r2["a"] is not r["a"]
    if cached:
        assert f.take() == ([(1, 10)] if blank_searched else [])  # only the uncacheable blank row
    else:
        assert f.take() == [(3, 10)]  # cache_queries=False / memory_gb <= 4: every call searches
        assert o.query_cache is None

    # two qids with one text: one row, equal but distinct dicts
    r = search({"p": t[2], "q": t[2]}, top_k=10)
    assert f.take() == [(1, 10)] and r["p"] == r["q"] and r["p"] and r["p"] is not r["q"]
    before = size()

    # " foo " and "foo": one cache entry where the key is stripped, two where it is not; the rows are the same either way
    ra = search({"u": f" {t[3]} "}, top_k=10)
    assert f.take() == [(1, 10)]
    rb = search({"v": t[3]}, top_k=10)
    assert ra["u"] == rb["v"] and ra["u"]
    if cached and strip:
        assert f.take() == [] and size() == before + 1 and f"{t[3]}:10" in o.query_cache
    elif cached:
        assert f.take() == [(1, 10)] and size() == before + 2 and {f" {t[3]} :10", f"{t[3]}:10"} <= set(o.query_cache)
    else:
        assert f.take() == [(1, 10)]

    # the same text with another top_k is another entry
    before = size()
    r3 = search({"v": t[3]}, top_k=3)
    assert f.take() == [(1, 3)] and 0 < len(r3["v"]) <= 3 and list(r3["v"]) == list(rb["v"])[:len(r3["v"])]
    assert size() == before + (1 if cached else 0)

    # an all-out-of-vocabulary query: {} and nothing cached
    before = size()
    assert search({"o": "zzzzzz qqqqqq"}, top_k=10) == {"o": {}} and size() == before
    assert f.take() == [(1, 10)]

    # top_k <= 0: {} for every qid, no search call
    for k in (0, -3):
        assert search({"a": t[0], "b": "", "n": t[4]}, top_k=k) == {"a": {}, "b": {}, "n": {}}
        assert f.take() == []
    assert size() == before

    # top_k beyond the corpus asks the backend for n_docs rows
    r = search({"n": t[4]}, top_k=10 ** 6)
    assert f.take() == [(1, n_docs)] and 0 < len(r["n"]) <= n_docs
    positive(r)

    # a full cache (1 000 entries) does not grow: the query is answered, not stored, and searched again next time
    if cached:
        o.query_cache.clear()
        for i in range(1000):
            o.query_cache[f"dummy{i}:10"] = (np.zeros(0, np.int64), np.zeros(0, np.float32))
        r = search({"m": t[5]}, top_k=10)
        assert r["m"] and f.take() == [(1, 10)] and len(o.query_cache) == 1000
        assert search({"m": t[5]}, top_k=10) == r and f.take() == [(1, 10)] and len(o.query_cache) == 1000
        assert search({"h": "dummy7"}, top_k=10) == {"h": {}} and f.take() == []  # a stored entry is a hit
    assert f.factory_calls == 1
    o.close()


def _check_service_k1(corpus, queries, tmp):
    """k1 / b are plain attributes: assigning one makes the next search upload again and empties the cache."""
    o, search, f, *_ = _make("service_k1", corpus, tmp)
    t = [queries[f"q{i}"] for i in range(3)]
    r = search({"a": t[0], "c": t[1]}, top_k=10)
    assert f.factory_calls == 1 and f.take() == [(2, 10)] and len(o.query_cache) == 2
    o.k1 = 0.9
    assert search({"a": t[0]}, top_k=0) == {"a": {}} and f.factory_calls == 1 and len(o.query_cache) == 2  # nothing to search: no upload
    r2 = search({"a": t[0], "e": t[2]}, top_k=10)
    assert f.factory_calls == 2 and f.take() == [(2, 10)]  # "a" is searched again: its entry went with the upload
    assert set(o.query_cache) == {f"{t[0]}:10", f"{t[2]}:10"}
    assert set(r2["a"]) and r2["a"] != r["a"]  # other impacts, other scores
    search({"a": t[0]}, top_k=10)
    assert f.factory_calls == 2 and f.take() == []
    o.close()


def _worker(rank, world, port, golden_dir, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as fh:
        j = json.load(fh)
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            try:
                if case == "service_k1":
                    _check_service_k1(j["corpus"], j["queries"], tmp)
                else:
                    _check_rules(case, j["corpus"], j["queries"], tmp)
                ret[(rank, case)] = "ok"
            except Exception:
                ret[(rank, case)] = traceback.format_exc()
                break  # the ranks may no longer be in step: the remaining cases are reported as not run
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def outcomes(golden_dir):
    ctx = mp.get_context("spawn")
    with ctx.Manager() as m:
        ret = m.dict()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, WORLD, port, golden_dir, ret)) for r in range(WORLD)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=300)
        for p in procs:
            if p.is_alive():
                p.kill()
        return dict(ret), [p.exitcode for p in procs]


@pytest.mark.parametrize("case", CASES)
def test_dict_search_rules(outcomes, case):
    ret, exitcodes = outcomes
    for rank in range(WORLD):
        assert ret.get((rank, case), f"not run (worker exit codes {exitcodes})") == "ok"
