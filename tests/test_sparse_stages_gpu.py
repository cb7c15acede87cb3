"""The sparse search's stages in combinations no other GPU suite runs, on the device: filter + expand + boost, and filter + expand
+ collapse + rank model, each equal -- ids, order and the bits of the scores -- to the list doors chained over the complete
filtered, expanded ranking.  tests/test_sparse_stages_cpu.py pins which entry points such a call reaches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"


def _items(results):
    return {q: [(d, np.float32(s).view(np.uint32)) for d, s in row.items()] for q, row in results.items()}


def test_filter_expand_boost_and_filter_expand_collapse_rank_equal_the_chained_doors():
    import sparse_rx
    from sparse_rx.ltr import ForestModel
    n = 400
    rng = np.random.default_rng(47)
    words = [f"w{i}" for i in range(40)]
    corpus = {f"d{i}": {"text": " ".join(rng.choice(words, size=int(rng.integers(5, 30))))} for i in range(n)}
    queries = {"q1": "w1 w2", "q2": "w7", "q3": "w1 w2", "blank": " "}
    fields = {"votes": rng.integers(0, 1000, n).astype(np.int32), "parent": (rng.permutation(n) // 3).astype(np.int64),
              "flag": (np.arange(n) % 3 != 0).astype(np.int32)}
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(corpus)
    svc.set_doc_fields(fields)
    svc.enable_feedback()
    svc._be.boost_page = 16
    kw = dict(expand_docs=5, expand_terms=6, where={"q1": {"must": [{"field": "flag", "eq": 1}]}, "q2": {"must": [{"field": "flag", "eq": 1}]}},
              excluded_docs={"q3": [f"d{i}" for i in range(0, n, 2)]})
    full = svc.search_bm25(queries, top_k=n, **kw)  # the complete ranking of the expanded queries over their allowed docs
    assert 100 < len(full["q1"]) < n and 100 < len(full["q3"]) <= n // 2 and full["blank"] == {}
    assert list(full["q1"]) != list(full["q3"])  # equal texts under different filter rows: rows of their own

    calls = []
    search_device = svc._be.dev.search_device
    svc._be.dev.search_device = lambda *args, **kwargs: (calls.append(args[3]), search_device(*args, **kwargs))[1]
    # a boost of up to 31.6 next to scores of the expanded queries of about 1: no early page bounds the rest of a ranking
    spec = {"functions": [{"field_value": {"field": "votes", "lo": 0, "hi": 1000, "modifier": "sqrt", "factor": 1.0}}], "boost_mode": "sum"}
    got = svc.search_bm25(queries, top_k=8, boost=spec, **kw)
    assert calls[0] == 5 and calls[1] == 16 and len(calls) >= 4  # the first pass, then at least three pages of 16
    assert _items(got) == _items(svc.boost_results(full, spec, top_k=8)) and len(got["q2"]) == 8 and got["blank"] == {}

    del calls[:]
    model = ForestModel.from_arrays([0, 1, -1, -1, -1], np.float32([0.05, 500.0, 1.0, 2.0, 3.0]), [1, 2, 0, 0, 0], [4, 3, 0, 0, 0], [0, 5])
    svc.set_rank_model(model, ["score", "votes"])
    got = svc.search_bm25(queries, top_k=6, collapse_by="parent", per_group=2, rank_model=True, rank_pool=40, **kw)
    assert calls[:2] == [5, 160]  # the first pass, then the collapse door's first fetch for a pool of 40
    want = svc.rerank_model(svc.collapse(full, "parent", top_k=40, per_group=2), 6)
    assert _items(got) == _items(want) and len(got["q1"]) == 6 and got["blank"] == {}
    svc.close()
