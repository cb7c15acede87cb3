"""What the sparse search composes on the host, without a GPU: the calls the three pagers (``deep_search``, ``collapse_deep``,
``boost_deep``) make of their search and reduce functions; the device entry points ``SparseBackend.search_dicts`` reaches for
every legal subset of {filter, expand, collapse, boost}, with recorders in their place; what ``search_bm25`` and the registry
mirrors' ``search`` hand to the pooled pass and to the model rerank, and which refusal wins when a call has two faults; and the
three list doors (``boost_results``, ``rerank_model``, ``sort_results``) over CPU fakes.

The expected values are literals recorded from the hand-written loops, routes and doors this composition replaced -- they are
not computed from a restatement of its rule."""
import itertools
import threading

import numpy as np
import pytest
import torch

import sparse_rx
from sparse_rx import _capi
from sparse_rx.backend import SparseBackend, collapse_deep
from sparse_rx.boost import boost_deep
from sparse_rx.filter import DocFilter
from sparse_rx.index import deep_search


def _message(fn, *args, **kwargs):
    with pytest.raises(ValueError) as e:
        fn(*args, **kwargs)
    return str(e.value)


# ---- the pagers ---------------------------------------------------------------------------------------------------------------
# three rankings of (doc, score), best first; the group of a doc is doc // 100
RANKINGS = [[(100 * i, float(s)) for i, s in enumerate([100, 99, 98, 10, 9, 8, 7, 6, 5, 4])],          # 10 rows, 10 groups
            [(1000 + 100 * (i % 2) + i // 2, 50.0 - 0.5 * i) for i in range(18)],                      # 18 rows, 2 groups
            [(2000 + i, 40.0 - 0.25 * i) for i in range(40)]]                                          # 40 rows, 1 group
BATCH = (torch.zeros(4, dtype=torch.int32), torch.empty(0, dtype=torch.int32), torch.empty(0, dtype=torch.float32))


class _PagedSearch:
    """``search_fn`` over fixed rankings: the rows ranked strictly after the cursor, a cursor of score 0 ends a ranking"""

    def __init__(self, rankings):
        self.rankings, self.calls = rankings, []

    def __call__(self, q_ptr, q_term, q_weight, kk, **kw):
        assert q_ptr.numel() == len(self.rankings) + 1 and q_term is BATCH[1] and q_weight is BATCH[2]  # the batch goes through as it is
        if "after" in kw:
            a_doc, a_score = kw["after"]
            assert a_doc.dtype == torch.int32 and a_score.dtype == torch.float32 and a_doc.is_contiguous() and a_score.is_contiguous()
            self.calls.append((kk, a_doc.tolist(), a_score.tolist()))
        else:
            self.calls.append((kk, None, None))
        nq = len(self.rankings)
        d = torch.full((nq, kk), -1, dtype=torch.int32)
        s, c = torch.zeros((nq, kk)), torch.zeros(nq, dtype=torch.int32)
        for q, rows in enumerate(self.rankings):
            if "after" in kw:
                ad, sc = int(a_doc[q]), float(a_score[q])
                rows = [] if sc == 0.0 else [(doc, v) for doc, v in rows if v < sc or (v == sc and doc > ad)]
            for j, (doc, v) in enumerate(rows[:kk]):
                d[q, j], s[q, j] = doc, v
            c[q] = min(kk, len(rows))
        return d, s, c


def _collapse_fn(log):
    def fn(d, s, c, kk):  # one row per group (doc // 100), a doc id of -1 is dead
        log.append((int(d.shape[1]), None, c is None, kk))
        assert d.is_contiguous() and s.is_contiguous() and 1 <= kk <= d.shape[1]
        nq = d.shape[0]
        od, os_, oc = torch.full((nq, kk), -1, dtype=torch.int32), torch.zeros((nq, kk)), torch.zeros(nq, dtype=torch.int32)
        for q in range(nq):
            seen = set()
            for j in range(d.shape[1] if c is None else int(c[q])):
                doc = int(d[q, j])
                if doc >= 0 and doc // 100 not in seen and len(seen) < kk:
                    od[q, len(seen)], os_[q, len(seen)] = doc, s[q, j]
                    seen.add(doc // 100)
            oc[q] = len(seen)
        return od, os_, oc
    return fn


class _BoostOne:
    """``boost_fn`` whose factor is 1 for every doc, with the bounds of a factor in [0.5, 2]"""
    boost_mode, F_lo, F_hi = "multiply", 0.5, 2.0

    def __init__(self, log):
        self.log = log

    def __call__(self, d, s, c, kk, carry=None, want_pos=False):
        self.log.append((int(d.shape[1]), None if carry is None else int(carry[0].shape[1]), c is None, kk))
        assert d.is_contiguous() and s.is_contiguous() and kk >= 1
        assert carry is None or all(t.is_contiguous() for t in carry)
        nq = d.shape[0]
        od, os_, oc = torch.full((nq, kk), -1, dtype=torch.int32), torch.zeros((nq, kk)), torch.zeros(nq, dtype=torch.int32)
        for q in range(nq):
            rows = [(float(s[q, j]), int(d[q, j])) for j in range(d.shape[1] if c is None else int(c[q]))]
            if carry is not None:
                rows += [(float(carry[1][q, j]), int(carry[0][q, j])) for j in range(int(carry[2][q]))]
            rows = sorted(rows, key=lambda r: (-r[0], r[1]))[:kk]
            for j, (v, doc) in enumerate(rows):
                od[q, j], os_[q, j] = doc, v
            oc[q] = len(rows)
        return od, os_, oc


def _paged(door, max_depth, k=3, rankings=RANKINGS, first=8, page=8):
    """One run of a paged door -> (the search calls, the reduce calls, the kept docs, the kept counts)"""
    search, log = _PagedSearch(rankings), []
    reduce_fn = _collapse_fn(log) if door is collapse_deep else _BoostOne(log)
    batch = (torch.zeros(len(rankings) + 1, dtype=torch.int32),) + BATCH[1:]
    kd, ks, kc = door(search, reduce_fn, *batch, k, first, page=page, max_depth=max_depth)
    assert kd.shape == ks.shape == (len(rankings), k)
    return search.calls, log, kd.tolist(), kc.tolist()


def test_collapse_deep_trace():
    # query 0 holds 3 groups after page 1; query 1 is exhausted by its short page 3; query 2 still wants more at 20 rows
    assert _paged(collapse_deep, 20) == (
        [(8, None, None), (8, [0, 1103, 2007], [0.0, 46.5, 38.25]), (4, [0, 1107, 2015], [0.0, 42.5, 36.25])],
        [(8, None, False, 3), (11, None, True, 3), (7, None, True, 3)],
        [[0, 100, 200], [1000, 1100, -1], [2000, -1, -1]], [3, 2, 1])
    assert _paged(collapse_deep, None) == (
        [(8, None, None), (8, [0, 1103, 2007], [0.0, 46.5, 38.25]), (8, [0, 1107, 2015], [0.0, 42.5, 36.25]),
         (8, [0, 0, 2023], [0.0, 0.0, 34.25]), (8, [0, 0, 2031], [0.0, 0.0, 32.25]), (8, [0, 0, 2039], [0.0, 0.0, 30.25])],
        [(8, None, False, 3), (11, None, True, 3), (11, None, True, 3), (11, None, True, 3), (11, None, True, 3), (11, None, True, 3)],
        [[0, 100, 200], [1000, 1100, -1], [2000, -1, -1]], [3, 2, 1])


def test_collapse_deep_edges():
    # first is clamped by max_depth; a list shallower than k is padded to k columns; nobody active: one search call
    assert _paged(collapse_deep, 2) == ([(2, None, None)], [(2, None, False, 2)], [[0, 100, -1], [1000, 1100, -1], [2000, -1, -1]], [2, 2, 1])
    assert _paged(collapse_deep, None, rankings=RANKINGS[:1]) == ([(8, None, None)], [(8, None, False, 3)], [[0, 100, 200]], [3])


def test_boost_deep_trace():
    # query 0 settles on page 1 (2 * 6 < 98); query 1 is exhausted by its short page 3; query 2 still wants more at 20 rows
    assert _paged(boost_deep, 20) == (
        [(8, None, None), (8, [0, 1103, 2007], [0.0, 46.5, 38.25]), (4, [0, 1107, 2015], [0.0, 42.5, 36.25])],
        [(8, None, False, 3), (8, 3, False, 3), (4, 3, False, 3)],
        [[0, 100, 200], [1000, 1100, 1001], [2000, 2001, 2002]], [3, 3, 3])
    assert _paged(boost_deep, None) == (
        [(8, None, None), (8, [0, 1103, 2007], [0.0, 46.5, 38.25]), (8, [0, 1107, 2015], [0.0, 42.5, 36.25]),
         (8, [0, 0, 2023], [0.0, 0.0, 34.25]), (8, [0, 0, 2031], [0.0, 0.0, 32.25]), (8, [0, 0, 2039], [0.0, 0.0, 30.25])],
        [(8, None, False, 3), (8, 3, False, 3), (8, 3, False, 3), (8, 3, False, 3), (8, 3, False, 3), (8, 3, False, 3)],
        [[0, 100, 200], [1000, 1100, 1001], [2000, 2001, 2002]], [3, 3, 3])


def test_boost_deep_reads_on_at_a_tie():
    """bound == k-th score is not settled: an unseen doc with a lower id could tie"""
    tie = [[(7, 8.0), (9, 4.0), (11, 3.0), (12, 2.0), (13, 1.0)]]
    assert _paged(boost_deep, None, k=1, rankings=tie, first=2, page=2) == (
        [(2, None, None), (2, [9], [4.0])], [(2, None, False, 1), (2, 1, False, 1)], [[7]], [1])
    below = [[(7, 8.5), (9, 4.0), (11, 3.0), (12, 2.0), (13, 1.0)]]
    assert _paged(boost_deep, None, k=1, rankings=below, first=2, page=2) == ([(2, None, None)], [(2, None, False, 1)], [[7]], [1])


def test_boost_deep_refusals_come_before_any_search():
    for mode, f_lo, message in (("replace", 0.0, "boost_mode \"replace\" has no bound on an unseen doc: the exact door refuses it (search_sorted orders by a field alone)"),
                                ("nope", 0.0, "unknown boost_mode 'nope'"),
                                ("multiply", -0.5, "boost_mode \"multiply\" with a factor that can be negative (F_lo = -0.5) has no bound on an unseen doc: "
                                                   "the exact door refuses it")):
        search, fn = _PagedSearch(RANKINGS), _BoostOne([])
        fn.boost_mode, fn.F_lo = mode, f_lo
        assert _message(boost_deep, search, fn, *BATCH, 3, 8, page=8) == message
        assert not search.calls and not fn.log


def test_deep_search_trace():
    search = _PagedSearch(RANKINGS)  # query 0 is exhausted on page 2
    d, s, c = deep_search(search, *BATCH, 20, 8)
    assert search.calls == [(8, None, None), (8, [700, 1103, 2007], [6.0, 46.5, 38.25]), (4, [0, 1107, 2015], [0.0, 42.5, 36.25])]
    assert c.tolist() == [10, 18, 20] and d.shape == s.shape == (3, 20)
    assert d[0].tolist() == [100 * i for i in range(10)] + [-1] * 10 and d[2].tolist() == list(range(2000, 2020))
    search = _PagedSearch(RANKINGS)  # k <= page: one call, handed through
    assert deep_search(search, *BATCH, 8, 8)[2].tolist() == [8, 8, 8] and search.calls == [(8, None, None)]
    search = _PagedSearch(RANKINGS[:1])  # everybody exhausted on page 2: no third call
    assert deep_search(search, torch.zeros(2, dtype=torch.int32), *BATCH[1:], 20, 8)[2].tolist() == [10]
    assert search.calls == [(8, None, None), (8, [700], [6.0])]


# ---- the route from a host batch to host rows -----------------------------------------------------------------------------------
N_DOCS = 1100  # above the engine's list depth, so that top_k = 1025 stays 1025
BOOST = {"functions": [{"field_value": {"field": "price", "lo": 0.0, "hi": 50.0}}], "boost_mode": "sum"}
QUERIES = {"a": "alpha w3", "b": "beta w5 w9", "c": "alpha w3"}


def _corpus():
    return {f"d{i}": {"text": f"alpha beta w{i} w{i % 7}"} for i in range(N_DOCS)}


def _columns():
    return {"parent": [i // 4 for i in range(N_DOCS)], "price": np.linspace(0.0, 50.0, N_DOCS, dtype=np.float32)}


def _rows_after(after, q, kk):
    """Every query ranks doc i at score N_DOCS - i: the rows behind the cursor of query ``q``"""
    start = 0
    if after is not None:
        start = N_DOCS if float(after[1][q]) == 0.0 else int(after[0][q]) + 1
    return list(range(start, min(start + kk, N_DOCS)))


class _Route:
    """A backend over a 1100-doc host index (nothing is uploaded) whose device index, forward index, field table and BoostFn are
    recorders over CPU tensors"""

    def __init__(self, monkeypatch):
        self.events = []
        be = self.be = SparseBackend("cpu", 14)
        be.build(_corpus(), idf_kind="bm25")
        be.set_fields(_columns())
        be.boost_page = 16
        rec = self

        def block(nq, kk, after):
            d, s, c = np.full((nq, kk), -1, np.int32), np.zeros((nq, kk), np.float32), np.zeros(nq, np.int32)
            for q in range(nq):
                rows = _rows_after(after, q, kk)
                d[q, : len(rows)], s[q, : len(rows)], c[q] = rows, [N_DOCS - r for r in rows], len(rows)
            return d, s, c

        class Dev:
            device, n_docs, doc_base = torch.device("cpu"), N_DOCS, 0

            def search(self, q_ptr, q_term, q_weight, k, filter=None, q_filter=None):
                assert isinstance(q_ptr, np.ndarray) and (q_filter is None or isinstance(q_filter, np.ndarray))
                rec.events.append(("dev.search", k, filter is not None, q_filter is not None))
                return block(len(q_ptr) - 1, k, None)

            def search_device(self, qp, qt, qw, kk, out=None, after=None, filter=None, q_filter=None):
                assert isinstance(qp, torch.Tensor) and (q_filter is None or isinstance(q_filter, torch.Tensor))
                rec.events.append(("dev.search_device", kk, after is not None, filter is not None, q_filter is not None))
                return tuple(torch.from_numpy(a) for a in block(qp.numel() - 1, kk, after))

        class Forward:
            def expand_device(self, qp, qt, qw, d, s, c, **kw):
                rec.events.append(("expand_device", kw["fb_docs"], int(d.shape[1]), s is not None, kw["alpha"], kw["beta"], kw["doc_weight"]))
                return qp, qt, qw, None

            def close(self):
                pass

        class Table:
            device, columns = "cpu", be._fields

            def collapse_device(self, by, d, s, c, kk, per_group, nulls):  # groups of 400 docs
                rec.events.append(("collapse_device", by, int(d.shape[1]), c is None, kk, per_group, nulls))
                nq = d.shape[0]
                od, os_, oc = torch.full((nq, kk), -1, dtype=torch.int32), torch.zeros((nq, kk)), torch.zeros(nq, dtype=torch.int32)
                for q in range(nq):
                    seen, n = {}, 0
                    for j in range(d.shape[1] if c is None else int(c[q])):
                        doc = int(d[q, j])
                        if doc >= 0 and seen.get(doc // 400, 0) < per_group and n < kk:
                            od[q, n], os_[q, n] = doc, s[q, j]
                            seen[doc // 400] = seen.get(doc // 400, 0) + 1
                            n += 1
                    oc[q] = n
                return od, os_, oc

            def close(self):
                pass

        class Boost(_BoostOne):
            def __init__(self, table, resolved):
                assert table is rec.table and isinstance(resolved, sparse_rx.BoostResolver)
                self.boost_mode, self.F_lo, self.F_hi = resolved.boost_mode_name, resolved.F_lo, resolved.F_hi
                self.log = _Tagged(rec.events, "boost_fn")

        def search_arrays(q_ptr, q_term, q_weight, k):
            rec.events.append(("search_arrays", k))
            return block(len(q_ptr) - 1, k, None)

        self.table = Table()
        be.dev, be._forward, be.field_table, be.search_arrays = Dev(), Forward(), lambda: self.table, search_arrays
        monkeypatch.setattr(sparse_rx.boost, "BoostFn", Boost)
        self.filter = _FilterSpec({"a": 0, "b": 1, "c": 1})

    def specs(self, combo, k):
        be = self.be
        return dict(filter=self.filter if "filter" in combo else None,
                    collapse=be.collapse_spec("parent" if "collapse" in combo else None, 2, "drop", None, k),
                    expand=be.expand_spec(4 if "expand" in combo else None, 10, 0.25, "uniform"),
                    boost=be.boost_spec(BOOST if "boost" in combo else None, None, k))

    def trace(self, combo, k, **keywords):
        self.events = []
        out = self.be.search_dicts(QUERIES, k, **self.specs(combo, k), **keywords)
        assert list(out) == list(QUERIES)
        return self.events, [len(row) for row in out.values()]


class _Tagged:
    def __init__(self, events, tag):
        self.events, self.tag = events, tag

    def append(self, item):
        self.events.append((self.tag,) + item)


class _FilterSpec:
    """What ``filter_spec`` returns, over a two-row filter on the CPU"""

    def __init__(self, row_of_qid):
        self.row_of_qid, self.asked = row_of_qid, 0

    def on_device(self, index):
        self.asked += 1
        return DocFilter.from_masks(np.ones((2, N_DOCS), dtype=bool), device="cpu", doc_base=0)


@pytest.fixture
def route(monkeypatch):
    return _Route(monkeypatch)


STAGES = ("filter", "expand", "collapse", "boost")
COMBOS = [c for n in range(5) for c in itertools.combinations(STAGES, n) if not ("collapse" in c and "boost" in c)]
SD, T, F = "dev.search_device", True, False
FIRST_PASS = ("expand_device", 4, 4, True, 0.75, 0.25, "uniform")
COLLAPSED = [("collapse_device", "parent", 64, False, 5, 2, "drop"), ("collapse_device", "parent", 1029, True, 5, 2, "drop")]
BOOSTED = [("boost_fn", 16, None, False, 5), ("boost_fn", 16, 5, False, 5), ("boost_fn", 16, 5, False, 5), ("boost_fn", 16, 5, False, 5)]


def _paged_route(first, page, reduced, flt, n_pages):
    """search and reduce calls in turn: page 1 at ``first``, ``n_pages - 1`` further ones at ``page``"""
    searches = [(SD, first, F, flt, flt)] + [(SD, page, T, flt, flt)] * (n_pages - 1)
    return [e for pair in zip(searches, reduced) for e in pair]


# (combination, top_k) -> the entry points hit, in order.  "a" and "c" share a text: one row, unless their filter rows differ
EXPECTED_ROUTE = {
    ((), 5): [("search_arrays", 5)],
    ((), 1025): [("search_arrays", 1025)],
    (("filter",), 5): [("dev.search", 5, T, T)],
    (("filter",), 1025): [("dev.search", 1025, T, T)],
    (("expand",), 5): [(SD, 4, F, F, F), FIRST_PASS, (SD, 5, F, F, F)],
    (("expand",), 1025): [(SD, 4, F, F, F), FIRST_PASS, ("dev.search", 1025, F, F)],
    (("collapse",), 5): _paged_route(64, 1024, COLLAPSED, F, 2),
    (("boost",), 5): _paged_route(16, 16, BOOSTED, F, 4),
    (("filter", "expand"), 5): [(SD, 4, F, T, T), FIRST_PASS, (SD, 5, F, T, T)],
    (("filter", "expand"), 1025): [(SD, 4, F, T, T), FIRST_PASS, ("dev.search", 1025, T, T)],
    (("filter", "collapse"), 5): _paged_route(64, 1024, COLLAPSED, T, 2),
    (("filter", "boost"), 5): _paged_route(16, 16, BOOSTED, T, 4),
    (("expand", "collapse"), 5): [(SD, 4, F, F, F), FIRST_PASS] + _paged_route(64, 1024, COLLAPSED, F, 2),
    (("expand", "boost"), 5): [(SD, 4, F, F, F), FIRST_PASS] + _paged_route(16, 16, BOOSTED, F, 4),
    (("filter", "expand", "collapse"), 5): [(SD, 4, F, T, T), FIRST_PASS] + _paged_route(64, 1024, COLLAPSED, T, 2),
    (("filter", "expand", "boost"), 5): [(SD, 4, F, T, T), FIRST_PASS] + _paged_route(16, 16, BOOSTED, T, 4),
}


def test_the_recorded_routes_are_complete():
    assert len(COMBOS) == 12
    assert set(EXPECTED_ROUTE) == {(c, k) for c in COMBOS for k in (5, 1025) if k == 5 or not ({"collapse", "boost"} & set(c))}


def test_route_of_every_combination(route):
    for (combo, k), expected in EXPECTED_ROUTE.items():
        events, sizes = route.trace(combo, k)
        assert events == expected, (combo, k)
        assert sizes == [k, k, k], (combo, k)
    assert route.filter.asked == 8  # once per filtered call


def test_boost_and_collapse_refuse_each_other(route):
    collapse = route.be.collapse_spec("parent", 2, "drop", None, 5)
    assert _message(route.be.boost_spec, BOOST, None, 5, "search", collapse) == (
        "search: boost= and collapse_by= do not combine in one call (chain collapse() over the boosted result)")
    assert "returns at most 1024 rows per query, got top_k=1025" in _message(route.be.collapse_spec, "parent", 2, "drop", None, 1025)
    assert "returns at most 1024 rows per query, got top_k=1025" in _message(route.be.boost_spec, BOOST, None, 1025)


def test_the_two_first_rules(route):
    """collapse: min(max(4 k, 64), 1024, n_docs) with pages of 1024; boost: min(max(4 k, 64), max(page, k), n_docs) with pages of
    min(boost_page, 1024) -- read off the first two search calls"""
    firsts = lambda combo, k: [e[1] for e in route.trace(combo, k)[0] if e[0] == SD][:2]
    assert firsts(("collapse",), 5) == [64, 1024] and firsts(("collapse",), 300) == [1024, 1024]
    assert firsts(("boost",), 5) == [16, 16] and firsts(("boost",), 40) == [40, 16]
    route.be.boost_page = 4096
    assert firsts(("boost",), 5) == [64] and firsts(("boost",), 300) == [1024]  # settled on page 1
    route.be.n_docs_total = 50
    assert firsts(("boost",), 5) == [50, 1024] and firsts(("collapse",), 5) == [50, 1024]


def test_depth_keywords_reach_the_pagers(route):
    be = route.be
    route.events = []
    be.search_dicts(QUERIES, 5, collapse=be.collapse_spec("parent", 2, "drop", 100, 5))
    assert [e[1] for e in route.events if e[0] == SD] == [64, 36]
    route.events = []
    be.search_dicts(QUERIES, 5, boost=be.boost_spec(BOOST, 40, 5))
    assert [e[1] for e in route.events if e[0] == SD] == [16, 16, 8]


def test_equal_texts_share_a_row_only_under_the_same_filter_row(route):
    seen = []
    route.be.dev.search = lambda q_ptr, q_term, q_weight, k, filter=None, q_filter=None: (
        seen.append((len(q_ptr) - 1, q_filter.tolist())), (np.zeros((len(q_ptr) - 1, k), np.int32), np.zeros((len(q_ptr) - 1, k), np.float32),
                                                            np.zeros(len(q_ptr) - 1, np.int32)))[1]
    route.be.search_dicts(QUERIES, 5, filter=_FilterSpec({"a": 0, "b": 1, "c": 1}))
    route.be.search_dicts(QUERIES, 5, filter=_FilterSpec({"a": 1, "b": 1, "c": 1}))
    assert seen == [(3, [0, 1, 1]), (2, [1, 1])]


def test_an_empty_batch_and_an_all_oov_row(route):
    be = route.be
    for combo in COMBOS:
        route.events = []
        assert be.search_dicts({"a": "", "b": None}, 5, **route.specs(combo, 5)) == {"a": {}, "b": {}}
        assert route.events == []
    cache = {}
    assert be.search_dicts({"a": "zzz qqq", "b": "alpha"}, 5, cache=cache, lock=threading.RLock()) == {"a": {}, "b": {f"d{i}": float(N_DOCS - i) for i in range(5)}}
    assert list(cache) == ["alpha:5"]  # the all-OOV row is searched, answered {} and not cached


def test_more_like_this_route(route):
    be = route.be
    seeds = {"a": ["d1", "d2"], "b": ["d3"]}
    route.events = []
    out = be.more_like_this(seeds, top_k=5, terms=7, include_seeds=True)
    assert route.events == [("expand_device", 2, 2, False, 0.0, 1.0, "uniform"), (SD, 5, F, F, F)]
    assert out == {qid: {f"d{i}": float(N_DOCS - i) for i in range(5)} for qid in seeds}
    route.events = []
    be.filter_spec = lambda *args, **kwargs: _FilterSpec({"a": 0, "b": 1})
    be.more_like_this(seeds, top_k=5, terms=7)
    assert route.events == [("expand_device", 2, 2, False, 0.0, 1.0, "uniform"), (SD, 5, F, T, T)]
    route.events = []
    be.more_like_this(seeds, top_k=2000, terms=7)  # k_eff = 1100: the batch goes to the host once
    assert route.events == [("expand_device", 2, 2, False, 0.0, 1.0, "uniform"), ("dev.search", 1100, T, T)]


def test_cache_rules(route):
    be, lock = route.be, threading.RLock()
    cache = {}
    plain = lambda: route.trace((), 5, cache=cache, lock=lock)[0]
    assert plain() == [("search_arrays", 5)] and sorted(cache) == ["alpha w3:5", "beta w5 w9:5"]
    assert plain() == []  # read
    held = dict(cache)
    for combo in COMBOS[1:]:  # a staged call neither reads nor writes
        assert route.trace(combo, 5, cache=cache, lock=lock)[0] == EXPECTED_ROUTE[combo, 5]
        assert cache == held and all(cache[key] is held[key] for key in held)
    full = {f"x{i}": None for i in range(1000)}
    assert route.trace((), 5, cache=full, lock=lock)[0] == [("search_arrays", 5)] and len(full) == 1000
    nearly = {f"x{i}": None for i in range(999)}
    route.trace((), 5, cache=nearly, lock=lock)
    assert len(nearly) == 1000 and "alpha w3:5" in nearly and "beta w5 w9:5" not in nearly
    # strip_key and blank: the two call sites' rules
    cache = {}
    be.search_dicts({"a": " alpha "}, 5, cache=cache, lock=lock, strip_key=False)
    be.search_dicts({"a": " alpha "}, 5, cache=cache, lock=lock, strip_key=True)
    assert sorted(cache) == [" alpha :5", "alpha:5"]
    route.events = []
    assert be.search_dicts({"a": "  "}, 5, blank="whitespace") == {"a": {}} and route.events == []
    assert be.search_dicts({"a": "  "}, 5, blank="empty") == {"a": {}} and route.events == [("search_arrays", 5)]


# ---- the search doors -----------------------------------------------------------------------------------------------------------
DOOR_STAGES = {"filter": dict(allowed_docs=["d1", "d2", "d3"]), "terms": dict(must_terms=["alpha"], operators=True),
               "where": dict(where={"must": [{"field": "parent", "gte": 2}]}),
               "collapse": dict(collapse_by="parent", per_group=2, collapse_nulls="drop", collapse_depth=500),
               "expand": dict(expand_docs=4, expand_terms=7, expand_weight=0.25, expand_by="uniform")}
DOOR_Q = {"a": "alpha +w3 -w4", "b": "   ", "c": ""}


def _model():
    return sparse_rx.ForestModel.from_arrays(np.array([0, -1, -1]), np.array([0.5, 1.0, 2.0], dtype=np.float32), np.array([1, 0, 0]), np.array([2, 0, 0]), [0, 3])


class _Door:
    """An API mirror over a 300-doc host index (nothing is uploaded) whose ``search_dicts`` and ``rerank_model_results`` are recorders"""

    def __init__(self, cls, fields=True, forward=True):
        obj = self.obj = cls({"type": "bm25"}) if cls is sparse_rx.OptimizedRetriever else cls()
        self.name = "search_bm25" if cls is sparse_rx.RetrievalService else "search"
        be = self.be = obj._be
        be.build({f"d{i}": {"text": f"alpha beta w{i} w{i % 7}"} for i in range(300)}, idf_kind="bm25")
        if cls is sparse_rx.RetrievalService:
            obj._built_k1b = (obj.k1, obj.b)
        if fields:
            obj.set_doc_fields({"parent": [i // 4 for i in range(300)], "price": np.linspace(0.0, 50.0, 300, dtype=np.float32)})
        if forward:
            be._forward = object()
        obj.set_rank_model(_model(), ["score"])
        self.calls = []

        def search_dicts(queries, top_k, *, order="term", cache=None, lock=None, strip_key=True, blank="empty", filter=None, collapse=None,
                         expand=None, boost=None):
            self.calls.append(("search_dicts", dict(queries), top_k, order, cache is not None, strip_key, blank,
                               None if filter is None else type(filter).__name__,
                               None if collapse is None else (collapse.by, collapse.per_group, collapse.nulls, collapse.depth),
                               None if expand is None else (expand.docs, expand.terms, expand.weight, expand.by),
                               None if boost is None else (boost.boost_mode_name, boost.depth)))
            return {qid: {f"d{i}": float(300 - i) for i in range(min(top_k, 300))} for qid in queries}

        def rerank_model_results(results, top_k=None, extra=None, mode="replace", call="rerank_model"):
            self.calls.append(("rerank_model_results", {qid: len(row) for qid, row in results.items()}, top_k, extra, mode, call))
            return {qid: dict(list(row.items())[:top_k]) for qid, row in results.items()}

        be.search_dicts, be.rerank_model_results = search_dicts, rerank_model_results

    def search(self, *args, **kwargs):
        self.calls = []
        return getattr(self.obj, self.name)(*args, **kwargs)


MIRRORS = [sparse_rx.RetrievalService, sparse_rx.OptimizedBM25Retriever, sparse_rx.OptimizedRetriever]
# what differs between the doors: (order, an always-on cache, strip_key, blank)
DOOR_SETTINGS = {sparse_rx.RetrievalService: ("term", True, True, "whitespace"), sparse_rx.OptimizedBM25Retriever: ("term", True, True, "empty"),
                 sparse_rx.OptimizedRetriever: ("token", True, False, "empty")}


@pytest.mark.parametrize("cls", MIRRORS)
def test_rank_model_with_every_other_stage(cls):
    door = _Door(cls)
    keywords = {key: value for stage in DOOR_STAGES.values() for key, value in stage.items()}
    out = door.search(DOOR_Q, 7, rank_model=True, rank_pool=40, **keywords)
    assert {qid: len(row) for qid, row in out.items()} == {"a": 7, "b": 7, "c": 7}
    scored = {"a": "alpha w3", "b": "", "c": ""}  # operators=True: the + word stays in the scored text, the - word leaves it
    assert door.calls == [("search_dicts", scored, 40) + DOOR_SETTINGS[cls] + ("FieldFilterSpec", ("parent", 2, "drop", 500), (4, 7, 0.25, "uniform"), None),
                          ("rerank_model_results", {"a": 40, "b": 40, "c": 40}, 7, None, "replace", door.name)]
    door.search(DOOR_Q, 7, rank_model=True)  # the default pool: min(max(4 * 7, 100), 1024, 300)
    assert door.calls == [("search_dicts", DOOR_Q, 100) + DOOR_SETTINGS[cls] + (None, None, None, None),
                          ("rerank_model_results", {"a": 100, "b": 100, "c": 100}, 7, None, "replace", door.name)]
    door.search(DOOR_Q, 7, boost=BOOST, boost_depth=50, **DOOR_STAGES["expand"])  # no model: one pass at the caller's top_k
    assert door.calls == [("search_dicts", DOOR_Q, 7) + DOOR_SETTINGS[cls] + (None, None, (4, 7, 0.25, "uniform"), ("sum", 50))]
    door.search(DOOR_Q, 7, rank_model=False, rank_pool=5000)  # rank_pool without rank_model is not looked at
    assert door.calls == [("search_dicts", DOOR_Q, 7) + DOOR_SETTINGS[cls] + (None, None, None, None)]


@pytest.mark.parametrize("cls", MIRRORS)
def test_the_specs_of_a_ranked_call_are_checked_against_the_pool(cls):
    door = _Door(cls)
    out = door.search(DOOR_Q, 2000, rank_model=True, collapse_by="parent")  # top_k above 1 024 with a collapse: the pool is 300
    assert door.calls == [("search_dicts", DOOR_Q, 300) + DOOR_SETTINGS[cls] + (None, ("parent", 1, "own", None), None, None),
                          ("rerank_model_results", {"a": 300, "b": 300, "c": 300}, 2000, None, "replace", door.name)]
    assert len(out["a"]) == 300


@pytest.mark.parametrize("cls", MIRRORS)
def test_which_refusal_wins_at_the_door(cls):
    door, name = _Door(cls), "search_bm25" if cls is sparse_rx.RetrievalService else "search"
    collapse = DOOR_STAGES["collapse"]
    assert _message(door.search, DOOR_Q, 7, rank_model=True, boost=BOOST, collapse_by="nope") == (
        f"{name}: rank_model= and boost= do not combine in one call (chain boost_results() over the reranked result)")
    assert _message(door.search, DOOR_Q, 7, rank_model=True, rank_pool=5000, boost=BOOST) == (
        f"{name}: rank_model= and boost= do not combine in one call (chain boost_results() over the reranked result)")
    assert _message(door.search, DOOR_Q, 7, rank_model=True, rank_pool=5000, collapse_by="nope") == "rank_pool must be in [1, 1024], got 5000"
    assert _message(door.search, DOOR_Q, 7, boost=BOOST, **collapse) == (
        f"{name}: boost= and collapse_by= do not combine in one call (chain collapse() over the boosted result)")
    assert _message(door.search, DOOR_Q, 7, boost={"functions": "nope"}, **collapse) != _message(door.search, DOOR_Q, 7, boost=BOOST, **collapse)
    assert _message(door.search, DOOR_Q, 2000, boost=BOOST, **collapse) == f"{name}(collapse_by=...) returns at most 1024 rows per query, got top_k=2000"
    assert _message(door.search, DOOR_Q, 2000, expand_docs=99, **collapse) == f"{name}(collapse_by=...) returns at most 1024 rows per query, got top_k=2000"
    assert _message(door.search, DOOR_Q, 2000, allowed_docs=["nope"], **collapse) == "unknown doc id 'nope' in allowed_docs"
    assert _message(door.search, DOOR_Q, 7, must_terms="alpha", operators=True, allowed_docs=["nope"]) == (
        "must_terms must be a sequence of strings or a dict qid -> sequence, not one string")
    assert _message(door.search, DOOR_Q, 7, expand_docs=99, boost={"functions": "nope"}) == _message(door.be.expand_spec, 99)
    assert not door.calls
    bare = _Door(cls, fields=False, forward=False)  # no fields and no forward index
    assert _message(bare.search, DOOR_Q, 7, expand_docs=4, **collapse) == f"{name}(collapse_by=...) needs the docs' fields: call set_doc_fields() first"
    assert _message(bare.search, DOOR_Q, 7, expand_docs=4, boost=BOOST) == f"{name}(expand_docs=...) needs the forward index: call enable_feedback() first"
    assert _message(bare.search, DOOR_Q, 7, expand_docs=4, where={"must": []}) == f"{name}(where=...) needs the docs' fields: call set_doc_fields() first"
    assert _message(bare.search, DOOR_Q, 7, rank_model=True, expand_docs=4, collapse_by="parent") == (
        f"{name}(collapse_by=...) needs the docs' fields: call set_doc_fields() first")
    bare.be._rank_model = None
    assert _message(bare.search, DOOR_Q, 7, rank_model=True, boost=BOOST) == f"{name}(rank_model=True) needs a model: call set_rank_model() first"
    bare.be.host = None
    assert _message(bare.search, DOOR_Q, 7, rank_model=True, boost=BOOST) == cls.not_built
    assert not bare.calls


def test_top_k_zero_at_both_doors():
    """The service answers {} before it looks at the cache or the index; the registry mirror goes on to search_dicts, whose cache
    may hold the key"""
    warm = (np.array([3, 4], dtype=np.int64), np.array([2.0, 1.0], dtype=np.float32))
    for cls in MIRRORS:
        door = _Door(cls)
        door.obj.query_cache["alpha:0"] = warm
        del door.be.search_dicts  # the real one
        door.be.search_arrays = None  # nothing is searched
        out = door.search({"a": "alpha", "b": "beta"}, 0)
        assert out == ({"a": {}, "b": {}} if cls is sparse_rx.RetrievalService else {"a": {"d3": 2.0, "d4": 1.0}, "b": {}}), cls
        assert door.search({"a": "alpha"}, 0, rank_model=True) == {"a": {}}  # before the pooled pass, at both
        assert door.search({"a": "alpha"}, -3, collapse_by="parent") == {"a": {}}
        assert _message(door.search, {"a": "alpha"}, 0, collapse_by="nope") == "unknown field 'nope'"  # the specs come first


def test_the_service_uploads_again_when_k1_or_b_changed():
    door = _Door(sparse_rx.RetrievalService)
    svc, seen = door.obj, []
    svc._upload = lambda: (seen.append("upload"), setattr(svc, "_built_k1b", (svc.k1, svc.b)))[0]
    door.be.enable_feedback = lambda mode="bm25": seen.append(("enable_feedback", mode))
    svc.k1 = 0.9
    door.search(DOOR_Q, 7, expand_docs=4)
    assert seen == ["upload", ("enable_feedback", "bm25")] and [c[0] for c in door.calls] == ["search_dicts"]
    svc.b = 0.5
    door.search(DOOR_Q, 7)
    assert seen == ["upload", ("enable_feedback", "bm25"), "upload"]
    door.search(DOOR_Q, 0)  # top_k <= 0 returns before the upload
    svc.b = 0.6
    assert door.search(DOOR_Q, 0) == {"a": {}, "b": {}, "c": {}} and len(seen) == 3
    svc.k1 = 1.0
    door.search(DOOR_Q, 7, rank_model=True, expand_docs=4)  # the pooled pass uploads, once
    assert seen[3:] == ["upload", ("enable_feedback", "bm25")] and [c[0] for c in door.calls] == ["search_dicts", "rerank_model_results"]


# ---- the list doors ---------------------------------------------------------------------------------------------------------------
class _Lists:
    """A backend over a 300-doc host index whose field table and BoostFn are CPU fakes: every door reverses the list it is given
    (and doubles a new score), so the result shows the positions and the scores that came back"""

    def __init__(self, monkeypatch):
        be = self.be = SparseBackend("cpu", 14)
        be.build({f"d{i}": {"text": f"alpha beta w{i}"} for i in range(300)}, idf_kind="bm25")
        be.set_fields({"parent": [i // 4 for i in range(300)], "price": np.linspace(0.0, 50.0, 300, dtype=np.float32)})
        be.set_rank_model(_model(), ["score", ("extra", 1)])
        self.launches = launches = []

        def reverse(doc, score, count, k):
            assert doc.dtype == torch.int32 and score.dtype == torch.float32 and count.dtype == torch.int32
            nq = doc.shape[0]
            pos, ns, cnt = torch.zeros((nq, k), dtype=torch.int32), torch.zeros((nq, k)), torch.zeros(nq, dtype=torch.int32)
            for q in range(nq):
                n = min(k, int(count[q]))
                for j in range(n):
                    pos[q, j] = int(count[q]) - 1 - j
                    ns[q, j] = 2.0 * float(score[q, int(count[q]) - 1 - j])
                cnt[q] = n
            return pos, ns, cnt

        class Table:
            device, columns = "cpu", be._fields

            def rank_model_device(self, model, features, doc, score, count, k, extra=None, mode="replace", want_pos=False, named_extra=()):
                launches.append(("rank", tuple(doc.shape), k, None if extra is None else extra.nan_to_num(nan=-1.0).tolist(), mode, want_pos))
                pos, ns, cnt = reverse(doc, score, count, k)
                return None, ns, cnt, pos

            def sort_lists_device(self, by, doc, score, count, k, order, nulls, want_pos=False):
                launches.append(("sort", by, tuple(doc.shape), k, order, nulls, want_pos))
                pos, _, cnt = reverse(doc, score, count, k)
                return None, None, None, torch.stack([cnt, cnt, cnt], dim=1), pos

        class Boost:
            def __init__(self, table, resolved):
                pass

            def __call__(self, doc, score, count, k, carry=None, want_pos=False):
                launches.append(("boost", tuple(doc.shape), k, carry, want_pos))
                pos, ns, cnt = reverse(doc, score, count, k)
                return None, ns, cnt, pos

        table = Table()
        be.field_table = lambda: table
        monkeypatch.setattr(sparse_rx.boost, "BoostFn", Boost)
        self.doors = {"boost_results": lambda results, top_k=None, **kw: be.boost_results(results, kw.pop("boost", BOOST), top_k, **kw),
                      "rerank_model": lambda results, top_k=None, **kw: be.rerank_model_results(results, top_k, **kw),
                      "sort_results": lambda results, top_k=None, **kw: be.sort_results(results, kw.pop("by", "price"), top_k=top_k, **kw)}


@pytest.fixture
def lists(monkeypatch):
    return _Lists(monkeypatch)


LIST_DOORS = {"boost_results": ("boost_results", _capi.SRX_BOOST_MAX_M, True), "rerank_model": ("rerank_model", _capi.SRX_LTR_MAX_M, True),
              "sort_results": ("sort_results", _capi.SRX_ORDER_MAX_M, False)}  # (call, cap, the scores returned are new)
RESULTS = {"a": {"d5": 3.0, "d9": 2.0, "d7": 1.0}, "b": {}, "c": {"d1": 0.5}}


@pytest.mark.parametrize("name", sorted(LIST_DOORS))
def test_list_door(lists, name):
    door, launches = lists.doors[name], lists.launches
    call, cap, new = LIST_DOORS[name]
    f = 2.0 if new else 1.0
    assert door({}) == {} and door(None) == {} and door({"a": {}, "b": []}) == {"a": {}, "b": {}} and not launches
    assert door(RESULTS) == {"a": {"d7": 1.0 * f, "d9": 2.0 * f, "d5": 3.0 * f}, "b": {}, "c": {"d1": 0.5 * f}}
    assert list(door(RESULTS)["a"]) == ["d7", "d9", "d5"]
    assert door(RESULTS, 1) == {"a": {"d7": 1.0 * f}, "b": {}, "c": {"d1": 0.5 * f}}
    assert door(RESULTS, 2) == {"a": {"d7": 1.0 * f, "d9": 2.0 * f}, "b": {}, "c": {"d1": 0.5 * f}}
    assert door(RESULTS, 50) == door(RESULTS)  # above the list length: k = m
    assert [launch[-1] for launch in launches] == [True] * 6 and len({launch[0] for launch in launches}) == 1  # one launch per call
    shape_and_k = [(launch[2], launch[3]) if name == "sort_results" else (launch[1], launch[2]) for launch in launches]
    assert shape_and_k == [((2, 3), 3), ((2, 3), 3), ((2, 3), 1), ((2, 3), 2), ((2, 3), 3), ((2, 3), 3)]
    as_rows = {"a": [{"doc_id": d, "score": s} for d, s in RESULTS["a"].items()], "b": [], "c": RESULTS["c"]}
    assert door(as_rows) == door(RESULTS)  # a search_by_vector row and a dict row
    deep = {"a": {f"d{i % 300}" if i < 300 else f"x{i}": 1.0 for i in range(cap + 1)}}
    assert _message(door, deep) == f"{call} takes lists of at most {cap} docs, got {cap + 1} (no silent truncation)"  # before the unknown id
    assert _message(door, {"a": {"d1": 1.0, "nope": 0.5}}) == "unknown doc id 'nope' among the candidates of 'a'"
    assert _message(door, {"a": {"nope": 0.5}}, 0) == "top_k must be >= 1, got 0"  # top_k before the lists
    assert _message(door, {}, 0) == "top_k must be >= 1, got 0"
    assert _message(door, None, -1) == "top_k must be >= 1, got -1"


def test_list_doors_own_checks_come_first(lists):
    be = lists.be
    assert _message(be.rerank_model_results, RESULTS, 0, mode="nope") == "mode must be one of ['replace', 'sum'], got 'nope'"
    assert _message(be.sort_results, RESULTS, "nope", top_k=0) == "unknown field 'nope'"
    assert _message(be.boost_results, RESULTS, None, 0) == "boost_results needs a boost"
    assert _message(be.boost_results, RESULTS, {"functions": "nope"}, 0) != "top_k must be >= 1, got 0"
    assert _message(be.boost_results, RESULTS, BOOST, 0, call="x") == "top_k must be >= 1, got 0"
    be._rank_model = None
    assert _message(be.rerank_model_results, RESULTS, 0, mode="nope") == "rerank_model(rank_model=True) needs a model: call set_rank_model() first"
    be._fields = None
    assert _message(be.sort_results, RESULTS, "price", top_k=0) == "sort_results(...) needs the docs' fields: call set_doc_fields() first"
    assert _message(be.boost_results, RESULTS, BOOST, 0) == "boost_results(boost=...) needs the docs' fields: call set_doc_fields() first"
    assert not lists.launches


def test_rerank_model_builds_its_extra_plane(lists):
    out = lists.be.rerank_model_results(RESULTS, 2, extra={"a": {"d9": [7.0, 8.0, 9.0], "d7": [4.0]}, "zzz": {"d1": [1.0]}}, mode="sum")
    assert out == {"a": {"d7": 2.0, "d9": 4.0}, "b": {}, "c": {"d1": 1.0}}
    # [live query, list position, extra slot]: missing = NaN (shown as -1), values beyond the model's slots are cut
    assert lists.launches == [("rank", (2, 3), 2, [[[-1.0, -1.0], [7.0, 8.0], [4.0, -1.0]], [[-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0]]], "sum", True)]
