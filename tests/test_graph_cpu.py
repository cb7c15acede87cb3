"""The graph dense index without a GPU: the twenty-second header against its symbol table, one refusal per stated reason (none
reaches a device), the service's refusals, and graph_ref.search on a 6-node graph whose walk is written out by hand."""
import ctypes

import numpy as np
import pytest

import graph_ref as ref
import sparse_rx
from sparse_rx import _capi, graph
from test_dense_scale_cpu import _ctype_class, _prototypes

P = [(i + 1) << 20 for i in range(8)]  # aligned addresses, never dereferenced


def test_table_agrees_with_the_header():
    protos = _prototypes("graph/sparse_rx_graph.h")
    assert set(protos) == set(_capi.GRAPH_SYMBOLS) and len(protos) == 3
    for name, (res, args) in _capi.GRAPH_SYMBOLS.items():
        assert (_ctype_class(res), [_ctype_class(a) for a in args]) == protos[name], name
        f = getattr(_capi.lib(), name)
        assert f.restype is res and list(f.argtypes) == args
    assert "dense_graph.hip" in _capi.SOURCES and any(p.endswith("sparse_rx_graph.h") for p in _capi._deps())
    assert sparse_rx.GraphHalfIndex is graph.GraphHalfIndex and "GraphHalfIndex" in sparse_rx.__all__
    assert ctypes.sizeof(_capi.GraphDesc) == 48
    assert graph.default_max_iter(64, 4, 32) == 63 and graph.default_max_iter(512, 8, 64) == 15 and graph.default_max_iter(32, 1, 16) == 64


def _search(L, desc=..., queries=P[2], nq=3, itopk=64, width=4, max_iter=10, seed_doc=None, n_seed=32, k=10, filter=None, out_doc=P[3], **kw):
    d = dict(device=0, type=0, n_docs=1000, doc_base=0, dim_pad=128, degree=32, corpus=P[0], graph=P[1])
    d.update(kw)
    return L.srx_graph_search(ctypes.byref(_capi.GraphDesc(**d)) if desc is ... else desc, queries, nq, itopk, width, max_iter, seed_doc, n_seed, k, filter,
                              out_doc, P[4], P[5], None, None, 0.0)


def _prune(L, knn=P[0], n=100, d0=64, degree=32, out=P[1]):
    return L.srx_graph_prune(0, knn, n, d0, degree, out, None)


def _merge(L, fwd=P[0], n=100, degree=32, rev_ptr=P[1], rev_src=P[2], out=P[3]):
    return L.srx_graph_merge(0, fwd, n, degree, rev_ptr, rev_src, out, None)


# (call, changed arguments, a phrase only the refusing check's message has)
REFUSALS = [(_search, {"desc": None}, "null desc"), (_search, {"type": 2}, "type must"), (_search, {"dim_pad": 96}, "dim_pad must"),
            (_search, {"dim_pad": 1088}, "dim_pad must"), (_search, {"degree": 8}, "degree must"), (_search, {"degree": 48}, "degree must"),
            (_search, {"n_docs": 0}, "n_docs out of range"), (_search, {"n_docs": 2 ** 31 - 1}, "n_docs out of range"),
            (_search, {"doc_base": -1}, "doc_base + n_docs"), (_search, {"doc_base": 2 ** 31 - 1001}, "doc_base + n_docs"), (_search, {"nq": -1}, "nq < 0"),
            (_search, {"itopk": 0}, "itopk must"), (_search, {"itopk": 48}, "itopk must"), (_search, {"itopk": 544}, "itopk must"),
            (_search, {"width": 0}, "<= width <="), (_search, {"width": 9}, "<= width <="),
            (_search, {"max_iter": 0}, "<= max_iter <="), (_search, {"max_iter": 1025}, "<= max_iter <="), (_search, {"n_seed": 0}, "<= n_seed <="),
            (_search, {"n_seed": 513}, "<= n_seed <="), (_search, {"k": 0}, "<= k <="), (_search, {"k": 65}, "<= k <="),
            (_search, {"max_iter": 64}, "visit budget"), (_search, {"max_iter": 63, "n_seed": 129}, "visit budget"),
            (_search, {"corpus": None}, "desc holds"), (_search, {"graph": None}, "desc holds"), (_search, {"queries": None}, "null queries"),
            (_search, {"out_doc": None}, "null output"), (_search, {"corpus": P[0] + 8}, "corpus must be 16"), (_search, {"queries": P[2] + 4}, "queries must be 16"),
            (_search, {"graph": P[1] + 2}, "4-byte"), (_search, {"seed_doc": P[6] + 1}, "4-byte"),
            (_search, {"filter": ctypes.byref(_capi.DocFilterDesc(bits=None, n_filters=1, q_filter=None))}, "null filter bits"),
            (_search, {"filter": ctypes.byref(_capi.DocFilterDesc(bits=P[6], n_filters=0, q_filter=None))}, "n_filters must"),
            (_prune, {"n": -1}, "n out of range"), (_prune, {"n": 2 ** 31 - 1}, "n out of range"), (_prune, {"degree": 24}, "degree must"),
            (_prune, {"d0": 31}, "<= d0 <="), (_prune, {"d0": 129}, "<= d0 <="), (_prune, {"knn": None}, "null pointer"), (_prune, {"out": None}, "null pointer"),
            (_prune, {"knn": P[0] + 2}, "4-byte"), (_merge, {"n": -1}, "n out of range"), (_merge, {"degree": 0}, "degree must"), (_merge, {"fwd": None}, "null pointer"),
            (_merge, {"rev_ptr": None}, "null pointer"), (_merge, {"rev_src": None}, "null pointer"), (_merge, {"out": None}, "null pointer"),
            (_merge, {"rev_ptr": P[1] + 4}, "8-byte"), (_merge, {"out": P[3] + 1}, "4-byte")]


@pytest.mark.parametrize("call,kw,word", REFUSALS, ids=[f"{c.__name__}-{'-'.join(k)}-{i}" for i, (c, k, _) in enumerate(REFUSALS)])
def test_refusals_fire_before_a_device_is_touched(call, kw, word):
    L = _capi.lib()
    assert call(L, **kw) == -1
    msg = L.srx_last_error().decode()
    assert msg.startswith(call.__name__.replace("_", "srx_graph_", 1) + ":") and word in msg, msg
    assert _search(L, nq=0, queries=None, corpus=None, graph=None, out_doc=None) == 0  # empty calls launch nothing
    assert _prune(L, n=0, knn=None, out=None) == 0 and _merge(L, n=0, fwd=None, rev_ptr=None, rev_src=None, out=None) == 0


def test_service_refusals():
    svc = sparse_rx.RetrievalService()
    e = np.zeros((4, 8), np.float32)
    for kw, match in [({"storage": "f32"}, "ann='graph' needs storage"), ({"storage": "mxfp8"}, "ann='graph' needs storage"),
                      ({"storage": "pq"}, "ann='graph' is not offered with storage='pq'"), ({"screen": "pq"}, "ann='graph' is not offered with storage='pq'"),
                      ({"screen": "binary"}, "screen='binary' is not offered with ann='graph'"), ({"nlist": 2}, "nlist= / nprobe= are not offered with ann='graph'"),
                      ({"nprobe": 1}, "nlist= / nprobe= are not offered with ann='graph'"), ({"graph_degree": 20}, "degree must be"),
                      ({"itopk": 40}, "itopk must be"), ({"itopk": 1024}, "itopk must be"), ({"search_width": 9}, "search_width must be"),
                      ({"graph_degree": 128}, "degree must be"), ({"ann": "hnsw"}, "ann must be")]:
        with pytest.raises(ValueError, match=match):
            svc.set_embeddings(e, **{"storage": "f16", "ann": "graph", **kw})
    for kw in ({"graph_degree": 32}, {"itopk": 64}, {"search_width": 4, "ann": "ivf", "nlist": 2, "nprobe": 1}):
        with pytest.raises(ValueError, match="need ann='graph'"):
            svc.set_embeddings(e, storage="f16", **kw)
    with pytest.raises(ValueError, match="not offered for token embeddings"):
        svc.set_token_embeddings({}, ann="graph")
    svc._be.sharded = lambda: True
    with pytest.raises(ValueError, match="ann='graph' is not offered with a sharded index"):
        svc.set_embeddings(e, storage="f16", ann="graph")
    assert getattr(svc, "_dense", None) is None
    svc.close()


def test_reference_walk_by_hand():
    """v = 1 5 3 6 2 4 for docs 0 .. 5, a beam of 2, one parent per step, the walk starts at doc 0 (global id 10):
    seeds        visited {0}           beam 0
    step 1       0 -> 1, 2             beam 1 2      (0 falls off)
    step 2       1 -> 3 (0 visited)    beam 3 1      (2 falls off unexpanded: 4 is never reached)
    step 3       3 -> 5 (1 visited)    beam 3 1      (5 scored, too low)
    step 4       nothing unexpanded: stop after 3 steps, 5 docs scored."""
    V = np.array([[1, 5, 3, 6, 2, 4]], np.float32)
    g = np.array([[1, 2], [3, 0], [4, -1], [5, 1], [2, 2], [9, 5]], np.int32)
    seeds = np.array([[10, 10, 3, -1]], np.int32)  # a repeat, a local id that is outside once doc_base is taken off, the padding
    d, s, c, st = ref.search(V, g, 2, 1, 10, 2, seeds=seeds, doc_base=10)
    assert d.tolist() == [[13, 11]] and s.tolist() == [[6.0, 5.0]] and c.tolist() == [2] and st.tolist() == [[3, 5]]
    d, s, c, st = ref.search(V, g, 2, 1, 2, 2, seeds=seeds, doc_base=10, allowed=np.array([[1, 1, 1, 0, 1, 1]], bool))
    assert d.tolist() == [[11, -1]] and s.tolist() == [[5.0, 0.0]] and c.tolist() == [1] and st.tolist() == [[2, 4]]
    d, s, c, st = ref.search(V, g, 2, 1, 10, 2, n_seed=3, score_offset=-4.5)  # spread seeds 0, 2, 4; only 5 and 6 stay positive
    # seeds 0 2 4 -> beam 2 4; 2 -> (4 visited); 4 -> (2 visited): stop after 2 steps, 3 docs scored, nothing above 0
    assert c.tolist() == [0] and d.tolist() == [[-1, -1]] and st.tolist() == [[2, 3]]
    assert ref.prune(np.array([[1, 2, 1, 0], [2, 0, 5, 2], [0, 1, 1, 1]], np.int32), 2).tolist() == [[1, 2], [2, 0], [0, 1]]
    # row 0: valid 1 (j 0), 2 (j 1); 2 is reached through 1 only at r = 0 < 1: knn[1][0] == 2 -> one detour; order (0, j0), (1, j1)
    assert ref.merge(np.array([[1, 2], [2, -1], [0, 0]], np.int32)).tolist() == [[1, 2], [2, 0], [0, 1]]
    # node 0: fwd[:1] = 1, rev = [2] (position 0 of source 2; the repeat at position 1 is cut by rev[:1]), fwd[1:] = 2 -> 1 2
