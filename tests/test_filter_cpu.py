"""Filtered search without a GPU: the fourth header and its symbol table, every refusal of the eight entry points (none
reaches a device), the mask packing, the keyword checks of the API mirrors, and the NumPy restatement
(tests/filter_ref.py) on a hand-written example."""
import ctypes
import os
import re

import numpy as np
import pytest

import filter_ref
import sparse_rx
from sparse_rx import _capi
from sparse_rx.backend import doc_filter_spec
from sparse_rx.filter import DocFilter, filter_words, pack_masks, validate_q_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(12)]  # 16-byte aligned addresses, never dereferenced


def test_fourth_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "sparse_rx_filter.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_capi.FILTER_SYMBOLS) and len(declared) == 8, declared ^ set(_capi.FILTER_SYMBOLS)
    assert '#include "sparse_rx.h"' in hdr
    for other in (_capi.SYMBOLS, _capi.RESCORE_SYMBOLS, _capi.QUANT_SYMBOLS):
        assert not set(_capi.FILTER_SYMBOLS) & set(other)
    assert "filter.hip" in _capi.SOURCES
    assert len(_capi.SYMBOLS) == 35
    L = _capi.lib()
    assert L.srx_version() == 301
    for name, (res, args) in _capi.FILTER_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    assert sparse_rx.DocFilter is DocFilter


@pytest.mark.parametrize("n_docs,words", [(1, 4), (31, 4), (32, 4), (33, 4), (127, 4), (128, 4), (129, 8), (20_011, 628), (2 ** 31 - 2, 67_108_864)])
def test_filter_words(n_docs, words):
    assert _capi.lib().srx_filter_words(n_docs) == words == filter_words(n_docs) == filter_ref.words(n_docs)
    assert words % 4 == 0 and words * 32 >= n_docs > (words - 4) * 32


def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg, (rc, msg)


def test_filter_words_refusals():
    for n in (0, -1, 2 ** 31 - 1, 2 ** 40):
        _refused(_capi.lib().srx_filter_words(n), "n_docs")
        with pytest.raises(ValueError):
            filter_words(n)


def test_builder_refusals():
    L = _capi.lib()
    ok = dict(device=0, bits=P[0], n_filters=2, n_docs=100, value=1, stream=None)
    call = lambda **kw: L.srx_filter_fill(*{**ok, **kw}.values())
    for n in (0, -3, 2 ** 31 - 1):
        _refused(call(n_docs=n), "n_docs")
    _refused(call(bits=None), "null pointer")
    _refused(call(bits=P[0] + 4), "16-byte aligned")
    for nf in (0, -1):
        _refused(call(n_filters=nf), "n_filters")
    for v in (2, -1):
        _refused(call(value=v), "value must be 0 or 1")
    assert b"srx_filter_fill" in L.srx_last_error()

    ok = dict(device=0, row=P[0], n_docs=100, doc_base=0, doc=P[1], n=5, value=1, stream=None)
    call = lambda **kw: L.srx_filter_set_docs(*{**ok, **kw}.values())
    _refused(call(n_docs=0), "n_docs")
    _refused(call(row=None), "null pointer")
    _refused(call(row=P[0] + 8), "16-byte aligned")
    _refused(call(doc_base=-1), "doc_base")
    _refused(call(doc_base=2 ** 31 - 1 - 100), "doc_base")
    _refused(call(value=3), "value must be 0 or 1")
    _refused(call(n=-1), "n < 0")
    _refused(call(doc=None), "null pointer")
    assert call(n=0, doc=None) == 0  # nothing to do: no launch
    assert b"srx_filter_set_docs" in L.srx_last_error()

    ok = dict(device=0, bits=P[0], n_filters=2, n_docs=100, out=P[1], stream=None)
    call = lambda **kw: L.srx_filter_count(*{**ok, **kw}.values())
    _refused(call(n_docs=-1), "n_docs")
    _refused(call(bits=None), "null pointer")
    _refused(call(bits=P[0] + 2), "16-byte aligned")
    _refused(call(n_filters=0), "n_filters")
    _refused(call(out=None), "null pointer")
    assert b"srx_filter_count" in L.srx_last_error()


def _filter(**kw):
    d = dict(bits=P[8], n_filters=1, q_filter=None)
    d.update(kw)
    return ctypes.byref(_capi.DocFilterDesc(**d))


def _index_handle():
    """An index handle over never-dereferenced pointers (srx_index_create needs a visible device, so a box without one has
    no handle: the checks that come before the index is looked at are then the ones tested)."""
    d = _capi.IndexDesc(device=0, val_type=0, n_docs=1000, vocab=50, nnz=4000, n_blocks=2000, doc_base=0, tile_log2=6, n_tiles=16,
                        unit_tiles=1, term_ptr=P[0], post=P[1], tile_skip=P[2], idf=P[3], term_bound=None, post16=P[4])
    h = ctypes.c_void_p()
    return h if _capi.lib().srx_index_create(ctypes.byref(d), ctypes.byref(h)) == 0 else None


@pytest.mark.parametrize("packed", [False, True])
def test_filtered_search_refusals(packed):
    L = _capi.lib()
    f = L.srx_search_filtered_packed if packed else L.srx_search_filtered
    name = b"srx_search_filtered_packed" if packed else b"srx_search_filtered"
    outs = dict(out_packed=P[5]) if packed else dict(out_doc=P[5], out_score=P[6], out_count=P[7])
    ok = dict(ix=None, q_ptr=P[0], q_term=P[1], q_weight=P[2], nq=3, k=10, filter=_filter(), after_doc=None, after_score=None, **outs,
              ws=P[9], ws_bytes=1 << 30, stream=None)
    call = lambda **kw: f(*{**ok, **kw}.values())
    # the filter is checked before anything else
    _refused(call(filter=None), "null filter")
    _refused(call(filter=_filter(bits=None)), "null filter bits")
    _refused(call(filter=_filter(bits=P[8] + 4)), "16-byte aligned")
    for nf in (0, -2):
        _refused(call(filter=_filter(n_filters=nf)), "n_filters")
    assert name in L.srx_last_error()
    _refused(call(), "null index")  # the plain search's refusals follow
    h = _index_handle()
    if h is None:
        return
    try:
        call = lambda **kw: f(*{**ok, "ix": h, **kw}.values())
        _refused(call(after_doc=P[10]), "go together")
        _refused(call(after_score=P[10]), "go together")
        for k in (0, 1025):
            assert call(k=k) == -1
        _refused(call(nq=-1), "nq >= 0")
        _refused(call(q_ptr=None), "null query / output pointer")
        for o in outs:
            assert call(**{o: None}) == -1
        assert call(ws=None) == -3 and call(ws_bytes=16) == -3  # SRX_ERR_NOMEM
        assert call(nq=0, q_ptr=None) == 0  # nothing to do: no launch
    finally:
        L.srx_index_destroy(h)


@pytest.mark.parametrize("u8", [False, True])
def test_filtered_dense_refusals(u8):
    L = _capi.lib()
    if u8:
        f, who = L.srx_dense_search_u8_filtered, b"srx_dense_search_u8_filtered"
        ok = dict(device=0, corpus=P[0], scales=P[1], n_docs=1000, dim=64, queries=P[2], nq=2, k=10, doc_base=0, filter=_filter(), out_doc=P[3],
                  out_score=P[4], out_count=P[5], ws=P[6], ws_bytes=1 << 30, stream=None)
    else:
        f, who = L.srx_dense_search_f32_filtered, b"srx_dense_search_f32_filtered"
        ok = dict(device=0, corpus=P[0], n_docs=1000, dim=64, queries=P[2], nq=2, k=10, doc_base=0, filter=_filter(), out_doc=P[3],
                  out_score=P[4], out_count=P[5], ws=P[6], ws_bytes=1 << 30, stream=None, offset=0.0)
    call = lambda **kw: f(*{**ok, **kw}.values())
    _refused(call(filter=None), "null filter")
    _refused(call(filter=_filter(bits=None)), "null filter bits")
    _refused(call(filter=_filter(bits=P[8] + 8)), "16-byte aligned")
    _refused(call(filter=_filter(n_filters=0)), "n_filters")
    for kw in (dict(nq=-1), dict(n_docs=0), dict(k=0), dict(k=1025)):
        _refused(call(**kw), "need n_docs > 0")
    for dim in (0, 32, 1088):
        _refused(call(dim=dim), "multiple of 64")
    _refused(call(doc_base=-1), "doc_base")
    for null in ("corpus", "queries", "out_doc", "out_score", "out_count") + (("scales",) if u8 else ()):
        _refused(call(**{null: None}), "null pointer")
    assert call(ws=None) == -3 and call(ws_bytes=64) == -3  # SRX_ERR_NOMEM
    assert who in L.srx_last_error()
    assert call(nq=0, queries=None) == 0  # nothing to do: no launch


# ---- packing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 129, 20_011])
def test_from_masks_packing(n_docs):
    rng = np.random.default_rng(n_docs)
    masks = rng.random((3, n_docs)) < 0.4
    masks[1] = True
    masks[2] = False
    got = pack_masks(masks)
    assert got.dtype == np.uint32 and got.shape == (3, filter_ref.words(n_docs))
    for r in range(3):
        assert np.array_equal(got[r], filter_ref.pack(masks[r]))
        assert np.array_equal(filter_ref.unpack(got[r], n_docs), masks[r])
    assert np.array_equal(pack_masks(masks[0])[0], got[0])  # one mask = one row
    f = DocFilter.from_masks(masks, device="cpu", doc_base=7)  # the tensor a device would hold (a CPU filter cannot be searched)
    assert (f.n_filters, f.n_docs, f.doc_base, f.words) == (3, n_docs, 7, filter_ref.words(n_docs))
    assert np.array_equal(f.bits.numpy().view(np.uint32), got)
    assert filter_ref.popcount(got[1], n_docs) == n_docs and not got[2].any()
    tail = got[1][n_docs // 32:] if n_docs % 32 else got[1][n_docs // 32:]
    assert int(tail[0]) == (1 << (n_docs % 32)) - 1 if n_docs % 32 else not tail.any()  # tail bits of the last word are 0
    with pytest.raises(ValueError):
        pack_masks(masks.astype(np.int32))
    with pytest.raises(ValueError):
        pack_masks(np.zeros((2, 0), bool))


def test_q_filter_validation():
    assert validate_q_filter(None, 3, 2) is None
    assert validate_q_filter([-1, 0, 1], 3, 2).dtype == np.int32
    for bad in ([0, 1], [0, 1, 2], [-2, 0, 0], [0.0, 1.0, 0.0], [[0, 1, 0]]):
        with pytest.raises(ValueError):
            validate_q_filter(bad, 3, 2)


# ---- keyword checks of the API mirrors ---------------------------------------------------------------------------------------
def test_doc_filter_keywords():
    row_of = {f"d{i}": i for i in range(10)}
    queries = {"a": "x", "b": "y", "c": "z"}
    assert doc_filter_spec(row_of, queries, None, None) is None
    with pytest.raises(ValueError, match="not both"):
        doc_filter_spec(row_of, queries, ["d1"], ["d2"])
    with pytest.raises(ValueError, match="unknown doc id 'nope'"):
        doc_filter_spec(row_of, queries, None, ["d1", "nope"])
    with pytest.raises(ValueError, match="unknown doc id"):
        doc_filter_spec(row_of, queries, {"b": ["d1", "d77"]}, None)
    with pytest.raises(ValueError, match="one string"):
        doc_filter_spec(row_of, queries, "d1", None)
    s = doc_filter_spec(row_of, queries, ["d3", "d1", "d3"], None)
    assert s.allow and [r.tolist() for r in s.lists] == [[3, 1, 3]] and s.row_of_qid == {"a": 0, "b": 0, "c": 0}
    s = doc_filter_spec(row_of, queries, None, {"c": ["d9"], "a": [], "other": ["d0"]})
    assert not s.allow and [r.tolist() for r in s.lists] == [[], [9]] and s.row_of_qid == {"a": 0, "b": -1, "c": 1}
    s = doc_filter_spec(row_of, queries, {"other": ["d0"]}, None)  # no qid of the call is filtered: one unused empty row
    assert len(s.lists) == 1 and set(s.row_of_qid.values()) == {-1}


def test_service_keyword_checks_need_no_gpu(golden_dir):
    """Both keywords, and an unknown doc id, are refused before anything is searched (the index here is host-only)."""
    import json
    from sparse_rx.index import build_host_index
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    svc = sparse_rx.RetrievalService(device="cuda:0")
    svc._be.set_host(build_host_index(j["corpus"]))
    with pytest.raises(ValueError, match="not both"):
        svc.search_bm25(j["queries"], allowed_docs=["doc0"], excluded_docs=["doc1"])
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.search_bm25(j["queries"], excluded_docs={"q0": ["doc0", "missing"]})
    r = sparse_rx.OptimizedBM25Retriever(device="cuda:0")
    r._be.set_host(build_host_index(j["corpus"]))
    with pytest.raises(ValueError, match="not both"):
        r.search(j["queries"], allowed_docs=["doc0"], excluded_docs=["doc1"])
    with pytest.raises(ValueError, match="unknown doc id"):
        r.search(j["queries"], allowed_docs=["doc0", "missing"])


# ---- the restatement on a hand-written example -----------------------------------------------------------------------------------
def test_restatement_by_hand():
    n, base = 40, 100
    mask = np.zeros(n, bool)
    mask[[0, 5, 31, 32, 39]] = True
    row = filter_ref.pack(mask)
    assert row.tolist() == [(1 << 0) | (1 << 5) | (1 << 31), (1 << 0) | (1 << 7), 0, 0]  # 40 docs: 2 words, padded to 4
    assert filter_ref.popcount(row, n) == 5 and np.array_equal(filter_ref.unpack(row, n), mask)
    # two queries, the unfiltered ranking at unlimited depth (GLOBAL ids = base + local row), padded with -1 / 0
    full_doc = np.array([[139, 101, 105, 132, 120, 100, -1], [110, 111, 112, -1, -1, -1, -1]], np.int32)
    full_score = np.array([[9, 8, 7, 7, 3, 1, 0], [5, 4, 3, 0, 0, 0, 0]], np.float32)
    full_count = np.array([6, 3], np.int32)
    d, s, c = filter_ref.filtered_rows(full_doc, full_score, full_count, mask, base, 3)
    assert c.tolist() == [3, 0]
    assert d.tolist() == [[139, 105, 132], [-1, -1, -1]] and s.tolist() == [[9, 7, 7], [0, 0, 0]]
    d, s, c = filter_ref.filtered_rows(full_doc, full_score, full_count, mask, base, 5)
    assert c.tolist() == [4, 0] and d[0].tolist() == [139, 105, 132, 100, -1] and s[0].tolist() == [9, 7, 7, 1, 0]
    # per-query masks: None = that query is not filtered
    d, s, c = filter_ref.filtered_rows(full_doc, full_score, full_count, [mask, None], base, 2)
    assert c.tolist() == [2, 2] and d.tolist() == [[139, 105], [110, 111]]
    d, s, c = filter_ref.filtered_rows(full_doc, full_score, full_count, np.zeros(n, bool), base, 4)
    assert c.tolist() == [0, 0] and (d == -1).all() and not s.any()
