"""Order by a field without a GPU: the thirteenth header and its symbol table, the workspace formula against its restatement,
every refusal of both entry points (none reaches a device), the restatement (tests/order_ref.py) on six docs worked by hand,
the doors over a stub table (decoding, paging, every ValueError) and ``facets`` unchanged by the helper it now shares."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import facets_ref
import order_ref
import sparse_rx
from order_ref import ASC, DESC, F32, I32, I64, NULLS_DROP, NULLS_FIRST, NULLS_LAST
from sparse_rx import _capi, fields
from sparse_rx.backend import SparseBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(16)]  # 16-byte aligned addresses, never dereferenced
I32_MAX = 2 ** 31 - 1


def test_thirteenth_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "order", "sparse_rx_order.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr.split("#ifndef SPARSE_RX_ORDER_H")[1]))
    assert declared == set(_capi.ORDER_SYMBOLS) == {"srx_order_workspace_bytes", "srx_order_topk", "srx_order_lists"}
    assert '#include "sparse_rx_fields.h"' in hdr
    others = (_capi.SYMBOLS, _capi.RESCORE_SYMBOLS, _capi.QUANT_SYMBOLS, _capi.FILTER_SYMBOLS, _capi.HALF_SYMBOLS, _capi.MMR_SYMBOLS,
              _capi.TERMS_SYMBOLS, _capi.MAXSIM_SYMBOLS, _capi.FIELDS_SYMBOLS, _capi.COLLAPSE_SYMBOLS, _capi.FACET_SYMBOLS, _capi.FEEDBACK_SYMBOLS)
    assert [len(t) for t in others] == [35, 4, 4, 8, 5, 3, 2, 3, 1, 1, 2, 2]
    for other in others:
        assert not set(_capi.ORDER_SYMBOLS) & set(other)
    assert sum(len(t) for t in others) + len(_capi.ORDER_SYMBOLS) == 73
    assert os.listdir(os.path.join(ROOT, "include", "order")) == ["sparse_rx_order.h"]
    assert "order.hip" in _capi.SOURCES and os.path.join(_capi.INCLUDE_DIR, "order", "sparse_rx_order.h") in _capi._deps()
    assert "include/order/sparse_rx_order.h" in open(os.path.join(ROOT, "__graft_entry__.py")).read().split('"""')[1]
    L = _capi.lib()
    assert L.srx_version() == 301
    for name, (res, args) in _capi.ORDER_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    for name, value in (("SRX_ORDER_ASC", 0), ("SRX_ORDER_DESC", 1), ("SRX_ORDER_NULLS_LAST", 0), ("SRX_ORDER_NULLS_FIRST", 1), ("SRX_ORDER_NULLS_DROP", 2)):
        assert re.search(rf"\b{name} = {value}\b", hdr) and getattr(_capi, name) == value == getattr(order_ref, name.split("_", 2)[2])
    assert re.search(r"#define SRX_ORDER_MAX_M 2048\b", hdr) and _capi.SRX_ORDER_MAX_M == 2048 == order_ref.MAX_M
    assert _capi.SRX_MAX_K == order_ref.MAX_K == 1024
    assert (order_ref.I32, order_ref.I64, order_ref.F32, order_ref.SET64) == (_capi.SRX_FIELD_I32, _capi.SRX_FIELD_I64, _capi.SRX_FIELD_F32,
                                                                             _capi.SRX_FIELD_SET64)
    assert (order_ref.MIN_SEG, order_ref.CHUNK) == (_capi.SRX_ORDER_MIN_SEG, _capi.SRX_ORDER_CHUNK) == (32768, 8192)
    assert fields.ORDERS == {"asc": 0, "desc": 1} and fields.ORDER_NULLS == {"last": 0, "first": 1, "drop": 2}


def test_order_plan_is_the_c_function():
    L = _capi.lib()
    seg_edges = [32768, 65536, 3 * 32768, 10 * 65536]
    docs = sorted({1, 2, 33, 8192, 2 ** 31 - 2, 10 ** 7} | {e + o for e in seg_edges for o in (-1, 0, 1)})
    for n_docs in docs:
        for n_rows in (0, 1, 2, 1000, 65536):
            for k in (1, 7, 511, 512, 513, 639, 640, 641, 1000, 1023, 1024):
                want = order_ref.plan(n_docs, n_rows, k)
                assert _capi.order_plan(n_docs, n_rows, k) == want and L.srx_order_workspace_bytes(n_docs, n_rows, k) == want[1], (n_docs, n_rows, k)
    # by hand: k <= 512 scans 32 768 docs per segment, k = 1 024 scans 65 536
    assert _capi.order_plan(32768, 1, 10) == (1, 128) and _capi.order_plan(32769, 1, 10) == (2, 256) and _capi.order_plan(200000, 3, 64) == (7, 21 * 776)
    assert _capi.order_plan(65536, 1, 1024) == (1, 12296) and _capi.order_plan(65537, 2, 1024) == (2, 4 * 12296)
    assert _capi.order_plan(2 ** 31 - 2, 1, 1)[0] == 65536
    for bad in ((0, 1, 1), (2 ** 31 - 1, 1, 1), (10, -1, 1), (10, 1, 0), (10, 1, 1025), (10, 2 ** 22, 1024)):
        assert L.srx_order_workspace_bytes(*bad) < 0, bad
    assert L.srx_order_workspace_bytes(10, 2 ** 21 - 1, 1024) > 0


# ---- every refusal of both calls ------------------------------------------------------------------------------------------------
def _refused(rc, word, code=-1):
    msg = _capi.lib().srx_last_error()
    assert rc == code and word.encode() in msg, (rc, msg, word)


def _col(data, valid, typ):
    return ctypes.pointer(_capi.FieldColDesc(data=data, valid=valid, type=typ))


def _flt(bits, n_filters=2, q_filter=None):
    return ctypes.pointer(_capi.DocFilterDesc(bits=bits, n_filters=n_filters, q_filter=q_filter))


def _shared_refusals(call):
    """What both entry points check of the column, the index and the order"""
    _refused(call(col=None), "null col")
    _refused(call(col=_col(P[0], None, 3)), "a SET64 column has no order")
    for typ in (-1, 4, 99):
        _refused(call(col=_col(P[0], None, typ)), "unknown column type")
    for typ in (0, 1, 2):
        _refused(call(col=_col(None, None, typ)), "null data")
    for typ, off in ((0, 2), (0, 1), (2, 2), (1, 4), (1, 2)):
        _refused(call(col=_col(P[0] + off, None, typ)), "aligned for its type")
    for off in (4, 8, 2):
        _refused(call(col=_col(P[0], P[1] + off, 0)), "validity row must be 16-byte aligned")
    for order in (-1, 2, 99):
        _refused(call(order=order), "unknown order")
    for nulls in (-1, 3, 99):
        _refused(call(nulls=nulls), "unknown nulls mode")
    for n in (0, -3, 2 ** 31 - 1, 2 ** 40):
        _refused(call(n_docs=n), "n_docs must be in [1, 2^31 - 2]")
    _refused(call(doc_base=-1), "negative doc_base")
    _refused(call(doc_base=2 ** 31 - 1 - 1000), "doc_base + n_docs must be below 2^31 - 1")
    _refused(call(doc_base=2 ** 40), "doc_base + n_docs must be below 2^31 - 1")


def test_row_form_refusals():
    L = _capi.lib()
    ok = dict(device=0, col=_col(P[0], P[1], 1), n_docs=1000, doc_base=0, order=DESC, nulls=NULLS_LAST, filter=_flt(P[2], 2, P[4]), n_rows=3, k=10,
              after_doc=P[5], out_doc=P[6], out_key=P[7], out_extra=P[8], workspace=P[9], workspace_bytes=3 * 128, stream=None)
    call = lambda **kw: L.srx_order_topk(*{**ok, **kw}.values())
    _shared_refusals(call)
    for k in (0, -1, 1025, I32_MAX):
        _refused(call(k=k), "k must be in [1, 1024]")
    _refused(call(n_rows=-1), "n_rows < 0")
    _refused(call(n_rows=2 ** 22, k=1024), "n_rows * k")
    _refused(call(filter=_flt(None)), "null filter bits")
    for off in (4, 8):
        _refused(call(filter=_flt(P[2] + off)), "filter rows must be 16-byte aligned")
    for n in (0, -1):
        _refused(call(filter=_flt(P[2], n)), "n_filters must be >= 1")
    for name in ("out_doc", "out_key", "out_extra"):
        _refused(call(**{name: None}), "null out_doc / out_key / out_extra")
    _refused(call(workspace=None), "null workspace")
    _refused(call(workspace=P[9] + 4), "workspace must be 8-byte aligned")
    for short in (3 * 128 - 1, 0, -5):
        _refused(call(workspace_bytes=short), "workspace too small", code=-3)
    _refused(call(n_docs=32769), "workspace too small", code=-3)  # two segments
    assert b"srx_order_topk:" in L.srx_last_error()
    # nothing to do: no launch, whatever the pointers are; the checks still come first
    assert call(n_rows=0) == 0
    assert call(n_rows=0, filter=None, after_doc=None, out_doc=None, out_key=None, out_extra=None, workspace=None, workspace_bytes=0) == 0
    assert call(n_rows=0, col=_col(P[0] + 4, None, 2), k=1024, n_docs=2 ** 31 - 2 - 5, doc_base=4) == 0  # natural alignment and the limits pass
    assert call(n_rows=0, col=_col(P[0] + 8, None, 1), k=1, order=ASC, nulls=NULLS_DROP) == 0
    _refused(call(n_rows=0, k=0), "k must be in")
    _refused(call(n_rows=0, filter=_flt(P[2], 0)), "n_filters")
    _refused(call(n_rows=0, doc_base=2 ** 31 - 2 - 1000 + 1), "doc_base + n_docs")


def test_list_form_refusals():
    L = _capi.lib()
    ok = dict(device=0, col=_col(P[0], P[1], 0), n_docs=1000, doc_base=0, order=ASC, nulls=NULLS_FIRST, cand_doc=P[2], cand_score=P[3], cand_count=P[4],
              nq=3, m=100, k=10, out_doc=P[5], out_score=P[6], out_key=P[7], out_pos=P[8], out_extra=P[9], stream=None)
    call = lambda **kw: L.srx_order_lists(*{**ok, **kw}.values())
    _shared_refusals(call)
    for m in (0, -1, 2049, I32_MAX):
        _refused(call(m=m, k=1), "m must be in [1, 2048]")
    for k in (0, -1, 101):
        _refused(call(k=k), "k must be in [1, m]")
    _refused(call(nq=-1), "nq < 0")
    _refused(call(nq=2 ** 21, m=2048), "nq * m")
    for name in ("cand_doc", "cand_score"):
        _refused(call(**{name: None}), "null cand_doc / cand_score")
    for name in ("out_doc", "out_score", "out_key", "out_extra"):
        _refused(call(**{name: None}), "null out_doc / out_score / out_key / out_extra")
    assert b"srx_order_lists:" in L.srx_last_error()
    assert call(nq=0) == 0
    assert call(nq=0, cand_doc=None, cand_score=None, cand_count=None, out_doc=None, out_score=None, out_key=None, out_pos=None, out_extra=None) == 0
    assert call(nq=0, m=2048, k=2048, doc_base=2 ** 31 - 2 - 1000) == 0 and call(nq=0, m=1, k=1) == 0
    _refused(call(nq=0, m=0, k=1), "m must be in")
    _refused(call(nq=0, k=101), "k must be in")


# ---- the restatement on six docs worked by hand -----------------------------------------------------------------------------------
def test_six_docs_by_hand():
    """docs 100 .. 105 hold 5, 3, -, 5, 3, 9 (doc 102 has no value); the set is all six"""
    data, valid = np.array([5, 3, 77, 5, 3, 9], dtype=np.int64), np.array([1, 1, 0, 1, 1, 1], dtype=bool)
    top = lambda order, nulls, k=6, after=None, **kw: order_ref.order_topk(I64, data, valid, 100, order, nulls, k, after=after, **kw)
    d, key, e = top(ASC, NULLS_LAST)
    assert d.tolist() == [[101, 104, 100, 103, 105, 102]] and key.tolist() == [[3, 3, 5, 5, 9, 0]] and e.tolist() == [[6, 5, 6]]
    d, key, e = top(DESC, NULLS_LAST)  # equal values by ascending doc id in both directions
    assert d.tolist() == [[105, 100, 103, 101, 104, 102]] and key.tolist() == [[9, 5, 5, 3, 3, 0]] and e.tolist() == [[6, 5, 6]]
    d, key, e = top(ASC, NULLS_FIRST)
    assert d.tolist() == [[102, 101, 104, 100, 103, 105]] and key.tolist() == [[0, 3, 3, 5, 5, 9]] and e.tolist() == [[6, 5, 6]]
    d, key, e = top(DESC, NULLS_FIRST, k=3)
    assert d.tolist() == [[102, 105, 100]] and e.tolist() == [[3, 2, 6]]
    d, key, e = top(DESC, NULLS_DROP)
    assert d.tolist() == [[105, 100, 103, 101, 104, -1]] and key.tolist() == [[9, 5, 5, 3, 3, 0]] and e.tolist() == [[5, 5, 6]]  # total counts doc 102
    d, key, e = top(ASC, NULLS_DROP, k=2)
    assert d.tolist() == [[101, 104]] and e.tolist() == [[2, 2, 6]]
    # the cursor: what doc 100 precedes
    assert top(ASC, NULLS_LAST, after=[100])[0].tolist() == [[103, 105, 102, -1, -1, -1]]
    assert top(DESC, NULLS_LAST, after=[100])[0].tolist() == [[103, 101, 104, 102, -1, -1]]
    assert top(DESC, NULLS_FIRST, after=[100])[0].tolist() == [[103, 101, 104, -1, -1, -1]]
    assert top(DESC, NULLS_FIRST, after=[102])[0].tolist() == [[105, 100, 103, 101, 104, -1]]
    assert top(ASC, NULLS_LAST, after=[102])[2].tolist() == [[0, 0, 6]]   # the last doc of the order: nothing follows
    assert top(ASC, NULLS_DROP, after=[102])[2].tolist() == [[0, 0, 6]]   # a valueless cursor under DROP: empty
    assert top(ASC, NULLS_DROP, after=[104])[0].tolist() == [[100, 103, 105, -1, -1, -1]]
    for outside in (99, 106, -2, 5):
        assert top(ASC, NULLS_LAST, after=[outside])[2].tolist() == [[0, 0, 6]]
    assert top(ASC, NULLS_LAST, after=[-1])[0].tolist() == [[101, 104, 100, 103, 105, 102]]
    # rows: mask 0 = the docs 100, 102, 104; a cursor doc outside the row still positions (103 is not in row 0)
    masks = np.array([[1, 0, 1, 0, 1, 0], [0] * 6], dtype=bool)
    d, key, e = top(ASC, NULLS_LAST, k=2, masks=masks, q_filter=[0, 1, -1], n_rows=3, after=[103, -1, 105])
    assert d.tolist() == [[102, -1], [-1, -1], [102, -1]] and e.tolist() == [[1, 0, 3], [0, 0, 0], [1, 0, 6]]
    # pages of 2 chained by the cursor give the complete order
    for nulls, want in ((NULLS_LAST, [105, 100, 103, 101, 104, 102]), (NULLS_FIRST, [102, 105, 100, 103, 101, 104]), (NULLS_DROP, [105, 100, 103, 101, 104])):
        got, after = [], -1
        while True:
            d, _, e = top(DESC, nulls, k=2, after=[after])
            got += d[0, : e[0, 0]].tolist()
            if e[0, 0] < 2:
                break
            after = got[-1]
        assert got == want
    # floats: -0 == +0 (tie by doc), the NaN has no value, the key keeps the stored bits
    f = np.array([0.0, -0.0, np.nan, -np.inf, 1e-45, np.inf], dtype=np.float32)
    d, key, e = order_ref.order_topk(F32, f, None, 0, ASC, NULLS_LAST, 6)
    assert d.tolist() == [[3, 0, 1, 4, 5, 2]] and e.tolist() == [[6, 5, 6]]
    assert key.tolist() == [[0xFF800000, 0, 0x80000000, 1, 0x7F800000, 0]]
    assert order_ref.order_topk(F32, f, None, 0, DESC, NULLS_FIRST, 6)[0].tolist() == [[2, 5, 4, 0, 1, 3]]
    # lists: ties keep list order, a doc twice stays twice, 106 and -1 are not live, the count cuts
    cand = np.array([[104, 100, 102, 106, 101, 100, -1, 105]], dtype=np.int32)
    score = np.array([[8, 7, np.nan, 5, -4, 3, 2, 1]], dtype=np.float32)
    d, s, key, pos, e = order_ref.order_lists(I64, data, valid, 100, ASC, NULLS_LAST, cand, score, None, 8)
    assert d.tolist() == [[104, 101, 100, 100, 105, 102, -1, -1]] and pos.tolist() == [[0, 4, 1, 5, 7, 2, -1, -1]] and e.tolist() == [[6, 5, 6]]
    assert s.tolist() == [[score.view(np.uint32)[0, p] if p >= 0 else 0 for p in pos[0]]] and key.tolist() == [[3, 3, 5, 5, 9, 0, 0, 0]]
    d, s, key, pos, e = order_ref.order_lists(I64, data, valid, 100, DESC, NULLS_DROP, cand, score, [5], 3)
    assert d.tolist() == [[100, 104, 101]] and pos.tolist() == [[1, 0, 4]] and e.tolist() == [[3, 3, 4]]
    d, s, key, pos, e = order_ref.order_lists(I64, data, valid, 100, DESC, NULLS_FIRST, cand, score, [99], 2)
    assert d.tolist() == [[102, 105]] and e.tolist() == [[2, 1, 6]]
    for count in (0, -3):
        assert order_ref.order_lists(I64, data, valid, 100, ASC, NULLS_LAST, cand, score, [count], 2)[4].tolist() == [[0, 0, 0]]


# ---- the doors over a stub table ---------------------------------------------------------------------------------------------------
def _schema():
    n = 8
    price = np.ma.array(np.array([2.5, 1, 1, 7, 0, 3, 3, 9], dtype=np.float32), mask=[0, 0, 0, 0, 1, 0, 0, 0])
    return {"year": np.array([5, 3, 9, 5, 3, 1, 9, 7], dtype=np.int32), "big": (np.arange(n, dtype=np.int64) - 4) * 2 ** 40, "flag": np.arange(n) % 2 == 0,
            "src": ["b", "a", None, "c", "b", "a", "b", "c"], "price": price, "tags": [["x"], ["y", "z"]] * 4}


class _StubTable:
    """top_by_device / sort_lists_device answered by the restatement on CPU tensors; it records its calls"""

    def __init__(self, cols):
        self.cols, self.device, self.calls = cols, torch.device("cpu"), []

    def top_by_device(self, column, k, order="desc", nulls="last", filter=None, q_filter=None, n_rows=None, after=None):
        self.calls.append((column, k, order, nulls, n_rows, None if after is None else after.tolist()))
        c = self.cols[column]
        out = order_ref.order_topk(c.type, c.data, c.valid, 0, fields.ORDERS[order], fields.ORDER_NULLS[nulls], k, n_rows=n_rows,
                                   after=None if after is None else after.numpy())
        return tuple(torch.from_numpy(x) for x in out)

    def sort_lists_device(self, column, doc, score, count, k, order="desc", nulls="last", want_pos=False):
        self.calls.append((column, tuple(doc.shape), k))
        c = self.cols[column]
        d, s, key, pos, extra = order_ref.order_lists(c.type, c.data, c.valid, 0, fields.ORDERS[order], fields.ORDER_NULLS[nulls], doc.numpy(), score.numpy(),
                                                      count.numpy(), k)
        return tuple(torch.from_numpy(x) for x in (d, s.view(np.float32), key, extra, pos))


def _stub_backend():
    be = SparseBackend("cuda:0", 14)
    be._fields = fields.host_columns(_schema())
    table = _StubTable(be._fields)
    be.field_table = lambda: table
    be.host = type("Host", (), {"doc_ids": [f"d{i}" for i in range(8)], "vocabulary": {}, "n_docs": 8})()
    be.dev = object()
    return be, table


def test_search_sorted_over_a_stub_table(monkeypatch):
    be, table = _stub_backend()
    q = {"q0": "anything", "q1": ""}
    got = be.search_sorted(q, "year", match=None, top_k=3)
    assert got == {"q0": {"d2": 9, "d6": 9, "d7": 7}, "q1": {"d2": 9, "d6": 9, "d7": 7}} and list(got["q0"]) == ["d2", "d6", "d7"]
    assert all(type(v) is int for v in got["q0"].values()) and table.calls == [("year", 3, "desc", "last", 1, None)]  # one row for both queries
    got = be.search_sorted(q, "src", order="asc", match=None, top_k=8)["q0"]  # categories order alphabetically; d2 has none
    assert list(got.items()) == [("d1", "a"), ("d5", "a"), ("d0", "b"), ("d4", "b"), ("d6", "b"), ("d3", "c"), ("d7", "c"), ("d2", None)]
    assert list(be.search_sorted(q, "src", order="asc", nulls="first", match=None, top_k=2)["q0"].items()) == [("d2", None), ("d1", "a")]
    assert list(be.search_sorted(q, "src", nulls="drop", match=None, top_k=100)["q0"]) == ["d3", "d7", "d0", "d4", "d6", "d1", "d5"]
    got = be.search_sorted(q, "price", order="asc", match=None, top_k=3)["q0"]
    assert got == {"d1": 1.0, "d2": 1.0, "d0": 2.5} and all(type(v) is float for v in got.values())
    got = be.search_sorted(q, "flag", match=None, top_k=8)["q0"]
    assert list(got.items())[:5] == [("d0", True), ("d2", True), ("d4", True), ("d6", True), ("d1", False)] and type(got["d0"]) is bool
    assert be.search_sorted(q, "big", order="asc", match=None, top_k=2)["q1"] == {"d0": -4 * 2 ** 40, "d1": -3 * 2 ** 40}
    # a text without a token has the empty set under "any" / "all", and nothing is launched for it
    table.calls.clear()
    assert be.search_sorted({"q1": " "}, "year") == {"q1": {}} and be.search_sorted({}, "year") == {} and table.calls == []
    # top_k above the engine's list depth pages with the cursor: the same order, page by page
    monkeypatch.setattr(_capi, "SRX_MAX_K", 3)
    got = be.search_sorted(q, "price", order="asc", nulls="first", match=None, top_k=7)["q0"]
    assert list(got.items()) == [("d4", None), ("d1", 1.0), ("d2", 1.0), ("d0", 2.5), ("d5", 3.0), ("d6", 3.0), ("d3", 7.0)]
    assert [c[1:] for c in table.calls] == [(3, "asc", "first", 1, None), (3, "asc", "first", 1, [2]), (1, "asc", "first", 1, [6])]
    table.calls.clear()
    assert list(be.search_sorted(q, "year", match=None, top_k=100)["q0"]) == ["d2", "d6", "d7", "d0", "d3", "d1", "d4", "d5"]
    assert [c[5] for c in table.calls] == [None, [7], [1]]  # the third page came back short: the set is exhausted


def test_sort_results_over_a_stub_table():
    be, table = _stub_backend()
    res = {"q0": {"d0": 3.0, "d2": 2.5, "d7": 2.0, "d3": 1.0}, "q1": {}, "v": [{"doc_id": "d7", "score": 1.0}, {"doc_id": "d1", "score": 0.5}, {"doc_id": "d7", "score": 0.25}]}
    got = be.sort_results(res, "year")
    assert list(got["q0"].items()) == [("d2", 2.5), ("d7", 2.0), ("d0", 3.0), ("d3", 1.0)] and got["q1"] == {}  # d0 and d3 tie: list order
    assert list(got["v"].items()) == [("d7", 0.25), ("d1", 0.5)]  # a doc listed twice is one dict key; the later entry's score stands
    assert table.calls == [("year", (2, 4), 4)]
    assert list(be.sort_results(res, "src", order="asc", top_k=2)["q0"].items()) == [("d0", 3.0), ("d7", 2.0)]  # d7 and d3 are both "c": list order
    assert list(be.sort_results(res, "src", order="asc", nulls="first", top_k=1)["q0"]) == ["d2"]
    assert list(be.sort_results(res, "src", order="asc", nulls="drop")["q0"]) == ["d0", "d7", "d3"]
    assert be.sort_results({}, "year") == {}
    with pytest.raises(ValueError, match="unknown doc id 'zz'"):
        be.sort_results({"q0": {"zz": 1.0}}, "year")
    deep = {"q0": {f"d{i % 8}_{i}": 1.0 for i in range(2049)}}
    with pytest.raises(ValueError, match="at most 2048 docs, got 2049"):
        be.sort_results(deep, "year")


def test_backend_refusals():
    be, table = _stub_backend()
    q, r = {"q0": "w"}, {"q0": {"d0": 1.0}}
    for door, arg in ((be.search_sorted, q), (be.sort_results, r)):
        with pytest.raises(ValueError, match="unknown field 'nope'"):
            door(arg, "nope")
        with pytest.raises(ValueError, match="'tags' is a set column: a label set has no order"):
            door(arg, "tags")
        for bad in ("up", None, 1, "DESC"):
            with pytest.raises(ValueError, match="order must be one of asc, desc"):
                door(arg, "year", order=bad)
        for bad in ("own", None, 0):
            with pytest.raises(ValueError, match="nulls must be one of last, first, drop"):
                door(arg, "year", nulls=bad)
        with pytest.raises(ValueError, match="top_k must be >= 1"):
            door(arg, "year", top_k=0)
    with pytest.raises(ValueError, match=r"match=\"any\" puts the query's own terms into the any list"):
        be.search_sorted(q, "year", any_terms=["w"])
    with pytest.raises(ValueError, match="match must be"):
        be.search_sorted(q, "year", match="some")
    with pytest.raises(ValueError, match="must_terms must be a sequence"):
        be.search_sorted(q, "year", match="all", must_terms="w")
    with pytest.raises(ValueError, match="match must be"):  # facets checks match before top, as it did before it shared match_rows
        be.facets(q, ["src"], match="some", top=0)
    with pytest.raises(ValueError, match=r"match=\"any\""):
        be.facets(q, ["src"], any_terms=["w"], top=0)
    assert table.calls == []
    be._fields = None
    for door, arg, name in ((be.search_sorted, q, "search_sorted"), (be.sort_results, r, "sort_results")):
        with pytest.raises(ValueError, match=rf"{name}\(\.\.\.\) needs the docs' fields: call set_doc_fields"):
            door(arg, "year")


def test_check_order_args_and_decoding():
    s = fields.host_columns(_schema())
    assert fields.check_order_args(s, "year", "asc", "drop") == (0, 2) and fields.check_order_args(s, "src", "desc", "first") == (1, 1)
    for name in ("year", "big", "flag", "src", "price"):
        assert fields.check_order_args(s, name, "desc", "last") == (1, 0)
    assert fields.decode_order_key(s["price"], np.array([0x80000000, 0x3F800000])).tolist() == [-0.0, 1.0]
    assert np.signbit(fields.decode_order_key(s["price"], np.array([0x80000000]))[0])
    assert fields.decode_order_key(s["year"], np.array([-5, 7])).dtype == np.int32 and fields.decode_order_key(s["big"], np.array([-2 ** 62])).tolist() == [-2 ** 62]
    extra = np.array([[3, 2, 9], [0, 0, 4], [4, 4, 4]])
    assert fields.order_has_value(extra, "last", 4).tolist() == [[1, 1, 0, 0], [0] * 4, [1] * 4]
    assert fields.order_has_value(extra, "first", 4).tolist() == [[0, 1, 1, 0], [0] * 4, [1] * 4]
    assert fields.order_values(s["src"], np.array([2, 0, 0]), np.array([True, True, False])) == ["c", "a", None]


def test_field_table_refusals():
    cols = fields.host_columns(_schema())
    t = fields.FieldTable(cols, {name: (torch.from_numpy(c.data), None) for name, c in cols.items()}, torch.device("cpu"))
    doc, score = torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 4))
    for call in (lambda n: t.top_by_device(n, 3), lambda n: t.top_by(n, 3), lambda n: t.sort_lists_device(n, doc, score, None, 2),
                 lambda n: t.sort_lists(n, doc.numpy(), score.numpy(), None, 2)):
        with pytest.raises(ValueError, match="unknown field 'nope'"):
            call("nope")
        with pytest.raises(ValueError, match="set column"):
            call("tags")
    for k in (0, 1025):
        with pytest.raises(ValueError, match=r"k must be in \[1, 1024\]"):
            t.top_by_device("year", k)
    with pytest.raises(ValueError, match="q_filter picks rows of a filter"):
        t.top_by_device("year", 3, q_filter=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="q_filter picks rows of a filter"):
        t.top_by("year", 3, q_filter=[0, 1])
    with pytest.raises(ValueError, match="filter must be a DocFilter"):
        t.top_by_device("year", 3, filter=object())
    with pytest.raises(ValueError, match=r"after must be an int32 tensor \[n_rows\]"):
        t.top_by_device("year", 3, after=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="after must be a 1-D sequence"):
        t.top_by("year", 3, after=[[1]])
    with pytest.raises(ValueError, match=r"int32 tensor \[nq, m\]"):
        t.sort_lists_device("year", doc.long(), score, None, 2)
    with pytest.raises(ValueError, match="lists of 1 to 2048 positions, got 2049"):
        t.sort_lists_device("year", torch.zeros((1, 2049), dtype=torch.int32), torch.zeros((1, 2049)), None, 2)
    with pytest.raises(ValueError, match="at most 2048 positions, got 2049"):
        t.sort_lists("year", np.zeros((1, 2049), np.int32), np.zeros((1, 2049), np.float32), None, 2)
    with pytest.raises(ValueError, match="score must be a float32 tensor of doc's shape"):
        t.sort_lists_device("year", doc, score[:, :3], None, 2)
    with pytest.raises(ValueError, match=r"count must be an int32 tensor \[nq\]"):
        t.sort_lists_device("year", doc, score, torch.zeros(3, dtype=torch.int32), 2)
    for k in (0, 5):
        with pytest.raises(ValueError, match=r"k must be in \[1, m = 4\]"):
            t.sort_lists_device("year", doc, score, None, k)
    with pytest.raises(ValueError, match="doc is on meta"):
        t.sort_lists_device("year", doc.to("meta"), score, None, 2)
    t.close()
    with pytest.raises(ValueError, match="the table is closed"):
        t.top_by_device("year", 3)
    with pytest.raises(ValueError, match="the table is closed"):
        t.sort_lists_device("year", doc, score, None, 2)


# ---- the mirrors ---------------------------------------------------------------------------------------------------------------
def test_doors_refuse_unbuilt_and_sharded(golden_dir, tmp_path):
    import tempfile
    import torch.distributed as dist
    from test_dict_search_cpu import _Counted
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    q = {qid: j["queries"][qid] for qid in ("q0", "q1")}
    n = len(j["corpus"])
    assert not dist.is_initialized()
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method=f"file://{os.path.join(tmp, 'rendezvous')}", rank=0, world_size=1)
        try:
            for make, method in ((lambda f: sparse_rx.RetrievalService(shard_searcher_factory=f, sharded=True), "search_bm25"),
                                 (lambda f: sparse_rx.OptimizedBM25Retriever(shard_searcher_factory=f, sharded=True), "search"),
                                 (lambda f: sparse_rx.OptimizedRetriever({"type": "bm25"}, shard_searcher_factory=f, sharded=True, cache_dir=str(tmp_path)), "search")):
                f = _Counted()
                o = make(f)
                with pytest.raises(ValueError, match="not built"):
                    o.search_sorted(q, "year")
                with pytest.raises(ValueError, match="not built"):
                    o.sort_results({}, "year")
                (o.build_bm25_index if method == "search_bm25" else o.build_index_from_corpus)(j["corpus"])
                r = getattr(o, method)(q, top_k=5)
                f.take()
                for door, arg, name in ((o.search_sorted, q, "search_sorted"), (o.sort_results, r, "sort_results")):
                    with pytest.raises(ValueError, match=rf"{name}\(\.\.\.\) needs the docs' fields: call set_doc_fields"):
                        door(arg, "year")
                o.set_doc_fields({"year": np.arange(n, dtype=np.int32)})
                for door, arg in ((o.search_sorted, q), (o.sort_results, r)):
                    with pytest.raises(ValueError, match="needs the whole index on one GPU"):
                        door(arg, "year")
                assert f.take() == []  # no search, no launch
                o.close()
        finally:
            dist.destroy_process_group()


def test_doors_and_their_defaults():
    for cls in (sparse_rx.RetrievalService, sparse_rx.OptimizedBM25Retriever, sparse_rx.OptimizedRetriever):
        sig = inspect.signature(cls.search_sorted).parameters
        assert list(sig)[:3] == ["self", "queries", "by"]
        want = dict(order="desc", top_k=10, match="any", nulls="last", allowed_docs=None, excluded_docs=None, must_terms=None, any_terms=None,
                    must_not_terms=None, where=None)
        assert {k: sig[k].default for k in want} == want and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want)
        sig = inspect.signature(cls.sort_results).parameters
        assert list(sig)[:3] == ["self", "results", "by"] and {k: sig[k].default for k in ("order", "nulls", "top_k")} == dict(order="desc", nulls="last", top_k=None)
        assert "corpus order" in cls.search_sorted.__doc__
    assert "corpus order" in SparseBackend.search_sorted.__doc__
    for cls in (sparse_rx.HybridRetriever, sparse_rx.ShardedSearcher, sparse_rx.HostBatchPipeline):
        assert not hasattr(cls, "search_sorted") and not hasattr(cls, "sort_results")
    assert "by" not in inspect.signature(sparse_rx.RetrievalService.search_hybrid).parameters
    for name in ("top_by_device", "top_by", "sort_lists_device", "sort_lists"):
        assert callable(getattr(fields.FieldTable, name))


# ---- facets shares match_rows now: what it returns is what it returned ----------------------------------------------------------
class _FacetStub:
    def __init__(self, cols):
        self.cols, self.device = cols, torch.device("cpu")

    def facet_device(self, column, spec, filter=None, q_filter=None, n_rows=None):
        assert filter is None and q_filter is None
        c = self.cols[column]
        return tuple(torch.from_numpy(x) for x in facets_ref.facet_counts(c.type, c.data, c.valid, spec.mode, spec.n_bins, spec.origin, spec.edges, None, None, n_rows))


def test_facets_on_text_small_is_unchanged(golden_dir):
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    n = len(j["corpus"])
    be = SparseBackend("cuda:0", 6)
    be.build(j["corpus"])
    be.set_fields({"src": [None if i % 13 == 4 else ("wiki", "arxiv", "web", "forum")[(i * 7) % 4 if i % 3 else 0] for i in range(n)],
                   "year": np.array([1990 + (i * 5) % 40 for i in range(n)], dtype=np.int32)})
    table = _FacetStub(be._fields)
    be.field_table = lambda: table
    be.dev = object()
    spec = {"src": None, "year": {"edges": [1990, 2000.5, 2010, 2029]}}
    queries = {"q0": j["queries"]["q0"], "blank": "  "}
    every = {"src": {"counts": {"wiki": 142, "forum": 48, "arxiv": 47, "web": 47}, "missing": 24, "other": 0, "total": 308},  # as the parent returns it
             "year": {"counts": {(2010, 2029): 152, (1990, 2000.5): 117, (2000.5, 2010): 39}, "missing": 0, "other": 0, "total": 308}}
    none = {name: {"counts": {}, "missing": 0, "other": 0, "total": 0} for name in spec}
    got = be.facets(queries, spec, match=None)
    assert got == {"q0": every, "blank": every} and list(got["q0"]["src"]["counts"]) == list(every["src"]["counts"])
    assert be.facets({"blank": "  ", "none": ""}, spec) == {"blank": none, "none": none}
    assert be.facets({"blank": " "}, spec, match="all") == {"blank": none}
    assert be.facets(queries, "src", match=None, top=1) == {q: {"src": {**every["src"], "counts": {"wiki": 142}}} for q in queries}
