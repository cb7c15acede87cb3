"""Late-interaction search without a GPU: the twenty-sixth header and its table, every refusal of the two entry points and of
the Python doors (none reaches a device), the workspace sizes, and tests/late_search_ref.py on matrices small enough to rank by
hand."""
import os
import re

import numpy as np
import pytest

import late_search_ref
import sparse_rx
from sparse_rx import _capi
from sparse_rx.late import TokenIndex, check_late_search, late_search_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(12)]  # 16-byte aligned addresses, never dereferenced


def test_header_and_table():
    assert os.listdir(os.path.join(ROOT, "include", "late")) == ["sparse_rx_maxsim_search.h"]
    body = open(os.path.join(ROOT, "include", "late", "sparse_rx_maxsim_search.h")).read().split("#ifndef SPARSE_RX_MAXSIM_SEARCH_H")[1]
    assert set(re.findall(r"\b(srx_maxsim_[a-z_0-9]+)\s*\(", body)) == set(_capi.MAXSIM_SEARCH_SYMBOLS) and len(_capi.MAXSIM_SEARCH_SYMBOLS) == 2
    assert not set(_capi.MAXSIM_SEARCH_SYMBOLS) & set(_capi.MAXSIM_SYMBOLS)
    deps = [os.path.basename(p) for p in _capi._deps()]
    assert "maxsim_search.hip" in _capi.SOURCES and {"sparse_rx_maxsim_search.h", "maxsim_common.h", "maxsim_search.hip"} <= set(deps)
    assert "include/late/sparse_rx_maxsim_search.h" in _capi.__doc__ and "maxsim_search.hip" not in _capi.UNIT_FLAGS
    L = _capi.lib()
    for name, (res, args) in _capi.MAXSIM_SEARCH_SYMBOLS.items():
        f = getattr(L, name)
        assert f.restype is res and list(f.argtypes) == args, name
    assert len(_capi.MAXSIM_SEARCH_SYMBOLS["srx_maxsim_search_half"][1]) == 20
    for name in ("check_late_search", "late_search_plan"):
        assert name in sparse_rx.__all__
    for cls in (sparse_rx.HybridRetriever, sparse_rx.ShardedSearcher, sparse_rx.HostBatchPipeline):
        assert not hasattr(cls, "search_late")


def test_workspace_bytes():
    ws = _capi.lib().srx_maxsim_search_workspace_bytes
    for args in ((-1, 32, 128, 100, 10), (1, 0, 128, 100, 10), (1, 129, 128, 100, 10), (1, 33, 1024, 100, 10), (1, 32, 96, 100, 10),
                 (1, 32, 128, 0, 10), (1, 32, 128, 2 ** 31 - 1, 10), (1, 32, 128, 100, 0), (1, 32, 128, 100, 1025)):
        assert ws(*args) == -1 and b"srx_maxsim_search_workspace_bytes" in _capi.lib().srx_last_error(), args
    # the group rule, the minimum (packed queries + one group's score rows) and the preferred size, pinned to the library
    for args, qg in (((1, 32, 128, 5000, 10), 1), ((2, 32, 128, 5000, 10), 2), ((3, 32, 128, 5000, 10), 4), ((33, 33, 128, 5000, 10), 2),
                     ((33, 128, 256, 5000, 10), 1), ((33, 32, 1024, 5000, 10), 1), ((33, 32, 512, 5000, 10), 2), ((33, 64, 512, 5000, 10), 1),
                     ((33, 96, 320, 5000, 10), 1), ((1024, 32, 128, 200000, 100), 4), ((2000, 32, 128, 10 ** 7, 1024), 4), ((0, 1, 64, 1, 1), 1)):
        nq, tq, dim_pad, n_docs, k = args
        g, lo, hi = late_search_plan(*args)
        qbytes = nq * ((tq + 31) // 32 * 32) * dim_pad * 2
        assert g == qg and hi == ws(*args) and lo <= hi, args
        assert qbytes + min(nq, qg) * n_docs * 4 <= lo <= qbytes + min(nq, qg) * (n_docs + 63) * 4 + 768, args
    base = (8, 31, 128, 5000, 100)  # monotone in every argument
    for i, more in enumerate((9, 33, 192, 9000, 101)):
        assert ws(*base[:i], more, *base[i + 1:]) >= ws(*base), i


def _call(**kw):
    ok = dict(device=0, type=0, tok=P[0], n_tok=5000, dim_pad=128, tok_ptr=P[1], n_docs=1000, doc_base=0, q_tok=P[2], q_cnt=P[3], nq=2, tq=32,
              k=4, filter=None, out_doc=P[4], out_score=P[5], out_count=P[6], ws=P[7], ws_bytes=1 << 30, stream=None)
    return _capi.lib().srx_maxsim_search_half(*{**ok, **kw}.values())


def test_refusals():
    def refused(word, **kw):
        msg = _capi.lib().srx_last_error()
        assert _call(**kw) == -1 and word.encode() in _capi.lib().srx_last_error() and b"srx_maxsim_search_half" in _capi.lib().srx_last_error(), (kw, msg)
    for t in (-1, 2):
        refused("type must be", type=t)
    for d in (0, 96, 1088):
        refused("multiple of 64", dim_pad=d)
    for tq, dim_pad in ((0, 64), (129, 64), (33, 1024), (65, 512)):
        refused("tq must be", tq=tq, dim_pad=dim_pad)
    for k in (0, -1, 1025):
        refused("k must be", k=k)
    for n in (0, -1, 2 ** 31 - 1):
        refused("n_docs", n_docs=n)
    for n in (-1, 2 ** 31 - 1):
        refused("n_tok", n_tok=n)
    refused("doc_base", doc_base=-1)
    refused("doc_base", doc_base=2 ** 31 - 1000)
    refused("nq < 0", nq=-1)
    for null in ("tok", "tok_ptr", "q_tok", "out_doc", "out_score", "out_count"):
        refused("null pointer", **{null: None})
    refused("16-byte aligned", tok=P[0] + 8)
    refused("16-byte aligned", q_tok=P[2] + 4)
    for bad, word in ((dict(bits=None, n_filters=1), "null filter bits"), (dict(bits=P[8] + 4, n_filters=1), "16-byte aligned"),
                      (dict(bits=P[8], n_filters=0), "n_filters")):
        import ctypes
        refused(word, filter=ctypes.byref(_capi.DocFilterDesc(q_filter=None, **bad)))
    lo = late_search_plan(2, 32, 128, 1000, 4)[1]
    assert _call(ws=None) == -3 and _call(ws_bytes=lo - 1) == -3 and b"workspace" in _capi.lib().srx_last_error()  # SRX_ERR_NOMEM
    # nothing to do: no launch, whatever the pointers
    assert _call(nq=0, tok=None, tok_ptr=None, q_tok=None, q_cnt=None, out_doc=None, out_score=None, out_count=None, ws=None, ws_bytes=0) == 0


def test_python_doors():
    assert check_late_search(32, 1024, 1024) == 1024 and check_late_search(1, 64, 1) == 1
    for k in (0, -1, 1025):
        with pytest.raises(ValueError, match="no silent truncation"):
            check_late_search(32, 128, k)
    with pytest.raises(ValueError, match="query tokens"):
        check_late_search(129, 64, 10)
    with pytest.raises(ValueError, match="exceed the limit"):
        check_late_search(33, 1024, 10)
    assert {"search", "search_device"} <= set(dir(TokenIndex))
    svc = sparse_rx.RetrievalService(device="cpu")
    with pytest.raises(ValueError, match="No token index"):
        svc.search_late({"a": np.ones((2, 4), np.float32)})
    svc._late = type("Fake", (), {"dim": 4, "n_docs": 3})()
    with pytest.raises(ValueError, match="no silent truncation"):
        svc.search_late({"a": np.ones((2, 4), np.float32)}, top_k=1025)
    with pytest.raises(ValueError, match="at most 128"):
        svc.search_late({"a": np.ones((129, 4), np.float32)})
    assert svc.search_late({}) == {} and svc.search_late({"a": np.ones((2, 4), np.float32)}, top_k=0) == {"a": {}}
    svc._late = None


def test_reference_rows_by_hand():
    s = np.array([[1.0, -2.0, 0.0, 1.0, -0.5], [-1.0, -3.0, -2.0, -1.0, -4.0]], np.float32)
    doc, score, count = late_search_ref.expected(s, None, 3, doc_base=10)
    assert doc.tolist() == [[10, 13, 12], [10, 13, 12]] and score.tolist() == [[1.0, 1.0, 0.0], [-1.0, -1.0, -2.0]] and count.tolist() == [3, 3]
    allowed = np.array([[False, True, False, False, True], [False] * 5])
    doc, score, count = late_search_ref.expected(s, allowed, 3)
    assert doc.tolist() == [[4, 1, -1], [-1, -1, -1]] and score.tolist() == [[-0.5, -2.0, 0.0], [0.0, 0.0, 0.0]] and count.tolist() == [2, 0]
    assert not score[1].view(np.uint32).any()  # the padding is +0.0f
