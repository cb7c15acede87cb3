"""The IVF-PQ dense index without a GPU: the twenty-first header against its symbol table, the plan and workspace formulas
restated in ivfpq.py, one refusal per class of the new entry points (none reaches a device), the service refusals."""
import ctypes

import numpy as np
import pytest

import sparse_rx
from sparse_rx import _capi, ivfpq
from test_dense_scale_cpu import _ctype_class, _prototypes

P = [(i + 1) << 20 for i in range(16)]  # aligned addresses, never dereferenced


def test_table_agrees_with_the_header():
    protos = _prototypes("ivfpq/sparse_rx_ivfpq.h")
    assert set(protos) == set(_capi.IVFPQ_SYMBOLS) and len(protos) == 5
    for name, (res, args) in _capi.IVFPQ_SYMBOLS.items():
        assert (_ctype_class(res), [_ctype_class(a) for a in args]) == protos[name], name
    assert "dense_ivfpq.hip" in _capi.SOURCES and _capi.UNIT_FLAGS["dense_ivfpq.hip"] == _capi.UNIT_FLAGS["dense_pq.hip"]
    assert any(p.endswith("sparse_rx_ivfpq.h") for p in _capi._deps()) and any(p.endswith("ivf_probe.h") for p in _capi._deps())
    assert sparse_rx.IvfPqIndex is ivfpq.IvfPqIndex and {"ivfpq", "IvfPqIndex"} <= set(sparse_rx.__all__)


def test_plan_and_workspace_formulas():
    L = _capi.lib()
    for nq in (0, 1, 5, 33, 512, 1024, 5000):
        for nlist, nprobe, tiles in ((1, 1, 1), (6, 3, 4), (6, 6, 41), (4000, 64, 300), (65536, 1024, 2 ** 16)):
            for M, k in ((1, 1), (13, 10), (96, 100), (128, 1024)):
                assert L.srx_ivfpq_workspace_bytes(nq, nlist, nprobe, k, M, tiles) == ivfpq.search_plan(nq, nlist, nprobe, k, M, tiles)[3], (nq, nlist, nprobe, k, M, tiles)
    assert ivfpq.search_plan(1, 3, 3, 10, 2, 41)[:3] == (1, 8, 16) and ivfpq.search_plan(1024, 3, 3, 10, 2, 41)[1] == 1
    for bad in ((-1, 6, 3, 10, 4, 2), (1, 0, 1, 10, 4, 2), (1, 65537, 1, 10, 4, 2), (1, 6, 0, 10, 4, 2), (1, 6, 7, 10, 4, 2), (1, 6, 3, 0, 4, 2),
                (1, 6, 3, 1025, 4, 2), (1, 6, 3, 10, 0, 2), (1, 6, 3, 10, 129, 2), (1, 6, 3, 10, 4, 0), (1, 2000, 1024, 10, 4, 2 ** 17)):
        assert L.srx_ivfpq_workspace_bytes(*bad) == -1 and L.srx_last_error().startswith(b"srx_ivfpq_workspace_bytes")
    assert L.srx_ivfpq_score_docs_workspace_bytes(3, 10) == 256 + 256
    for bad in ((-1, 1), (1, 0), (2 ** 20, 2 ** 11)):
        assert L.srx_ivfpq_score_docs_workspace_bytes(*bad) == -1 and L.srx_last_error().startswith(b"srx_ivfpq_score_docs_workspace_bytes")


def _desc(**kw):
    d = dict(device=0, type=0, n_docs=1000, doc_base=0, n_tiles=20, max_list_tiles=5, dim=40, dsub=8, dim_pad=64, nlist=6, codes=P[0], codebooks=P[1],
             centroids=P[2], list_tile=P[3], row_doc=P[4], doc_row=P[5], tile_list=P[6])
    d.update(kw)
    return ctypes.byref(_capi.IvfPqDesc(**d))


def _encode(L, type=0, cent=P[2], nlist=6, dim_pad=64, x=P[7], ld=40, n_src=100, dim=40, dsub=8, cb=P[1], src=P[8], row_list=P[9], n_rows=128, row0=0,
            n_total=1280, out=P[0]):
    return L.srx_ivfpq_encode(0, type, cent, nlist, dim_pad, x, ld, n_src, dim, dsub, cb, src, row_list, n_rows, row0, n_total, out, None)


def _search(L, desc=None, queries=P[7], nq=3, nprobe=2, k=10, probe_list=None, filter=None, out_doc=P[8], out_score=P[9], out_count=P[10], ws=P[11],
            ws_bytes=1 << 30, **kw):
    return L.srx_ivfpq_search(desc if desc is not None else _desc(**kw), queries, nq, nprobe, k, probe_list, filter, out_doc, out_score, out_count, ws, ws_bytes, None, 0.0)


def _score_docs(L, desc=None, queries=P[7], nq=3, cand_doc=P[8], cand_count=None, m=10, out=P[9], ws=P[11], ws_bytes=1 << 20, **kw):
    return L.srx_ivfpq_score_docs(desc if desc is not None else _desc(**kw), queries, nq, cand_doc, cand_count, m, out, ws, ws_bytes, None)


def _filter(bits=P[12], n_filters=2, q_filter=P[13]):
    return ctypes.byref(_capi.DocFilterDesc(bits=bits, n_filters=n_filters, q_filter=q_filter))


NULL, AL16 = "null", "16-byte"
DESC = [({"type": 2}, "type must be"), ({"dsub": 5}, "dsub must be"), ({"dim": 0}, "<= dim <="), ({"dim": 516, "dsub": 4, "dim_pad": 576}, "must be <= 128"),
        ({"dim_pad": 128}, "dim_pad must be"), ({"nlist": 0}, "nlist"), ({"nlist": 1001}, "nlist"), ({"n_docs": 0}, "n_docs out of range"),
        ({"n_tiles": 0}, "n_tiles out of range"), ({"max_list_tiles": 21}, "max_list_tiles"), ({"doc_base": -1}, "must fit int32"),
        ({"codes": None}, NULL), ({"tile_list": None}, NULL), ({"doc_row": None}, NULL), ({"codebooks": P[1] + 4}, AL16)]
REFUSALS = [*[(f, kw, word) for f in (_search, _score_docs) for kw, word in DESC],
            (_search, {"desc": ctypes.POINTER(_capi.IvfPqDesc)()}, "null desc"), (_search, {"nq": -1}, "nq < 0"), (_search, {"nprobe": 0}, "nprobe"),
            (_search, {"nprobe": 7}, "nprobe"), (_search, {"k": 0}, "1 <= k <= 1024"), (_search, {"k": 1025}, "1 <= k <= 1024"),
            (_search, {"nprobe": 1024, "nlist": 2000, "n_docs": 2000, "n_tiles": 2 ** 25, "max_list_tiles": 2 ** 17}, "2^26"),
            (_search, {"queries": None}, NULL), (_search, {"queries": P[7] + 4}, AL16), (_search, {"out_doc": None}, "null output"),
            (_search, {"filter": _filter(bits=None)}, "null filter bits"), (_search, {"filter": _filter(n_filters=0)}, "n_filters must"),
            (_score_docs, {"nq": -1}, "nq < 0"), (_score_docs, {"m": 0}, "m must be >= 1"), (_score_docs, {"nq": 2 ** 20, "m": 2 ** 11}, "nq * m must fit"),
            (_score_docs, {"cand_doc": None}, NULL), (_score_docs, {"out": None}, NULL), (_score_docs, {"queries": P[7] + 8}, AL16),
            (_encode, {"type": -1}, "type must be"), (_encode, {"dsub": 0}, "dsub must be"), (_encode, {"dim_pad": 0}, "dim_pad must be"),
            (_encode, {"nlist": 65537}, "nlist"), (_encode, {"n_rows": -1}, "negative count"), (_encode, {"n_src": -1}, "negative count"),
            (_encode, {"row0": 1216}, "row0 + n_rows > n_total"), (_encode, {"ld": 39}, "ld >= dim"), (_encode, {"row0": 32}, "multiple of 64"),
            (_encode, {"n_rows": 2 ** 31, "n_total": 2 ** 31}, "too many rows"), (_encode, {"src": None}, NULL), (_encode, {"row_list": None}, NULL),
            (_encode, {"x": P[7] + 2}, "4-byte"), (_encode, {"cent": P[2] + 8}, AL16), (_encode, {"out": P[0] + 4}, AL16)]


@pytest.mark.parametrize("call,kw,word", REFUSALS, ids=[f"{c.__name__}-{'-'.join(k)}-{i}" for i, (c, k, _) in enumerate(REFUSALS)])
def test_refusals_fire_before_a_device_is_touched(call, kw, word):
    L = _capi.lib()
    assert call(L, **kw) == -1
    msg = L.srx_last_error().decode()
    assert msg.startswith("srx_ivfpq" + call.__name__ + ":") and word in msg, msg


def test_nomem_and_empty_calls():
    L = _capi.lib()
    need = L.srx_ivfpq_workspace_bytes(3, 6, 2, 10, 5, 5)
    assert _search(L, ws=None) == -3 and _search(L, ws_bytes=need - 1) == -3 and b"workspace too small" in L.srx_last_error()
    assert _score_docs(L, ws=None) == -3 and _score_docs(L, ws_bytes=511) == -3 and L.srx_last_error().startswith(b"srx_ivfpq_score_docs")
    empty = dict(codes=None, codebooks=None, centroids=None, list_tile=None, row_doc=None, doc_row=None, tile_list=None)
    assert _search(L, nq=0, queries=None, out_doc=None, out_score=None, out_count=None, ws=None, ws_bytes=0, **empty) == 0
    assert _search(L, nq=0, filter=_filter()) == 0 and _score_docs(L, nq=0, queries=None, cand_doc=None, out=None, ws=None, ws_bytes=0, **empty) == 0
    assert _encode(L, n_rows=0, x=None, cb=None, cent=None, src=None, row_list=None, out=None) == 0


def test_service_refusals_and_the_unchanged_messages():
    svc = sparse_rx.RetrievalService()
    e = np.zeros((4, 8), np.float32)
    lists = {"ann": "ivfpq", "nlist": 2, "nprobe": 1}
    for kw, match in [({**lists, "storage": "mxfp8"}, "ann='ivfpq' is not offered with storage='mxfp8'"),
                      ({**lists, "storage": "f16", "screen": "binary"}, "screen='binary' is not offered with ann='ivfpq'"),
                      ({**lists, "storage": "pq", "screen": "pq"}, "screen='pq' is not offered with storage='pq'"),
                      ({**lists, "storage": "f16"}, "ann='ivfpq' needs storage='pq'"), ({**lists, "storage": "int8"}, "storage must be .* or 'pq'"),
                      ({**lists, "storage": "pq", "nlist": 5}, "nlist must be in"), ({**lists, "storage": "pq", "nprobe": 3}, "nprobe must be in"),
                      ({**lists, "storage": "pq", "pq_dsub": 5}, "dsub must be 4, 8 or 16"),
                      ({"storage": "pq", "ann": "ivf", "nlist": 2, "nprobe": 1}, "ann='ivf' is not offered with storage='pq' or screen='pq'"),
                      ({"storage": "f16", "screen": "pq", "ann": "ivf", "nlist": 2, "nprobe": 1}, "there are no product-quantised lists"),
                      ({"storage": "f16", "ann": "hnsw"}, "ann must be"), ({"storage": "f32", "ann": "ivf", "nlist": 2, "nprobe": 1}, "ann='ivf' needs storage"),
                      ({"nlist": 2}, "nlist= / nprobe= need ann")]:
        with pytest.raises(ValueError, match=match):
            svc.set_embeddings(e, **kw)
    with pytest.raises(ValueError, match="ann='ivfpq' is not offered for token embeddings"):
        svc.set_token_embeddings({}, ann="ivfpq")
    svc._be.sharded = lambda: True
    for storage, screen in (("pq", None), ("f16", "pq")):
        with pytest.raises(ValueError, match="ann='ivfpq' is not offered with a sharded index"):
            svc.set_embeddings(e, storage=storage, screen=screen, **lists)
    assert getattr(svc, "_dense", None) is None and not hasattr(ivfpq.IvfPqIndex, "mmr_device")
    svc._dense, svc.embedding_storage, svc.embedding_ann = object(), "pq", "ivfpq"
    with pytest.raises(ValueError, match="is not offered with storage='pq', ann='ivfpq'"):
        svc._need_mmr_rows("diversify()")
    svc._dense = None
    svc.close()
