"""The PQ dense index without a GPU: the twentieth header against its symbol table, the byte and workspace formulas restated in
pq.py, one refusal per stated reason (none reaches a device), the service and pairing refusals."""
import ctypes

import numpy as np
import pytest

import sparse_rx
from sparse_rx import _capi, pq
from test_dense_scale_cpu import _ctype_class, _prototypes

P = [(i + 1) << 20 for i in range(10)]  # aligned addresses, never dereferenced


def test_table_agrees_with_the_header():
    protos = _prototypes("pq/sparse_rx_pq.h")
    assert set(protos) == set(_capi.PQ_SYMBOLS) and len(protos) == 6
    for name, (res, args) in _capi.PQ_SYMBOLS.items():
        assert (_ctype_class(res), [_ctype_class(a) for a in args]) == protos[name], name
        f = getattr(_capi.lib(), name)
        assert f.restype is res and list(f.argtypes) == args
    assert "dense_pq.hip" in _capi.SOURCES and any(p.endswith("sparse_rx_pq.h") for p in _capi._deps())
    assert sparse_rx.DensePqIndex is pq.DensePqIndex and {"pq", "DensePqIndex"} <= set(sparse_rx.__all__)


def test_byte_and_workspace_formulas():
    L = _capi.lib()
    for n in (0, 1, 64, 65, 10 ** 7, 2 ** 31 - 2):
        for M in (1, 16, 17, 96, 128):
            assert L.srx_pq_bytes(n, M) == pq.pq_bytes(n, M) == -(-n // 64) * 64 * -(-M // 16) * 16
    for nq in (0, 1, 33, 1024, 5000):
        for n in (1, 64, 65, 16384, 40_000, 10 ** 6, 2 ** 25 + 1, 2 ** 31 - 2):
            for M, k in ((1, 1), (4, 10), (96, 100), (128, 1024)):
                assert L.srx_pq_workspace_bytes(nq, n, M, k) == pq.search_plan(nq, n, M, k)[2], (nq, n, M, k)
    for bad in ((-1, 1), (1, 0), (1, 129)):
        assert L.srx_pq_bytes(*bad) == -1 and L.srx_last_error().startswith(b"srx_pq_bytes")
    for bad in ((-1, 10, 4, 1), (1, 0, 4, 1), (1, 10, 0, 1), (1, 10, 129, 1), (1, 10, 4, 0), (1, 10, 4, 1025)):
        assert L.srx_pq_workspace_bytes(*bad) == -1 and L.srx_last_error().startswith(b"srx_pq_workspace_bytes")
    for dim, dsub, M in ((1, 4, 1), (3, 4, 1), (200, 16, 13), (512, 4, 128), (1024, 8, 128), (768, 8, 96)):
        assert pq.subspaces(dim, dsub) == M
    for dim, dsub in ((0, 8), (1025, 8), (513, 4), (768, 5)):
        with pytest.raises(ValueError):
            pq.subspaces(dim, dsub)


def _encode(L, x=P[0], ld=40, n_rows=100, dim=40, dsub=8, row0=0, n_total=100, cb=P[1], tiled=1, out=P[2]):
    return L.srx_pq_encode(0, x, ld, n_rows, dim, dsub, row0, n_total, cb, tiled, out, None)


def _lut(L, cb=P[0], dim=40, dsub=8, queries=P[1], ldq=40, nq=3, out=P[2]):
    return L.srx_pq_lut(0, cb, dim, dsub, queries, ldq, nq, out, None)


def _search(L, codes=P[0], n_docs=1000, dim=40, dsub=8, cb=P[1], queries=P[2], ldq=40, nq=3, k=10, doc_base=0, filter=None, out_doc=P[3], out_score=P[4],
            out_count=P[5], ws=P[6], ws_bytes=1 << 30):
    return L.srx_pq_search(0, codes, n_docs, dim, dsub, cb, queries, ldq, nq, k, doc_base, filter, out_doc, out_score, out_count, ws, ws_bytes, None, 0.0)


def _score_docs(L, codes=P[0], n_docs=1000, dim=40, dsub=8, cb=P[1], queries=P[2], ldq=40, nq=3, doc_base=0, cand_doc=P[3], cand_count=P[4], m=10,
                out=P[5]):
    return L.srx_pq_score_docs(0, codes, n_docs, dim, dsub, cb, queries, ldq, nq, doc_base, cand_doc, cand_count, m, out, None)


def _filter(bits=P[7], n_filters=2, q_filter=P[8]):
    return ctypes.byref(_capi.DocFilterDesc(bits=bits, n_filters=n_filters, q_filter=q_filter))


GEOMETRY = [({"dsub": 5}, "dsub must be"), ({"dsub": 0}, "dsub must be"), ({"dim": 0, "ld": 40}, "<= dim <="), ({"dim": 1025, "ld": 2000, "ldq": 2000}, "<= dim <="),
            ({"dim": 516, "dsub": 4, "ld": 516, "ldq": 516}, "must be <= 128")]
NULL, AL16, AL4 = "null pointer", "16-byte", "4-byte"
# (the call, changed arguments, a phrase only the refusing check's message has)
REFUSALS = [*[(f, {k: v for k, v in kw.items() if k in f.__code__.co_varnames}, word) for f in (_encode, _lut, _search, _score_docs) for kw, word in GEOMETRY],
            (_encode, {"tiled": 2}, "tiled must be"), (_encode, {"n_rows": -1}, "negative count"), (_encode, {"row0": -64}, "negative count"),
            (_encode, {"n_total": -1}, "negative count"), (_encode, {"row0": 64}, "row0 + n_rows > n_total"), (_encode, {"ld": 39}, "ld >= dim"),
            (_encode, {"row0": 32, "n_rows": 10}, "multiple of 64"), (_encode, {"n_rows": 2 ** 37 + 1, "n_total": 2 ** 37 + 1}, "too many rows"),
            (_encode, {"x": None}, NULL), (_encode, {"cb": None}, NULL), (_encode, {"out": None}, NULL), (_encode, {"x": P[0] + 2}, AL4),
            (_encode, {"cb": P[1] + 4}, AL16), (_encode, {"out": P[2] + 8}, AL16),
            (_lut, {"nq": -1}, "nq < 0"), (_lut, {"ldq": 39}, "ldq >= dim"), (_lut, {"cb": None}, NULL), (_lut, {"queries": None}, NULL), (_lut, {"out": None}, NULL),
            (_lut, {"queries": P[1] + 1}, AL4), (_lut, {"cb": P[0] + 8}, AL16), (_lut, {"out": P[2] + 4}, AL16),
            (_search, {"filter": _filter(bits=None)}, "null filter bits"), (_search, {"filter": _filter(bits=P[7] + 4)}, "filter rows must be 16-byte aligned"),
            (_search, {"filter": _filter(n_filters=0)}, "n_filters must"), (_search, {"nq": -1}, "1 <= k <= 1024"), (_search, {"n_docs": 0}, "n_docs > 0"),
            (_search, {"k": 0}, "1 <= k <= 1024"), (_search, {"k": 1025}, "1 <= k <= 1024"), (_search, {"ldq": 39}, "ldq >= dim"),
            (_search, {"doc_base": -1}, "must fit int32"), (_search, {"doc_base": 2 ** 31 - 1001}, "must fit int32"),
            *[(_search, {name: None}, NULL) for name in ("codes", "cb", "queries", "out_doc", "out_score", "out_count")],
            (_search, {"codes": P[0] + 8}, AL16), (_search, {"cb": P[1] + 4}, AL16), (_search, {"queries": P[2] + 2}, AL4),
            (_score_docs, {"nq": -1}, "nq < 0"), (_score_docs, {"m": 0}, "m must be >= 1"), (_score_docs, {"nq": 2 ** 20, "m": 2 ** 11}, "nq * m must fit"),
            (_score_docs, {"n_docs": 0}, "n_docs out of range"), (_score_docs, {"n_docs": 2 ** 31 - 1}, "n_docs out of range"), (_score_docs, {"ldq": 39}, "ldq >= dim"),
            (_score_docs, {"doc_base": -1}, "doc_base < 0"), *[(_score_docs, {name: None}, NULL) for name in ("codes", "cb", "queries", "cand_doc", "out")],
            (_score_docs, {"codes": P[0] + 4}, AL16), (_score_docs, {"queries": P[2] + 3}, AL4)]


@pytest.mark.parametrize("call,kw,word", REFUSALS, ids=[f"{c.__name__}-{'-'.join(k)}-{i}" for i, (c, k, _) in enumerate(REFUSALS)])
def test_refusals_fire_before_a_device_is_touched(call, kw, word):
    L = _capi.lib()
    assert call(L, **kw) == -1
    msg = L.srx_last_error().decode()
    assert msg.startswith("srx_pq" + call.__name__ + ":") and word in msg, msg


def test_nomem_and_empty_calls():
    L = _capi.lib()
    need = L.srx_pq_workspace_bytes(3, 1000, 5, 10)
    assert _search(L, ws=None) == -3 and _search(L, ws_bytes=need - 1) == -3 and b"workspace too small" in L.srx_last_error()
    assert _search(L, nq=1025, n_docs=40_000, ws_bytes=L.srx_pq_workspace_bytes(1, 40_000, 5, 10)) == -3
    assert _search(L, nq=0, codes=None, cb=None, queries=None, out_doc=None, out_score=None, out_count=None, ws=None, ws_bytes=0) == 0
    assert _search(L, nq=0, filter=_filter()) == 0 and _lut(L, nq=0, cb=None, queries=None, out=None) == 0
    assert _score_docs(L, nq=0, codes=None, cb=None, queries=None, cand_doc=None, cand_count=None, out=None) == 0
    assert _encode(L, n_rows=0, x=None, cb=None, out=None) == 0 and _encode(L, n_rows=0, row0=64) == 0 and _encode(L, n_rows=0, row0=33, tiled=0) == 0


def test_service_and_pairing_refusals():
    svc = sparse_rx.RetrievalService()
    e = np.zeros((4, 8), np.float32)
    for kw, match in [({"storage": "pq", "ann": "ivf", "nlist": 2, "nprobe": 1}, "ann='ivf' is not offered with storage='pq' or screen='pq'"),
                      ({"storage": "f16", "screen": "pq", "ann": "ivf", "nlist": 2, "nprobe": 1}, "ann='ivf' is not offered with storage='pq' or screen='pq'"),
                      ({"storage": "pq", "screen": "binary"}, "screen='binary' is not offered with storage='pq'"),
                      ({"storage": "pq", "screen": "pq"}, "screen='pq' is not offered with storage='pq'"),
                      ({"storage": "mxfp8", "screen": "pq"}, "screen='pq' is not offered with storage='mxfp8'"),
                      ({"screen": "bogus"}, "screen must be None or 'binary' or 'pq'"), ({"storage": "int8"}, "storage must be .* or 'pq'"),
                      ({"storage": "pq", "pq_dsub": 5}, "dsub must be 4, 8 or 16"), ({"screen": "pq", "oversample": 0}, "oversample")]:
        with pytest.raises(ValueError, match=match):
            svc.set_embeddings(e, **kw)
    with pytest.raises(ValueError, match="storage='pq' is not offered for token embeddings"):
        svc.set_token_embeddings({}, storage="pq")
    svc._be.sharded = lambda: True
    with pytest.raises(ValueError, match="storage='pq' is not offered with a sharded index"):
        svc.set_embeddings(e, storage="pq")
    with pytest.raises(ValueError, match="screen='pq' is not offered with a sharded index"):
        svc.set_embeddings(e, screen="pq")
    assert getattr(svc, "_dense", None) is None
    svc._dense, svc.embedding_storage = object(), "pq"  # an index without mmr_device, as DensePqIndex is
    assert not hasattr(pq.DensePqIndex, "mmr_device")
    with pytest.raises(ValueError, match="is not offered with storage='pq'"):
        svc._need_mmr_rows("diversify()")
    svc._dense = None
    svc.close()
    with pytest.raises(ValueError, match="DenseF32Index or a DenseHalfIndex"):
        sparse_rx.ScreenedDenseIndex(object(), object())
    exact = object.__new__(sparse_rx.DenseF32Index)
    with pytest.raises(ValueError, match="the screen must be a DenseBinaryIndex or a DensePqIndex"):
        sparse_rx.ScreenedDenseIndex(exact, object())
