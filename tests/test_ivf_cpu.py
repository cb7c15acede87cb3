"""The IVF dense index without a GPU: the nineteenth header against its symbol table, the workspace formula restated in ivf.py, one
refusal per stated reason (none reaches a device), the service's refusals."""
import ctypes

import numpy as np
import pytest

import sparse_rx
from sparse_rx import _capi, ivf
from test_dense_scale_cpu import _ctype_class, _prototypes

P = [(i + 1) << 20 for i in range(10)]  # aligned addresses, never dereferenced


def test_table_agrees_with_the_header():
    protos = _prototypes("ivf/sparse_rx_ivf.h")
    assert set(protos) == set(_capi.IVF_SYMBOLS) and len(protos) == 5
    for name, (res, args) in _capi.IVF_SYMBOLS.items():
        assert (_ctype_class(res), [_ctype_class(a) for a in args]) == protos[name], name
        f = getattr(_capi.lib(), name)
        assert f.restype is res and list(f.argtypes) == args
    assert "dense_ivf.hip" in _capi.SOURCES and any(p.endswith("sparse_rx_ivf.h") for p in _capi._deps())
    assert sparse_rx.IvfHalfIndex is ivf.IvfHalfIndex and "IvfHalfIndex" in sparse_rx.__all__
    assert ctypes.sizeof(_capi.IvfDesc) == 88


@pytest.mark.parametrize("nq,nlist,nprobe,k,tiles", [(1, 1, 1, 1, 1), (33, 130, 2, 10, 5), (129, 130, 130, 1024, 7), (5000, 65536, 1024, 100, 300),
                                                     (7, 4000, 64, 10, 1 << 20), (1024, 33, 33, 5, 40)])
def test_workspace_formula(nq, nlist, nprobe, k, tiles):
    assert _capi.lib().srx_ivf_workspace_bytes(nq, nlist, nprobe, k, tiles) == ivf.workspace_bytes(nq, nlist, nprobe, k, tiles)


def _desc(**kw):
    d = dict(device=0, type=0, n_docs=1000, doc_base=0, n_tiles=40, max_list_tiles=9, dim_pad=128, nlist=33, corpus=P[0], centroids=P[1],
             list_tile=P[2], row_doc=P[3], doc_row=P[4])
    d.update(kw)
    return _capi.IvfDesc(**d)


def _assign(L, type=0, cent=P[0], nlist=33, dim=40, dim_pad=64, rows=P[1], ld=40, n=100, out=P[2]):
    return L.srx_ivf_assign(0, type, cent, nlist, dim, dim_pad, rows, ld, n, out, None, None)


def _update(L, rows=P[0], ld=40, dim=40, nlist=33, ptr=P[1], member=P[2], prev=P[3], out=P[4]):
    return L.srx_ivf_update(0, rows, ld, dim, nlist, ptr, member, prev, out, None)


def _probe(L, desc=..., queries=P[5], nq=3, nprobe=4, out=P[6], ws=P[8], ws_bytes=1 << 30, **kw):
    return L.srx_ivf_probe(ctypes.byref(_desc(**kw)) if desc is ... else desc, queries, nq, nprobe, out, P[7], ws, ws_bytes, None)


def _search(L, desc=..., queries=P[5], nq=3, nprobe=4, k=10, probe_list=None, filter=None, out_doc=P[6], ws=P[9], ws_bytes=1 << 40, **kw):
    return L.srx_ivf_search(ctypes.byref(_desc(**kw)) if desc is ... else desc, queries, nq, nprobe, k, probe_list, filter, out_doc, P[7], P[8], ws,
                            ws_bytes, None, 0.0)


NLIST, NPROBE, NULL, AL16 = "<= nlist <=", "<= nprobe <=", "null pointer", "16-byte"
# (changed arguments, a phrase only the refusing check's message has)
DESC = [({"type": 2}, "type must"), ({"dim_pad": 96}, "dim_pad must"), ({"dim_pad": 1088}, "dim_pad must"), ({"nlist": 0}, NLIST),
        ({"nlist": 65537, "n_docs": 1 << 20}, NLIST), ({"nlist": 1001}, NLIST), ({"n_docs": 0}, "n_docs out of range"),
        ({"n_docs": 2 ** 31 - 1}, "n_docs out of range"), ({"n_tiles": 0}, "n_tiles out of range"), ({"n_tiles": (1 << 26) + 1}, "n_tiles out of range"),
        ({"max_list_tiles": 0}, "<= max_list_tiles"), ({"max_list_tiles": 41}, "<= max_list_tiles"), ({"doc_base": -1}, "doc_base + n_docs"),
        ({"doc_base": 2 ** 31 - 1001}, "doc_base + n_docs"), ({"corpus": None}, "desc holds"), ({"centroids": None}, "desc holds"), ({"list_tile": None}, "desc holds"),
        ({"row_doc": None}, "desc holds"), ({"corpus": P[0] + 8}, "centroids must be 16"), ({"centroids": P[1] + 8}, "centroids must be 16"), ({"desc": None}, "null desc"), ({"nq": -1}, "nq < 0"),
        ({"nprobe": 0}, NPROBE), ({"nprobe": 34}, NPROBE), ({"nprobe": 1025, "nlist": 2000, "n_docs": 4000}, NPROBE), ({"queries": None}, "null queries"),
        ({"queries": P[5] + 4}, "queries must be 16")]
REFUSALS = [(_assign, {"type": -1}, "type must"), (_assign, {"dim_pad": 32}, "dim_pad must"), (_assign, {"nlist": 0}, NLIST), (_assign, {"nlist": 65537}, NLIST),
            (_assign, {"n": -1}, "n out of range"), (_assign, {"n": 2 ** 31}, "n out of range"), (_assign, {"dim": 0}, "<= dim <="),
            (_assign, {"dim": 65}, "<= dim <="), (_assign, {"ld": 39}, "ld >= dim"), (_assign, {"cent": None}, NULL), (_assign, {"rows": None}, NULL),
            (_assign, {"out": None}, NULL), (_assign, {"rows": P[1] + 2}, "4-byte"), (_assign, {"cent": P[0] + 8}, AL16),
            (_update, {"nlist": 0}, NLIST), (_update, {"dim": 0}, "<= dim <="), (_update, {"dim": 1025, "ld": 1025}, "<= dim <="), (_update, {"ld": 39}, "ld >= dim"),
            (_update, {"rows": None}, NULL), (_update, {"ptr": None}, NULL), (_update, {"member": None}, NULL), (_update, {"prev": None}, NULL),
            (_update, {"out": None}, NULL), (_update, {"rows": P[0] + 1}, "4-byte"),
            *[(f, kw, word) for f in (_probe, _search) for kw, word in DESC], (_probe, {"out": None}, "null output"), (_search, {"out_doc": None}, "null output"),
            (_search, {"k": 0}, "<= k <="), (_search, {"k": 1025}, "<= k <="),
            (_search, {"filter": ctypes.byref(_capi.DocFilterDesc(bits=None, n_filters=1, q_filter=None))}, "null filter bits"),
            (_search, {"filter": ctypes.byref(_capi.DocFilterDesc(bits=P[6], n_filters=0, q_filter=None))}, "n_filters must")]


@pytest.mark.parametrize("call,kw,word", REFUSALS, ids=[f"{c.__name__}-{'-'.join(k)}-{i}" for i, (c, k, _) in enumerate(REFUSALS)])
def test_refusals_fire_before_a_device_is_touched(call, kw, word):
    L = _capi.lib()
    assert call(L, **kw) == -1
    msg = L.srx_last_error().decode()
    assert msg.startswith(call.__name__.replace("_", "srx_ivf_", 1) + ":") and word in msg, msg


def test_nomem_and_empty_calls():
    L = _capi.lib()
    assert _probe(L, ws=None) == -3 and _probe(L, ws_bytes=3 * 64 * 4 - 1) == -3
    assert _search(L, ws=None) == -3 and _search(L, ws_bytes=L.srx_ivf_workspace_bytes(3, 33, 4, 10, 9) - 1) == -3
    assert _search(L, nq=0, queries=None, corpus=None, ws=None, ws_bytes=0) == 0 and _probe(L, nq=0, queries=None, ws=None) == 0
    assert _assign(L, n=0, cent=None, rows=None, out=None) == 0
    for bad in [(-1, 33, 4, 10, 9), (3, 0, 1, 10, 9), (3, 65537, 4, 10, 9), (3, 33, 0, 10, 9), (3, 33, 34, 10, 9), (3, 2000, 1025, 10, 9),
                (3, 33, 4, 0, 9), (3, 33, 4, 1025, 9), (3, 33, 4, 10, 0)]:
        assert L.srx_ivf_workspace_bytes(*bad) == -1, bad


def test_service_refusals():
    svc = sparse_rx.RetrievalService()
    e = np.zeros((4, 8), np.float32)
    for kw, match in [({"storage": "f32"}, "ann='ivf' needs storage"), ({"storage": "mxfp8"}, "ann='ivf' needs storage"),
                      ({"storage": "f16", "screen": "binary"}, "screen='binary' is not offered with ann"), ({"storage": "f16", "ann": "hnsw"}, "ann must be"),
                      ({"storage": "f16", "nlist": 5}, "nlist must be"), ({"storage": "f16", "nlist": 0}, "nlist must be"),
                      ({"storage": "bf16", "nlist": 2, "nprobe": 3}, "nprobe must be"), ({"storage": "f16", "nlist": 2, "nprobe": 0}, "nprobe must be")]:
        with pytest.raises(ValueError, match=match):
            svc.set_embeddings(e, **{"ann": "ivf", "nlist": 2, "nprobe": 1, **kw})
    with pytest.raises(ValueError, match="nlist= / nprobe= need ann"):
        svc.set_embeddings(e, storage="f16", nlist=2)
    svc._be.sharded = lambda: True
    with pytest.raises(ValueError, match="ann='ivf' is not offered with a sharded index"):
        svc.set_embeddings(e, storage="f16", ann="ivf", nlist=2, nprobe=1)
    assert getattr(svc, "_dense", None) is None
    svc.close()
