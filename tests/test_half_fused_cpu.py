"""The fused half-precision search without a GPU: its header, unit and symbol table, the refusals of srx_dense_search_half (none
reaches a device), the workspace without the score matrix, and the ValueErrors of the service keyword."""
import ctypes
import os
import re

import numpy as np
import pytest

import sparse_rx
from sparse_rx import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(12)]  # 16-byte aligned addresses, never dereferenced


def test_header_unit_and_table():
    hdr = open(os.path.join(ROOT, "include", "fused", "sparse_rx_half_fused.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr.split("#ifndef")[1]))
    assert declared == set(_capi.HALF_FUSED_SYMBOLS) and len(declared) == 2
    deps = [os.path.basename(p) for p in _capi._deps()]
    assert "dense_half_fused.hip" in _capi.SOURCES and {"sparse_rx_half_fused.h", "dense_half_fused.hip"} <= set(deps)
    assert _capi.INCLUDED_SOURCES["dense_half_fused.hip"] == ["dense_half.hip"]  # the shared kernels: one copy of the text
    for name, value in (("CAP", _capi.SRX_HALF_FUSED_CAP), ("MIN_DOCS", _capi.SRX_HALF_FUSED_MIN_DOCS), ("PASS", _capi.SRX_HALF_FUSED_PASS)):
        assert re.search(rf"#define SRX_HALF_FUSED_{name} {value}\b", hdr), name
    L = _capi.lib()
    for name, (res, args) in _capi.HALF_FUSED_SYMBOLS.items():
        f = getattr(L, name)
        assert f.restype is res and list(f.argtypes) == args, name
    # the sample rule on both sides of each of its edges
    assert [_capi.half_fused_sample(n, k) for n, k in ((65535, 10), (65536, 10), (65536, 1024), (10 ** 6, 10), (10 ** 6, 1000), (10 ** 7, 100))] == \
        [0, 4096, 16384, 4096, 45824, 45824]


def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg and b"srx_dense_search_half_fused" in msg, (rc, msg)


@pytest.mark.parametrize("type_", [0, 1])
def test_search_refusals(type_):
    L = _capi.lib()
    flt = lambda **kw: ctypes.byref(_capi.DocFilterDesc(**{**dict(bits=P[8], n_filters=1, q_filter=None), **kw}))
    ok = dict(device=0, type=type_, corpus=P[0], n_docs=1000, dim_pad=64, queries=P[2], nq=2, k=10, doc_base=0, filter=None, out_doc=P[3],
              out_score=P[4], out_count=P[5], ws=P[6], ws_bytes=1 << 30, stream=None, offset=0.0)
    call = lambda **kw: L.srx_dense_search_half_fused(*{**ok, **kw}.values())
    _refused(call(type=2), "type must be")
    _refused(call(type=2, filter=flt(bits=None), k=0), "type must be")  # the order of the checks: type, filter, counts, ...
    _refused(call(filter=flt(bits=None), k=0), "null filter bits")
    _refused(call(filter=flt(n_filters=0)), "n_filters")
    for kw in (dict(nq=-1), dict(n_docs=0), dict(k=0), dict(k=1025, dim_pad=32)):
        _refused(call(**kw), "need n_docs > 0")
    for d in (0, 32, 96, 1088):
        _refused(call(dim_pad=d, doc_base=-1), "multiple of 64")
    _refused(call(doc_base=-1, corpus=None), "doc_base")
    _refused(call(doc_base=2 ** 31 - 1 - 1000), "doc_base")
    for null in ("corpus", "queries", "out_doc", "out_score", "out_count"):
        _refused(call(**{null: None}), "null pointer")
    _refused(call(corpus=P[0] + 4, ws=None), "16-byte aligned")
    need = L.srx_dense_half_fused_workspace_bytes(2, 1000, 10)
    assert call(ws=None) == -3 and call(ws_bytes=need - 1) == -3 and call(filter=flt(), ws_bytes=need - 1) == -3  # SRX_ERR_NOMEM, against its own size
    assert call(nq=0, queries=None) == 0  # nothing to do: no launch


def test_workspace_has_no_matrix():
    L = _capi.lib()
    for args in ((-1, 100, 10), (1, 0, 10), (1, 100, 0), (1, 100, 1025)):
        assert L.srx_dense_half_fused_workspace_bytes(*args) == -1 and b"srx_dense_half_fused_workspace_bytes" in L.srx_last_error()
    fused, matrix = L.srx_dense_half_fused_workspace_bytes(1024, 10_000_000, 10), L.srx_dense_half_workspace_bytes(1024, 10_000_000, 10)
    # the matrix route holds 96 queries x 10 M docs x 4 bytes at this size (its pass keeps the matrix within 4 GiB).  The fused
    # workspace is that call's without the matrix, plus the candidate buffers (8 bytes x CAP per query), a sample of 4 608 docs, the
    # packed block of a full pass and the fallback's 64 lists per query
    ld = -(-10_000_000 // 64) * 64
    assert matrix >= 96 * ld * 4
    assert fused <= matrix - 96 * ld * 4 + 1024 * _capi.SRX_HALF_FUSED_CAP * 8 + 1024 * 4608 * 4 + 1024 * 2048 + 1024 * 64 * (8 * 10 + 4) + (1 << 20) and fused * 6 < matrix
    # the header's formula; its only terms in n_docs are the sample's columns and the fallback's lists
    r = lambda b: -(-b // 256) * 256
    for nq, n, k in ((1024, 10_000_000, 10), (3000, 10 ** 9, 1000), (5, 100, 1024), (130, 65543, 10)):
        qb, S, lists = min(nq, 1024), _capi.half_fused_sample(n, k), min(nq, 1024) * max(1, min(-(-n // 32) // 64, 4096 // k, 64))
        want = (r(-(-qb // 128) * 128 * 2048) + r(qb * S * 4) + 2 * r(lists * k * 4) + r(lists * 4) + r(qb * 4) + r((qb * 33 + 1) * 4)
                + 2 * r(qb * _capi.SRX_HALF_FUSED_CAP * 4) + 256)
        assert L.srx_dense_half_fused_workspace_bytes(nq, n, k) == want, (nq, n, k)


def test_service_keyword_refusals():
    svc = sparse_rx.RetrievalService(device="cuda:0")
    e = np.zeros((4, 8), np.float32)
    for storage in ("f32", "mxfp8", "mxfp4", "pq"):
        with pytest.raises(ValueError, match="fused=True needs storage"):
            svc.set_embeddings(e, storage=storage, fused=True)
    for kw in (dict(ann="ivf", nlist=2, nprobe=1), dict(ann="graph"), dict(screen="binary"), dict(screen="pq")):
        with pytest.raises(ValueError, match="fused=True is not offered"):
            svc.set_embeddings(e, storage="bf16", fused=True, **kw)
    assert sparse_rx.DenseHalfIndex.fused is False
