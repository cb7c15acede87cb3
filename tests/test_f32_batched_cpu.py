"""The batched f32 search without a GPU: its header, unit and symbol table, the sample and workspace formulas against their Python
restatements, the refusals of srx_dense_search_f32_filtered (none reaches a device) and the ValueErrors of the service keyword."""
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
    hdr = open(os.path.join(ROOT, "include", "batched", "sparse_rx_f32_batched.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr.split("#ifndef")[1]))
    assert declared == set(_capi.F32_BATCHED_SYMBOLS) and len(declared) == 2
    deps = [os.path.basename(p) for p in _capi._deps()]
    assert "dense_f32_batched.hip" in _capi.SOURCES and {"sparse_rx_f32_batched.h", "dense_f32_batched.hip"} <= set(deps)
    assert "dense_f32_batched.hip" not in _capi.UNIT_FLAGS and "-ffp-contract=off" in _capi.HIPCC_FLAGS  # the flags of dense.hip and dense_score.hip
    for name in ("CAP", "MIN_DOCS", "PASS", "TARGET", "MAX_SAMPLE"):
        assert re.search(rf"#define SRX_F32_BATCHED_{name} {getattr(_capi, 'SRX_F32_BATCHED_' + name)}\b", hdr), name
    ratio, c = (float(re.search(rf"#define SRX_F32_BATCHED_{n} ([0-9.]+)", hdr).group(1)) for n in ("MEASURED_RATIO", "C"))
    assert c == max(2.0, 4.0 * ratio) and ratio > 0.0  # the issue's rule for c, from a ratio that was measured
    L = _capi.lib()
    for name, (res, args) in _capi.F32_BATCHED_SYMBOLS.items():
        f = getattr(L, name)
        assert f.restype is res and list(f.argtypes) == args, name
    # the sample rule on both sides of each of its edges: no sample, the floor, the target term, the cap, 4 S > n_docs
    cases = ((65535, 10), (65536, 10), (65536, 1024), (10 ** 6, 10), (10 ** 6, 1000), (10 ** 7, 1000), (65535 + 78, 1024), (60000 * 4, 1000))
    assert [_capi.f32_batched_sample(n, k) for n, k in cases] == [0, 4096, 16384, 4096, 122112, 262144, 16384, 29312]


def test_workspace_formula():
    L = _capi.lib()
    for args in ((-1, 100, 10), (1, 0, 10), (1, 100, 0), (1, 100, 1025)):
        assert L.srx_dense_f32_batched_workspace_bytes(*args) == -1 and b"srx_dense_f32_batched_workspace_bytes" in L.srx_last_error()
    for nq, n, k in ((1024, 10_000_000, 10), (3000, 10 ** 9, 1000), (5, 100, 1024), (130, 65543, 10), (1, 1, 1)):
        assert L.srx_dense_f32_batched_workspace_bytes(nq, n, k) == _capi.f32_batched_workspace(nq, n, k), (nq, n, k)


def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg and b"srx_dense_search_f32_batched" in msg, (rc, msg)


def test_search_refusals():
    L = _capi.lib()
    flt = lambda **kw: ctypes.byref(_capi.DocFilterDesc(**{**dict(bits=P[8], n_filters=1, q_filter=None), **kw}))
    ok = dict(device=0, emb=P[0], n_docs=1000, dim=64, queries=P[2], nq=2, k=10, doc_base=0, filter=None, out_doc=P[3], out_score=P[4],
              out_count=P[5], ws=P[6], ws_bytes=1 << 30, stream=None, offset=0.0)
    call = lambda **kw: L.srx_dense_search_f32_batched(*{**ok, **kw}.values())
    _refused(call(filter=flt(bits=None), k=0), "null filter bits")  # the order of the checks: filter, counts, dim, doc_base, pointers
    _refused(call(filter=flt(n_filters=0)), "n_filters")
    for kw in (dict(nq=-1), dict(n_docs=0), dict(k=0), dict(k=1025, dim=32)):
        _refused(call(**kw), "need n_docs > 0")
    for d in (0, 32, 96, 1088):
        _refused(call(dim=d, doc_base=-1), "multiple of 64")
    _refused(call(doc_base=-1, emb=None), "doc_base")
    _refused(call(doc_base=2 ** 31 - 1 - 1000), "doc_base")
    for null in ("emb", "queries", "out_doc", "out_score", "out_count"):
        _refused(call(**{null: None}), "null pointer")
    need = L.srx_dense_f32_batched_workspace_bytes(2, 1000, 10)
    assert call(ws=None) == -3 and call(ws_bytes=need - 1) == -3 and call(filter=flt(), ws_bytes=need - 1) == -3  # SRX_ERR_NOMEM, against its own size
    assert call(nq=0, queries=None) == 0  # nothing to do: no launch


def test_keyword_refusals():
    svc = sparse_rx.RetrievalService(device="cuda:0")
    e = np.zeros((4, 8), np.float32)
    for storage in ("f16", "bf16", "mxfp8", "mxfp4", "pq"):
        with pytest.raises(ValueError, match="batched=True needs storage"):
            svc.set_embeddings(e, storage=storage, batched=True)
    for kw in (dict(ann="ivfpq", nlist=2, nprobe=1), dict(screen="binary"), dict(screen="pq")):
        with pytest.raises(ValueError, match="batched=True is not offered"):
            svc.set_embeddings(e, storage="f32", batched=True, **kw)
    assert sparse_rx.DenseF32Index.batched is False
