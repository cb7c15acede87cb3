"""The MX dense index without a GPU: the eighteenth header against its symbol table, the byte formula, one refusal per stated
reason (none reaches a device), the reference quantiser checked against itself and against torch's e4m3, the service's refusals."""
import ctypes

import numpy as np
import pytest
import torch

import mx_ref as ref
import sparse_rx
from sparse_rx import _capi
from test_dense_scale_cpu import _ctype_class, _prototypes

P = [(i + 1) << 20 for i in range(8)]  # aligned addresses, never dereferenced


def test_table_agrees_with_the_header():
    protos = _prototypes("mx/sparse_rx_mx.h")
    assert set(protos) == set(_capi.MX_SYMBOLS) and len(protos) == 5
    for name, (res, args) in _capi.MX_SYMBOLS.items():
        assert (_ctype_class(res), [_ctype_class(a) for a in args]) == protos[name], name
        f = getattr(_capi.lib(), name)
        assert f.restype is res and list(f.argtypes) == args
    assert "dense_mx.hip" in _capi.SOURCES and any(p.endswith("sparse_rx_mx.h") for p in _capi._deps())
    assert sparse_rx.DenseMxIndex is sparse_rx.mx.DenseMxIndex and "DenseMxIndex" in sparse_rx.__all__
    assert _capi.lib().srx_version() == 301


@pytest.mark.parametrize("dtype", list(ref.TYPES))
@pytest.mark.parametrize("dim_pad", [64, 256, 320, 1024])
def test_bytes(dtype, dim_pad):
    L = _capi.lib()
    for n in (0, 1, 32, 33):
        assert L.srx_mx_bytes(ref.TYPES[dtype], n, dim_pad) == ref.nbytes(dtype, n, dim_pad)
    assert L.srx_mx_workspace_bytes(5, 1000, 10) == L.srx_dense_half_workspace_bytes(5, 1000, 10)


def _convert(L, type=0, emb=P[0], ld=40, n_rows=100, dim=40, dim_pad=64, row0=0, n_total=100, out=P[1]):
    return L.srx_mx_convert(0, type, emb, ld, n_rows, dim, dim_pad, row0, n_total, out, None, None)


def _search(L, type=0, corpus=P[0], n_docs=1000, dim_pad=128, queries=P[1], nq=3, k=10, doc_base=0, filter=None, out_doc=P[2], ws=P[5],
            ws_bytes=1 << 30):
    return L.srx_mx_search(0, type, corpus, n_docs, dim_pad, queries, nq, k, doc_base, filter, out_doc, P[3], P[4], ws, ws_bytes, None, 0.0)


def _docs(L, type=0, corpus=P[0], n_docs=1000, dim_pad=128, queries=P[1], nq=3, doc_base=0, cand_doc=P[2], m=10, out=P[4]):
    return L.srx_mx_score_docs(0, type, corpus, n_docs, dim_pad, queries, nq, doc_base, cand_doc, None, m, out, None)


REFUSALS = [(_convert, {"type": 2}), (_convert, {"n_rows": -1}), (_convert, {"row0": 64, "n_rows": 100}), (_convert, {"dim_pad": 96}),
            (_convert, {"dim_pad": 1088}), (_convert, {"dim": 0}), (_convert, {"dim": 65}), (_convert, {"ld": 39}), (_convert, {"row0": 16, "n_rows": 8}),
            (_convert, {"n_rows": 2 ** 36 + 1, "n_total": 2 ** 36 + 1}), (_convert, {"emb": None}), (_convert, {"out": None}),
            (_convert, {"emb": P[0] + 2}), (_convert, {"out": P[1] + 8}),
            (_search, {"type": -1}), (_search, {"nq": -1}), (_search, {"n_docs": 0}), (_search, {"k": 0}), (_search, {"k": 1025}),
            (_search, {"dim_pad": 32}), (_search, {"doc_base": -1}), (_search, {"doc_base": 2 ** 31 - 1001}), (_search, {"corpus": None}),
            (_search, {"out_doc": None}), (_search, {"queries": P[1] + 4}), (_search, {"corpus": P[0] + 8}),
            (_search, {"filter": ctypes.byref(_capi.DocFilterDesc(bits=None, n_filters=1, q_filter=None))}),
            (_search, {"filter": ctypes.byref(_capi.DocFilterDesc(bits=P[6], n_filters=0, q_filter=None))}),
            (_docs, {"type": 2}), (_docs, {"dim_pad": 1088}), (_docs, {"nq": -1}), (_docs, {"m": 0}), (_docs, {"nq": 2 ** 20, "m": 2 ** 11}),
            (_docs, {"n_docs": 0}), (_docs, {"n_docs": 2 ** 31 - 1}), (_docs, {"doc_base": -1}), (_docs, {"cand_doc": None}), (_docs, {"queries": P[1] + 8})]


@pytest.mark.parametrize("call,kw", REFUSALS, ids=[f"{c.__name__}-{'-'.join(k)}-{i}" for i, (c, k) in enumerate(REFUSALS)])
def test_refusals_fire_before_a_device_is_touched(call, kw):
    L = _capi.lib()
    assert call(L, **kw) == -1
    assert L.srx_last_error().startswith(b"srx_mx_") and len(L.srx_last_error()) > 20


def test_nomem_and_empty_calls():
    L = _capi.lib()
    assert _search(L, ws=None) == -3 and _search(L, ws_bytes=L.srx_mx_workspace_bytes(3, 1000, 10) - 1) == -3
    assert _search(L, nq=0, corpus=None, queries=None, ws=None, ws_bytes=0) == 0 and _docs(L, nq=0, corpus=None, cand_doc=None) == 0
    assert _convert(L, n_rows=0, emb=None, out=None) == 0
    assert L.srx_mx_bytes(2, 1, 64) == -1 and L.srx_mx_bytes(0, -1, 64) == -1 and L.srx_mx_bytes(0, 1, 96) == -1
    assert L.srx_mx_workspace_bytes(1, 0, 1) == -1


@pytest.mark.parametrize("dtype", list(ref.TYPES))
def test_reference_quantiser_keeps_representable_values(dtype):
    vals = ref.VALUES[dtype]
    assert len(vals) == {"mxfp8": 127, "mxfp4": 8}[dtype] and vals[-1] == {"mxfp8": 448.0, "mxfp4": 6.0}[dtype]
    for shift in (0, -110, 100):  # every value of the format, both signs, under three block scales (unclamped); the maximum pins the scale
        x = np.ldexp(np.concatenate([vals, -vals, [vals[-1]]]), shift).astype(np.float32)
        x = np.pad(x, (0, -len(x) % 32))
        x = np.stack([np.concatenate([blk[:31], [np.ldexp(vals[-1], shift)]]) for blk in x.reshape(-1, 32)]).reshape(1, -1).astype(np.float32)
        codes, scales, flag = ref.quantize(x, dtype, ref.pad64(x.shape[1]))
        assert flag == 0 and np.array_equal(ref.dequant(codes, scales, dtype)[:, : x.shape[1]], x.astype(np.float64))
        assert not ((codes & (ref.SIGN[dtype] - 1)) == 0)[codes >= ref.SIGN[dtype]].any()  # no negative zero


def test_reference_e4m3_rounding_is_torchs():
    rng = np.random.default_rng(7)
    a = np.abs(rng.standard_normal(20000) * np.exp2(rng.integers(-12, 9, 20000))).astype(np.float32)
    a = np.minimum(np.concatenate([a, ((ref.VALUES["mxfp8"][:-1] + ref.VALUES["mxfp8"][1:]) / 2).astype(np.float32)]), np.float32(448.0))
    want = torch.from_numpy(a).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(ref.round_codes(a.astype(np.float64), "mxfp8"), want)


def test_service_refusals():
    svc = sparse_rx.RetrievalService()
    e = np.zeros((4, 8), np.float32)
    with pytest.raises(ValueError, match="screen='binary' is not offered with storage='mxfp8'"):
        svc.set_embeddings(e, storage="mxfp8", screen="binary")
    with pytest.raises(ValueError, match="storage must be"):
        svc.set_embeddings(e, storage="mxfp6")
    with pytest.raises(ValueError, match="'f16' or 'bf16'"):
        svc.set_token_embeddings({}, storage="mxfp8")
    assert getattr(svc, "_dense", None) is None
    svc.close()
